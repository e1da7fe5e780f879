#!/usr/bin/env python3
"""Golden vectors of the greedy top-down partition (test infrastructure, run ONLY in the
build container, like make_golden.py whose stand-ins and helpers it uses).

Runs the upstream reference's ``kmerpapa.algorithms.greedy_penalty_plus_pseudo`` (v0.2.4)
under the identity stand-in for ``numba.njit`` and records data only -- losses as hex
floats, pattern names, totals, CLI text -- into ``tests/golden/greedy*.json``.

One substitution is needed for the recorded numbers to be the reference's: with numba the
reference's ``np.log`` is lowered to the C library's ``log``, but without numba it is
numpy's own float64 loop, which on this CPU is NOT the C library's (numpy 1.26: 21 % of 2e6
inputs in (0, 1) differ in the last bit).  So after importing the reference's greedy module
this script binds that module's ``np`` to a proxy whose ``log`` is ``math.log`` (the C
library's) and which forwards every other name to numpy.

Usage:  python3 tests/golden/make_golden_greedy.py [--jobs greedy_fit,greedy_grid,greedy_cli]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


class _NumpyWithLibmLog:
    """numpy, except ``log`` = the C library's (what numba compiles np.log to)."""

    def __init__(self, np):
        self._np = np

    def log(self, x):
        return math.log(x)

    def __getattr__(self, name):
        return getattr(self._np, name)


def _greedy_module():
    import numpy as np
    import kmerpapa.algorithms.greedy_penalty_plus_pseudo as gm
    gm.np = _NumpyWithLibmLog(np)
    return gm


FIT_POINTS = {5: [(0.5, 3.0), (2.0, 0.0), (1.0, 1e9)], 7: [(0.5, 6.0), (2.0, 0.0), (1.0, 1e9)]}


def job_greedy_fit(out):
    """greedy_partition (:279-293) on the 5-mer and 7-mer data at three (alpha, c) each:
    c = 0 splits down to single k-mers, c = 1e9 keeps the root whole."""
    gm = _greedy_module()
    res = {}
    for k, points in FIT_POINTS.items():
        ctx, gp, nu, nm = mg._context(k)
        fits = []
        for alpha, c in points:
            loss, M, U, names = gm.greedy_partition(gp, ctx, alpha, None, c, mg._Args(None, None))
            fits.append({"alpha": alpha, "penalty": c, "loss_hex": float(loss).hex(), "M": int(M), "U": int(U),
                         "names": list(names)})
        res[str(k)] = {"gen_pat": gp, "nmut": nm, "nunmut": nu, "fits": fits}
    with open(os.path.join(out, "greedy_fit.json"), "w") as fh:
        json.dump(res, fh)


def job_greedy_grid(out):
    """GridSearchCV (:338-353) on the 5-mers: the 2 x 2 grid at nfolds 2 and 3, nit 1 and 2,
    seed 1; every loglik value and get_best_a_c."""
    gm = _greedy_module()
    ctx, gp, nu, nm = mg._context(5)
    alphas, pens = [0.5, 2.0], [3.0, 6.0]
    runs = []
    for nf in (2, 3):
        for nit in (1, 2):
            cv = gm.GridSearchCV(gp, ctx, pens, alphas, nf, nit, 1)
            ll = [[float(cv.loglik(a, c)).hex() for c in pens] for a in alphas]
            best = cv.get_best_a_c()
            runs.append({"nfolds": nf, "nit": nit, "seed": 1, "loglik_hex": ll,
                         "best": [best[0], best[1], float(best[2]).hex()]})
    with open(os.path.join(out, "greedy_grid.json"), "w") as fh:
        json.dump({"gen_pat": gp, "alphas": alphas, "penalties": pens, "runs": runs}, fh)


def job_greedy_cli(out):
    """CLI stdout and stderr of --greedy, --greedyCV and --greedy --test_smaller_k on the 5-mers."""
    import contextlib
    import io as _io
    _greedy_module()
    from kmerpapa import cli
    pos = os.path.join(mg.REF_DATA, "mutated_5mers.txt")
    bg = os.path.join(mg.REF_DATA, "background_5mers.txt")
    common = ["-p", pos, "-b", bg, "-a", "0.5", "2", "-c", "3", "6", "--nfolds", "2", "--seed", "1"]
    runs = {"greedy": common + ["--greedy"], "greedyCV": common + ["--greedyCV"],
            "greedy_smaller_k": common + ["--greedy", "--test_smaller_k"]}
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for name, argv in runs.items():
            o = os.path.join(td, name + ".out")
            err = _io.StringIO()
            with contextlib.redirect_stderr(err):
                rc = cli.main(argv + ["-o", o])
            res[name] = {"argv": argv, "rc": rc, "output": open(o).read(), "stderr": err.getvalue()}
    with open(os.path.join(out, "greedy_cli.json"), "w") as fh:
        json.dump(res, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="greedy_fit,greedy_grid,greedy_cli")
    ap.add_argument("--python", default=mg.CANON_PY)
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        globals()["job_" + a.child](a.out)
        return
    with tempfile.TemporaryDirectory() as tmp:
        mg.make_shim(tmp)
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=tmp + os.pathsep + mg.REF_SRC,
                   PYTHONWARNINGS="ignore")
        for job in a.jobs.split(","):
            print("golden job", job, flush=True)
            subprocess.run([a.python, os.path.abspath(__file__), "--child", job, "--out", a.out], env=env,
                           check=True, cwd=tmp)


if __name__ == "__main__":
    main()
