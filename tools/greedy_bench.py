#!/usr/bin/env python3
"""Measure the greedy top-down partition (kp_greedy) on the benchmark's seeded synthetic
counts (bench.synthetic_counts' distributions and seed).

Runs (each GPU step in a child process of its own under its own time limit; after a step
that fails or times out nothing more is started):
  a   9-mer NNNNMNNNN: 5 x 5 grid, 5-fold greedy CV (125 lanes, one job) + the greedy fit
  b   unrestricted 11-mer NNNNNNNNNNN (4.2e6 k-mers; a lattice the DP refuses): same grid
  c   13-mer NNNNNNNNNNNNN (6.7e7 k-mers): the greedy fit only
  host   kp_greedy_host on this machine's CPU for run a (the serial baseline)
  ref    with --reference: the reference's own greedy fit on its 7-mer test data under
         the identity stand-in for numba.njit (only where the reference is installed)

Reported per run: wall-clock of the fold split, the CV job and the fit; the histogram
kernel's device time and its rate against the 8 TB/s HBM peak, counting 16 bytes per
frontier k-mer per depth (kp_greedy_last_stats); tree depth and leaf counts.

Usage: python tools/greedy_bench.py --runs a,b,c,host --out profiles/greedy/mi355x.json
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ALPHAS = [0.5, 1.0, 2.0, 5.0, 10.0]
PENALTIES = [3.0, 4.0, 5.0, 6.0, 7.0]
NFOLDS = 5
PEAK_HBM_GBS = 8000.0
RUNS = {"a": ("NNNNMNNNN", True, 240), "b": ("NNNNNNNNNNN", True, 420), "c": ("NNNNNNNNNNNNN", False, 420),
        "host": ("NNNNMNNNN", True, 1200)}


def synthetic_table(gen_pat, seed=9):
    """bench.synthetic_counts' counts as the ``[n, 2]`` (M, U) table in matches(gen_pat) order,
    with the k-mers' letters taken from the row index instead of a list of strings."""
    from kmerpapa_amd.pattern_utils import code, generality
    rng = np.random.RandomState(seed)
    n = generality(gen_pat)
    bg = rng.poisson(rng.lognormal(math.log(1.5e4), 0.8, size=n))
    f = {"A": 0.6, "C": 1.0, "G": 1.8, "T": 0.8}
    idx = np.arange(n, dtype=np.int64)
    mid = len(gen_pat) // 2
    fl = np.ones(n)
    w = 1
    for i, g in enumerate(gen_pat):
        r = len(code[g])
        if i in (mid - 1, mid + 1):
            fl *= np.array([f[x] for x in code[g]])[(idx // w) % r]
        w *= r
    rate = 2.7e-5 * fl * rng.lognormal(0.0, 0.3, size=n)
    pos = rng.binomial(bg, np.minimum(rate, 1.0))
    return np.stack([pos, bg - pos], axis=1).astype(np.uint64)


def _lanes(table, folds):
    """Lanes of the 5 x 5 grid's CV over one repeat's fold tables, as the drop-in module builds them."""
    from kmerpapa_amd.score_utils import get_betas
    M = np.ascontiguousarray(folds[:, :, 0].T)
    U = np.ascontiguousarray(folds[:, :, 1].T)
    trM = M.sum() - M.sum(axis=0)
    trU = U.sum() - U.sum(axis=0)
    lanes = []
    for a in ALPHAS:
        for c in PENALTIES:
            for f in range(NFOLDS):
                lanes.append((f, len(lanes) // NFOLDS, a, get_betas(a, trM[f], trU[f]), c))
    return M, U, lanes


def _rate(st):
    gbs = st["frontier_kmers"] * 16 / (st["hist_ms"] * 1e-3) / 1e9 if st["hist_ms"] > 0 else 0.0
    return {"hist_ms": round(st["hist_ms"], 3), "call_ms": round(st["total_ms"], 3),
            "frontier_kmers": st["frontier_kmers"], "items": st["items"], "depths": st["depths"],
            "batches": st["batches"], "hist_GBps": round(gbs, 1), "hist_pct_of_peak": round(100 * gbs / PEAK_HBM_GBS, 2)}


def child(run):
    from kmerpapa_amd import engine
    from kmerpapa_amd.CV_tools import make_all_folds
    from kmerpapa_amd.score_utils import get_betas
    gen_pat, with_cv, _ = RUNS[run]
    out = {"run": run, "gen_pat": gen_pat, "kernel_tag": engine.kernel_tag()}
    t0 = time.perf_counter()
    table = synthetic_table(gen_pat)
    out["n_kmers"] = int(table.shape[0])
    out["synthetic_s"] = round(time.perf_counter() - t0, 3)
    MU = table.sum(axis=0)
    fit_lane = [(-1, -1, 1.0, get_betas(1.0, MU[0], MU[1]), 5.0)]
    if run == "host":
        t0 = time.perf_counter()
        folds = make_all_folds(table, NFOLDS, 1, np.random.RandomState(1))[0]
        M, U, lanes = _lanes(table, folds)
        t1 = time.perf_counter()
        loss, chain, nl, _ = engine.greedy_host(gen_pat, M, U, lanes, NFOLDS)
        t2 = time.perf_counter()
        engine.greedy_host(gen_pat, table[:, 0], table[:, 1], fit_lane)
        t3 = time.perf_counter()
        out.update(fold_split_s=round(t1 - t0, 3), cv_s=round(t2 - t1, 3), fit_s=round(t3 - t2, 3),
                   total_s=round(t3 - t0, 3), cv_leaves_min=int(nl.min()), cv_leaves_max=int(nl.max()),
                   chain0_hex=float(chain[0]).hex())
        print(json.dumps(out), flush=True)
        return
    dev = engine.get_device(engine.visible_devices()[0])
    out["passes"] = []
    for rep in range(2):  # the first pass allocates the device arena, the second reuses it
        rec = {}
        t0 = time.perf_counter()
        if with_cv:
            folds = make_all_folds(table, NFOLDS, 1, np.random.RandomState(1))[0]
            M, U, lanes = _lanes(table, folds)
            t1 = time.perf_counter()
            loss, chain, nl = dev.greedy(gen_pat, M, U, lanes, NFOLDS)
            t2 = time.perf_counter()
            grid = [float(x) for x in chain]
            rec.update(fold_split_s=round(t1 - t0, 3), cv_s=round(t2 - t1, 3), cv=_rate(dev.greedy_stats()),
                       cv_leaves_min=int(nl.min()), cv_leaves_max=int(nl.max()), best_point=int(np.argmin(grid)),
                       chain0_hex=float(chain[0]).hex())
        t2 = time.perf_counter()
        loss, _, nl = dev.greedy(gen_pat, table[:, 0], table[:, 1], fit_lane)
        t3 = time.perf_counter()
        rec.update(fit_s=round(t3 - t2, 3), fit=_rate(dev.greedy_stats()), fit_leaves=int(nl[0]),
                   fit_loss_hex=float(loss[0]).hex(), total_s=round(t3 - t0, 3))
        out["passes"].append(rec)
    print(json.dumps(out), flush=True)


def reference_fit():
    """The reference's greedy_partition on its 7-mer test data under the identity stand-in
    for numba.njit, timed in a child interpreter (the serial Python baseline)."""
    gold = os.path.join(ROOT, "tests", "golden")
    code_ = ("import sys, time, tempfile; sys.path.insert(0, %r); import make_golden as mg\n"
             "tmp = tempfile.mkdtemp(); mg.make_shim(tmp); sys.path[:0] = [tmp, mg.REF_SRC]\n"
             "import kmerpapa.algorithms.greedy_penalty_plus_pseudo as gm\n"
             "ctx, gp, nu, nm = mg._context(7)\n"
             "t0 = time.perf_counter(); r = gm.greedy_partition(gp, ctx, 0.5, None, 6.0, None)\n"
             "print(time.perf_counter() - t0, len(r[3]))\n") % gold
    p = subprocess.run([sys.executable, "-c", code_], capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, PYTHONWARNINGS="ignore"))
    if p.returncode:
        return {"run": "ref", "error": p.stderr[-400:]}
    secs, leaves = p.stdout.split()[-2:]
    return {"run": "ref", "what": "reference greedy_partition, 7-mer test data, alpha 0.5, c 6, numba stand-in",
            "fit_s": round(float(secs), 3), "leaves": int(leaves)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="a,host")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--reference", action="store_true", help="also time the reference's own fit (7-mers)")
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    results = []
    rc = 0
    for run in a.runs.split(","):
        limit = RUNS[run][2]
        t0 = time.perf_counter()
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", run], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            results.append({"run": run, "error": f"time limit of {limit} s"})
            rc = 1
            break  # nothing more is started after a step that hung
        if p.returncode:
            results.append({"run": run, "error": p.stderr[-800:], "returncode": p.returncode})
            rc = 1
            break
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        rec["process_s"] = round(time.perf_counter() - t0, 3)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if a.reference and rc == 0:
        results.append(reference_fit())
        print(json.dumps(results[-1]), flush=True)
    doc = {"date": time.strftime("%Y-%m-%d"), "measured": True, "grid": {"alphas": ALPHAS, "penalties": PENALTIES,
                                                                         "nfolds": NFOLDS}, "results": results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    if rc:
        print(json.dumps(results[-1]), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
