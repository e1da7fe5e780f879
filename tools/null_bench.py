#!/usr/bin/env python3
"""Measure per-region null tables (kp_spec_null, kp_null.h) next to the loop they replace.

Input: the synthetic genome of tools/spectrum_bench.py (2^LOG2 bases, eight contigs) and its
six-type 9-mer model, as tools/simulate_bench.py.  Two region sets: one whole-contig region per
contig, and a gene-like set of GENES regions of 1 .. 5 kb at random places (they may overlap).

Measured, after one run that allocates, as the median of REPS runs over every contig:
  * kp_spec_null with R = 64, 1,024 and 10,000 replicates on both sets at scale 1: the kernel (HIP
    events, summed over the contigs) and the wall-clock of the calls, upload of the contig and
    read-back of the table included; at R = 1,024 on the whole contigs also the dense scale of
    tools/simulate_bench.py and the sparse scale 10^-3;
  * the yardstick, in the same process and session: kp_spec_simulate with cap = 0 over the same
    whole contigs -- its count and offsets kernels only, no write pass, no download of hits, no text
    -- once per replicate.  This is a lower bound on looping over ``simulate --replicate``;
  * once: the host session (one core) on the first 2^24 bases with HOST_REPS replicates, and
    whether the device gives the same table.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/null_bench.py --out profiles/null/mi355x.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.count_bench import synthetic_genome  # noqa: E402
from tools.predict_bench import synthetic_sites  # noqa: E402
from tools.simulate_bench import dense_scale  # noqa: E402
from tools.spectrum_bench import fit_model, with_alts  # noqa: E402

KNOBS = ("KP_NULL_REPS", "KP_NULL_GRID", "KP_SIM_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
SEED = 2026
GENES = 30_000
HOST_REPS = 16


def gene_regions(contigs, n_genes):
    """Per contig a share of ``n_genes`` regions of 1 .. 5 kb proportional to its length."""
    rng = np.random.RandomState(SEED)
    total = sum(s.shape[0] for _, s in contigs)
    out = []
    for _, seq in contigs:
        m = max(1, n_genes * seq.shape[0] // total)
        length = rng.randint(1000, 5001, size=m)
        begin = rng.randint(0, seq.shape[0] - 5000, size=m)
        out.append(np.stack([begin, begin + length], axis=1).astype(np.uint64))
    return out


def null_run(s, model, contigs, regions, n_reps, scale, by_type=False):
    null_ms = wall = 0.0
    hits = windows = draws = items = passes = 0
    check = 0
    for cid, ((name, seq), reg) in enumerate(zip(contigs, regions)):
        t0 = time.perf_counter()
        tab = s.spec_null(seq, reg, model.rates, SEED, cid, 0, n_reps, scale, by_type)
        wall += time.perf_counter() - t0
        st = s.spec_null_stats()
        null_ms += st["null_ms"]
        hits += st["hits"]
        windows += st["windows"]
        draws += st["draws"]
        items += st["items"]
        passes = max(passes, st["passes"])
        check += int(tab.sum(dtype=np.uint64)) + int(tab[:, -1].sum(dtype=np.uint64)) * 3
    return {"null_ms": null_ms, "wall_s": wall, "hits": hits, "windows": windows, "draws": draws, "items": items,
            "passes": passes, "check": check}


def yardstick_run(s, model, contigs, replicate, scale):
    """One replicate of the loop's cheapest part: the count and offsets pass of every contig."""
    import ctypes

    from kmerpapa_amd import engine
    count_ms = wall = 0.0
    hits = 0
    rates = np.ascontiguousarray(model.rates, np.float64)
    u64, u32, p = ctypes.c_uint64, ctypes.c_uint32, engine._ptr
    for cid, (name, seq) in enumerate(contigs):
        rb, re = np.zeros(1, np.uint64), np.full(1, seq.shape[0], np.uint64)
        n_hits = u64(0)
        t0 = time.perf_counter()
        # (the library call itself: engine's wrapper would draw again with room for the set)
        engine._check(engine.load().kp_spec_simulate(s._h, p(seq), u64(seq.shape[0]), u32(cid), p(rb), p(re), u64(1), p(rates),
                                                     ctypes.c_double(scale), u64(SEED), u32(replicate), u64(0), None, None,
                                                     None, ctypes.byref(n_hits)))
        wall += time.perf_counter() - t0
        st = s.spec_sim_stats()
        assert st["write_ms"] == 0.0
        count_ms += st["count_ms"]
        hits += n_hits.value
    return {"count_ms": count_ms, "wall_s": wall, "hits": hits}


def median_of(runs, keys):
    out = {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}
    out.update({k: v for k, v in runs[-1].items() if k not in keys and k != "check"})
    out["same_result_every_run"] = len({r["check"] for r in runs}) == 1
    return out


def child(log2, reps, sizes):
    from kmerpapa_amd import engine, spectrum
    for key in KNOBS:
        os.environ.pop(key, None)
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag(), "reps": reps}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    dev = engine.get_device(engine.visible_devices()[0])
    sites = with_alts(contigs, synthetic_sites(contigs, 2_000_000))
    parts = fit_model(dev, contigs, sites)
    model = spectrum.Model.from_partitions({kind: (n, [(0, 0)] * len(n), r) for kind, (n, r) in parts.items()})
    sets = {"whole_contigs": [np.array([(0, s.shape[0])], np.uint64) for _, s in contigs],
            "genes": gene_regions(contigs, GENES)}
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs), k=model.k, patterns=len(model.names),
               gene_regions=sum(r.shape[0] for r in sets["genes"]),
               gene_bases=int(sum((r[:, 1] - r[:, 0]).sum() for r in sets["genes"])), setup_s=round(time.perf_counter() - t0, 2))
    print(json.dumps(out), file=sys.stderr, flush=True)
    with spectrum.session(model, True) as s:
        runs = []
        for j in range(reps + 1):
            runs.append(dict(yardstick_run(s, model, contigs, j, 1.0), check=0))
        out["yardstick"] = median_of(runs[1:], ("count_ms", "wall_s"))
        del out["yardstick"]["same_result_every_run"]
        print(json.dumps(out["yardstick"]), file=sys.stderr, flush=True)
        out["null"] = {}
        cases = [(name, R, "scale_1", 1.0) for name in sets for R in sizes]
        if 1024 in sizes:
            cases += [("whole_contigs", 1024, "dense", dense_scale(model)), ("whole_contigs", 1024, "sparse", 1e-3)]
        for name, R, tag, scale in cases:
            runs = [null_run(s, model, contigs, sets[name], R, scale) for _ in range(reps + 1)][1:]
            rec = median_of(runs, ("null_ms", "wall_s"))
            rec.update(scale=scale, replicates=R, null_ms_per_replicate=round(rec["null_ms"] / R, 5),
                       yardstick_over_null_per_replicate=round(out["yardstick"]["count_ms"] / (rec["null_ms"] / R), 3),
                       draws_per_s=round(rec["draws"] / (rec["null_ms"] * 1e-3), 0))
            out["null"][f"{name}_R{R}_{tag}"] = rec
            print(json.dumps({f"{name}_R{R}_{tag}": rec}), file=sys.stderr, flush=True)
        if 1024 in sizes:
            runs = [null_run(s, model, contigs, sets["genes"], 256, 1.0, by_type=True) for _ in range(reps + 1)][1:]
            out["null"]["genes_R256_by_type"] = median_of(runs, ("null_ms", "wall_s"))
        # a yardstick call after the null calls: the session's table is intact
        out["yardstick_after_same_hits"] = yardstick_run(s, model, contigs, reps, 1.0)["hits"] == out["yardstick"]["hits"]
        # one host core on a slice, and the device on the same slice
        piece = contigs[0][1][:1 << min(24, log2 - 1)]
        reg = np.array([(0, piece.shape[0]), (piece.shape[0] // 3, piece.shape[0] // 2)], np.uint64)
        dtab = s.spec_null(piece, reg, model.rates, SEED, 0, 0, HOST_REPS)
    host = engine.HostSpec()
    host.spec_begin(model.k, model.words(), model.ptype, True)
    try:
        t0 = time.perf_counter()
        htab = host.spec_null(piece, reg, model.rates, SEED, 0, 0, HOST_REPS)
        sec = time.perf_counter() - t0
        draws = host.spec_null_stats()["draws"]
    finally:
        host.spec_end()
    out["host_one_core"] = {"bases": int(piece.shape[0]), "replicates": HOST_REPS, "seconds": round(sec, 3), "draws": draws,
                            "ns_per_draw": round(sec * 1e9 / max(draws, 1), 2), "equals_device": htab.tobytes() == dtab.tobytes()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 10000], help="replicates per call")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2, a.reps, a.sizes)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2), "--reps", str(a.reps), "--sizes"]
    cmd += [str(x) for x in a.sizes]
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
    except subprocess.TimeoutExpired:
        print(f"time limit of {a.limit} s", file=sys.stderr)
        return 1
    if p.returncode:
        return p.returncode
    doc = {"date": time.strftime("%Y-%m-%d"), "measured": True, "result": json.loads(p.stdout.strip().splitlines()[-1])}
    print(json.dumps(doc["result"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
