#!/usr/bin/env python3
"""Measure null tables per transcript by coding consequence (kp_spec_coding_null, kp_cnull.h) next
to the two calls whose work it unites.

Input: the synthetic genome of tools/spectrum_bench.py (2^LOG2 bases, eight contigs) and its
six-type 9-mer model, and the synthetic annotation of tools/coding_bench.py (TRANSCRIPTS transcripts
of nine segments on both strands, ``splice`` = 2).

Measured, after one run that allocates, as the median of REPS runs over every contig:
  * kp_spec_coding_null with R = 64, 1,024 and 10,000 replicates: the stage and the draw kernel
    (HIP events, summed over the contigs) and the wall-clock of the calls, upload of the contig and
    read-back of the table included;
  * the yardstick, in the same process and session -- the two calls whose work the new one unites:
    kp_spec_coding over the same annotation (its scan kernel; it does not depend on R), and
    kp_spec_null with the same R over the same segments and splice intervals given as regions (its
    kernel).  The null call's table is five times the new call's at 25 regions a transcript, so
    its runs are YARD_REPS after one that allocates;
  * once: the host session (one core) on the first HOST_TX transcripts of the first contig with
    HOST_REPS replicates, and whether the device gives the same table.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/coding_null_bench.py --out profiles/coding_null/mi355x.json
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

from tools.coding_bench import TRANSCRIPTS, annotation, coding_run  # noqa: E402
from tools.count_bench import synthetic_genome  # noqa: E402
from tools.predict_bench import synthetic_sites  # noqa: E402
from tools.spectrum_bench import fit_model, with_alts  # noqa: E402

KNOBS = ("KP_CNULL_REPS", "KP_CNULL_GRID", "KP_CODING_GRID", "KP_CODING_GLOBAL", "KP_CODING_LDS_P", "KP_NULL_REPS",
         "KP_NULL_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
SEED = 2028
HOST_TX = 200
HOST_REPS = 16
SIMULATE_COUNT_MS = 9.47  # the count pass of one `simulate` call over the genome


def regions_of(txs, splice):
    """The segments and splice intervals of the transcripts as kp_spec_null regions."""
    reg = []
    for _, segs in txs:
        reg += segs
        for (_, a), (b, _) in zip(segs[:-1], segs[1:]):
            first = (a, min(a + splice, b))
            second = (max(b - splice, first[1]), b)
            reg += [iv for iv in (first, second) if iv[1] > iv[0]]
    return np.array(reg, np.uint64).reshape(-1, 2)


def cnull_run(s, model, contigs, ann, splice, n_reps):
    stage_ms = draw_ms = wall = 0.0
    tot = {"positions": 0, "drawing": 0, "hits": 0, "unclassed": 0}
    check = passes = 0
    for cid, ((name, seq), txs) in enumerate(zip(contigs, ann)):
        t0 = time.perf_counter()
        tab = s.spec_coding_null(seq, txs, model.rates, SEED, cid, 0, n_reps, 1.0, splice)
        wall += time.perf_counter() - t0
        st = s.spec_coding_null_stats()
        stage_ms += st["stage_ms"]
        draw_ms += st["draw_ms"]
        passes = max(passes, st["passes"])
        for key in tot:
            tot[key] += st[key]
        check += int(tab.sum(dtype=np.uint64)) + int(tab[:, -1].sum(dtype=np.uint64)) * 3 + st["unclassed"] * 7
        del tab
    return dict(tot, stage_ms=stage_ms, draw_ms=draw_ms, kernel_ms=stage_ms + draw_ms, wall_s=wall, passes=passes, check=check)


def null_run(s, model, contigs, regions, n_reps):
    null_ms = wall = 0.0
    hits = draws = items = check = 0
    for cid, ((name, seq), reg) in enumerate(zip(contigs, regions)):
        t0 = time.perf_counter()
        tab = s.spec_null(seq, reg, model.rates, SEED, cid, 0, n_reps, 1.0)
        wall += time.perf_counter() - t0
        st = s.spec_null_stats()
        null_ms += st["null_ms"]
        hits += st["hits"]
        draws += st["draws"]
        items += st["items"]
        check += st["hits"]
        del tab
    return {"null_ms": null_ms, "wall_s": wall, "hits": hits, "draws": draws, "items": items, "check": check}


def median_of(runs, keys):
    out = {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}
    out.update({k: v for k, v in runs[-1].items() if k not in keys and k != "check"})
    out["same_result_every_run"] = len({r["check"] for r in runs}) == 1
    return out


def child(log2, reps, yard_reps, n_tx, splice, sizes):
    from kmerpapa_amd import engine, spectrum
    for key in KNOBS:
        os.environ.pop(key, None)
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag(), "reps": reps, "yardstick_reps": yard_reps, "splice": splice}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    dev = engine.get_device(engine.visible_devices()[0])
    sites = with_alts(contigs, synthetic_sites(contigs, 2_000_000))
    parts = fit_model(dev, contigs, sites)
    model = spectrum.Model.from_partitions({kind: (n, [(0, 0)] * len(n), r) for kind, (n, r) in parts.items()})
    ann = annotation(contigs, n_tx)
    regions = [regions_of(txs, splice) for txs in ann]
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs), k=model.k, patterns=len(model.names),
               transcripts=sum(len(t) for t in ann), regions=sum(r.shape[0] for r in regions),
               setup_s=round(time.perf_counter() - t0, 2))
    print(json.dumps(out), file=sys.stderr, flush=True)
    with spectrum.session(model, True) as s:
        runs = [coding_run(s, model, contigs, ann, splice) for _ in range(reps + 1)][1:]
        out["yardstick_coding"] = median_of(runs, ("scan_ms", "wall_s"))
        first_check = runs[0]["check"]
        print(json.dumps({"yardstick_coding": out["yardstick_coding"]["scan_ms"]}), file=sys.stderr, flush=True)
        out["coding_null"], out["yardstick_null"] = {}, {}
        for R in sizes:
            runs = [cnull_run(s, model, contigs, ann, splice, R) for _ in range(reps + 1)][1:]
            rec = median_of(runs, ("stage_ms", "draw_ms", "kernel_ms", "wall_s"))
            draws = rec["drawing"] * R
            rec.update(replicates=R, kernel_ms_per_replicate=round(rec["kernel_ms"] / R, 5),
                       simulate_count_over_kernel_per_replicate=round(SIMULATE_COUNT_MS / (rec["kernel_ms"] / R), 2),
                       draws=draws, draws_per_s=round(draws / (rec["draw_ms"] * 1e-3), 0))
            out["coding_null"][f"R{R}"] = rec
            print(json.dumps({f"coding_null_R{R}": rec}), file=sys.stderr, flush=True)
            runs = [null_run(s, model, contigs, regions, R) for _ in range(yard_reps + 1)][1:]
            yard = median_of(runs, ("null_ms", "wall_s"))
            yard["replicates"] = R
            out["yardstick_null"][f"R{R}"] = yard
            both = yard["null_ms"] + out["yardstick_coding"]["scan_ms"]
            rec.update(yardstick_kernels_ms=round(both, 4), kernel_over_yardstick=round(rec["kernel_ms"] / both, 4),
                       same_draws_as_yardstick=yard["draws"] == draws,
                       same_hits_as_yardstick=yard["hits"] == rec["hits"] + rec["unclassed"])
            print(json.dumps({f"yardstick_null_R{R}": yard, "kernel_over_yardstick": rec["kernel_over_yardstick"]}),
                  file=sys.stderr, flush=True)
        # a coding call after the coding-null calls: the session's table is intact
        out["yardstick_after_same"] = coding_run(s, model, contigs, ann, splice)["check"] == first_check
        seq, txs = contigs[0][1], ann[0][:HOST_TX]
        dtab = s.spec_coding_null(seq, txs, model.rates, SEED, 0, 0, HOST_REPS, 1.0, splice)
        dst = s.spec_coding_null_stats()
    host = engine.HostSpec()
    host.spec_begin(model.k, model.words(), model.ptype, True)
    try:
        t0 = time.perf_counter()
        htab = host.spec_coding_null(seq, txs, model.rates, SEED, 0, 0, HOST_REPS, 1.0, splice)
        sec = time.perf_counter() - t0
        hst = host.spec_coding_null_stats()
    finally:
        host.spec_end()
    draws = hst["drawing"] * HOST_REPS
    out["host_one_core"] = {"transcripts": len(txs), "replicates": HOST_REPS, "seconds": round(sec, 4), "draws": draws,
                            "ns_per_draw": round(sec * 1e9 / max(draws, 1), 2),
                            "equals_device": htab.tobytes() == dtab.tobytes() and all(
                                hst[key] == dst[key] for key in ("positions", "drawing", "hits", "unclassed"))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick-reps", type=int, default=2, help="runs of the kp_spec_null yardstick")
    ap.add_argument("--transcripts", type=int, default=TRANSCRIPTS)
    ap.add_argument("--splice", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 1024, 10000], help="replicates per call")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=1000, help="time limit of the measuring process, seconds")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2, a.reps, a.yardstick_reps, a.transcripts, a.splice, a.sizes)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2), "--reps", str(a.reps),
           "--yardstick-reps", str(a.yardstick_reps), "--transcripts", str(a.transcripts), "--splice", str(a.splice), "--sizes"]
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
