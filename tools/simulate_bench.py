#!/usr/bin/env python3
"""Measure the draw of a mutation set from a spectrum model (kp_spec_simulate, kp_sim.h) next to
the regions scan of the same session.

Input: the synthetic genome of tools/spectrum_bench.py (2^LOG2 bases, eight contigs) and its
six-type 9-mer model (one greedy partition per type fitted to about 10^6 synthetic sites, rates
(M + 0.5) / (M + U + 1)).  Two settings of ``scale``: 1 (sparse: about one position in a thousand
mutates) and the largest power of ten the rates allow (dense).

Measured, after one warm-up that allocates, as the median of REPS runs over every whole contig:
  * simulate: the count and offsets kernels and the write kernel (HIP events, summed over the
    contigs), and the wall-clock of the calls, upload of the contig and download of the hits
    included;
  * kp_spec_regions on one whole-contig region per contig, in the same session: its scan kernel
    (HIP events) and the wall-clock of the calls.  This is the yardstick;
  * once: the host session (one core) on the first 2^24 bases, extrapolated to the genome.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/simulate_bench.py --out profiles/simulate/mi355x.json
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
from tools.spectrum_bench import fit_model, with_alts  # noqa: E402

KNOBS = ("KP_SIM_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
SEED = 2026


def dense_scale(model):
    """The largest power of ten that keeps every REF base's three largest rates at or below 1."""
    top = 0.0
    for ref in range(4):
        top = max(top, sum(float(model.rates[model.ptype == 3 * ref + s].max()) for s in range(3)
                           if np.any(model.ptype == 3 * ref + s)))
    scale = 1.0
    while top * scale * 10.0 <= 1.0:
        scale *= 10.0
    return scale


def simulate_run(s, model, contigs, scale):
    count_ms = write_ms = wall = 0.0
    hits = windows = items = 0
    check = 0
    for cid, (name, seq) in enumerate(contigs):
        t0 = time.perf_counter()
        pos, alt, pid = s.spec_simulate(seq, [(0, seq.shape[0])], model.rates, SEED, cid, 0, scale)
        wall += time.perf_counter() - t0
        st = s.spec_sim_stats()
        count_ms += st["count_ms"]
        write_ms += st["write_ms"]
        hits += st["hits"]
        windows += st["windows"]
        items += st["items"]
        check += int(pos.sum() % (1 << 61)) + int(alt.sum()) + int(pid.sum())
    return {"count_ms": count_ms, "write_ms": write_ms, "wall_s": wall, "hits": hits, "windows": windows, "items": items,
            "check": check}


def regions_run(s, model, contigs):
    before = s.spec_stats()["scan_ms"]
    wall, check = 0.0, 0.0
    for name, seq in contigs:
        t0 = time.perf_counter()
        _, _, exp = s.spec_regions(seq, [(0, seq.shape[0])], model.rates, want_hist=False)
        wall += time.perf_counter() - t0
        check += float(exp.sum())
    return {"kernel_ms": s.spec_stats()["scan_ms"] - before, "wall_s": wall, "check": check}


def median_of(runs, keys):
    out = {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}
    out.update({k: v for k, v in runs[-1].items() if k not in keys and k != "check"})
    out["same_result_every_run"] = len({r["check"] for r in runs}) == 1
    return out


def child(log2, reps):
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
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs), k=model.k, patterns=len(model.names),
               setup_s=round(time.perf_counter() - t0, 2))
    print(json.dumps(out), file=sys.stderr, flush=True)
    scales = {"sparse": 1.0, "dense": dense_scale(model)}
    with spectrum.session(model, True) as s:
        reg = [regions_run(s, model, contigs) for _ in range(reps + 1)][1:]
        out["regions"] = median_of(reg, ("kernel_ms", "wall_s"))
        print(json.dumps(out["regions"]), file=sys.stderr, flush=True)
        out["simulate"] = {}
        for tag, scale in scales.items():
            runs = [simulate_run(s, model, contigs, scale) for _ in range(reps + 1)][1:]
            rec = median_of(runs, ("count_ms", "write_ms", "wall_s"))
            rec["scale"] = scale
            rec["count_over_regions_kernel"] = round(rec["count_ms"] / out["regions"]["kernel_ms"], 3)
            out["simulate"][tag] = rec
            print(json.dumps(rec), file=sys.stderr, flush=True)
        # a regions call after the simulate calls: the session's table is intact
        out["regions_after_same"] = regions_run(s, model, contigs)["check"] == reg[-1]["check"]
    # one host core on a slice
    piece = contigs[0][1][:1 << min(24, log2 - 1)]
    host = engine.HostSpec()
    host.spec_begin(model.k, model.words(), model.ptype, True)
    try:
        rec = {"bases": int(piece.shape[0])}
        for tag, scale in scales.items():
            t0 = time.perf_counter()
            pos, _, _ = host.spec_simulate(piece, [(0, piece.shape[0])], model.rates, SEED, 0, 0, scale)
            rec[tag + "_s"] = round(time.perf_counter() - t0, 3)
            rec[tag + "_genome_s_extrapolated"] = round(rec[tag + "_s"] * out["bases"] / piece.shape[0], 1)
            dpos, _, _ = dev_slice(dev, model, piece, scale)
            rec[tag + "_equals_device"] = pos.tobytes() == dpos.tobytes()
    finally:
        host.spec_end()
    out["host_one_core"] = rec
    print(json.dumps(out), flush=True)


def dev_slice(dev, model, piece, scale):
    from kmerpapa_amd import spectrum
    with spectrum.session(model, True) as s:
        return s.spec_simulate(piece, [(0, piece.shape[0])], model.rates, SEED, 0, 0, scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=500, help="time limit of the measuring process, seconds")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2, a.reps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2), "--reps", str(a.reps)]
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
