#!/usr/bin/env python3
"""Measure expected mutations per transcript by coding consequence (kp_spec_coding, kp_coding.h)
next to the scan it extends.

Input: the synthetic genome of tools/spectrum_bench.py (2^LOG2 bases, eight contigs) and its
six-type 9-mer model, as tools/null_bench.py, and a synthetic annotation of TRANSCRIPTS
transcripts of SEGMENTS segments of 100 .. 200 bases with introns of 500 .. 5,000 bases, on both
strands at random places (they may overlap).

Measured, after one run that allocates, as the median of REPS runs over every contig:
  * kp_spec_coding: the scan kernel (HIP events, summed over the contigs) and the wall-clock of the
    calls, upload of the contig and read-back of the counters and sums included;
  * the yardstick, in the same process and session: kp_spec_regions over the same segments given
    as regions -- the same loads and gathers without the codon work, the splice intervals and the
    counters per class;
  * once: the host session (one core) on the first HOST_TX transcripts of the first contig, and
    whether the device gives the same.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/coding_bench.py --out profiles/coding/mi355x.json
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

KNOBS = ("KP_CODING_GRID", "KP_CODING_GLOBAL", "KP_CODING_LDS_P", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
SEED = 2027
TRANSCRIPTS = 20_000
SEGMENTS = 9
HOST_TX = 200


def annotation(contigs, n_tx):
    """Per contig a share of ``n_tx`` transcripts ``(strand, segments)`` proportional to its length."""
    rng = np.random.RandomState(SEED)
    total = sum(s.shape[0] for _, s in contigs)
    out = []
    for _, seq in contigs:
        txs = []
        for _ in range(max(1, n_tx * seq.shape[0] // total)):
            lens = rng.randint(100, 201, size=SEGMENTS)
            lens[-1] += (-int(lens.sum())) % 3
            gaps = rng.randint(500, 5001, size=SEGMENTS - 1)
            at = int(rng.randint(0, seq.shape[0] - int(lens.sum() + gaps.sum())))
            segs = []
            for x, g in zip(lens.tolist(), gaps.tolist() + [0]):
                segs.append((at, at + x))
                at += x + g
            txs.append((int(rng.randint(0, 2)), segs))
        out.append(txs)
    return out


def coding_run(s, model, contigs, ann, splice):
    scan_ms = wall = 0.0
    items = positions = pairs = 0
    check = 0
    for (name, seq), txs in zip(contigs, ann):
        t0 = time.perf_counter()
        _, other, exp = s.spec_coding(seq, txs, splice, model.rates, want_hist=False)
        wall += time.perf_counter() - t0
        st = s.spec_coding_stats()
        scan_ms += st["scan_ms"]
        items += st["items"]
        positions += st["positions"]
        pairs += st["pairs"]
        check += int(other.sum(dtype=np.uint64)) + int(exp.view(np.uint64).sum(dtype=np.uint64) % (1 << 40))
    return {"scan_ms": scan_ms, "wall_s": wall, "items": items, "positions": positions, "pairs": pairs,
            "path": st["path"], "check": check}


def yardstick_run(s, model, contigs, ann):
    """kp_spec_regions over the same segments as regions."""
    before = s.spec_stats()
    wall = 0.0
    check = 0
    for (name, seq), txs in zip(contigs, ann):
        reg = np.array([seg for _, segs in txs for seg in segs], np.uint64)
        t0 = time.perf_counter()
        _, other, exp = s.spec_regions(seq, reg, model.rates, want_hist=False)
        wall += time.perf_counter() - t0
        check += int(other.sum(dtype=np.uint64)) + int(exp.view(np.uint64).sum(dtype=np.uint64) % (1 << 40))
    after = s.spec_stats()
    return {"scan_ms": after["scan_ms"] - before["scan_ms"], "wall_s": wall, "items": after["items"] - before["items"],
            "path": after["path"], "check": check}


def median_of(runs, keys):
    out = {k: round(statistics.median(r[k] for r in runs), 4) for k in keys}
    out.update({k: v for k, v in runs[-1].items() if k not in keys and k != "check"})
    out["same_result_every_run"] = len({r["check"] for r in runs}) == 1
    return out


def child(log2, reps, n_tx, splice):
    from kmerpapa_amd import engine, spectrum
    for key in KNOBS:
        os.environ.pop(key, None)
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag(), "reps": reps, "splice": splice}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    dev = engine.get_device(engine.visible_devices()[0])
    sites = with_alts(contigs, synthetic_sites(contigs, 2_000_000))
    parts = fit_model(dev, contigs, sites)
    model = spectrum.Model.from_partitions({kind: (n, [(0, 0)] * len(n), r) for kind, (n, r) in parts.items()})
    ann = annotation(contigs, n_tx)
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs), k=model.k, patterns=len(model.names),
               transcripts=sum(len(t) for t in ann), segments=sum(len(segs) for t in ann for _, segs in t),
               cds_bases=sum(e - b for t in ann for _, segs in t for b, e in segs), setup_s=round(time.perf_counter() - t0, 2))
    print(json.dumps(out), file=sys.stderr, flush=True)
    with spectrum.session(model, True) as s:
        runs = [yardstick_run(s, model, contigs, ann) for _ in range(reps + 1)][1:]
        out["yardstick_regions"] = median_of(runs, ("scan_ms", "wall_s"))
        out["yardstick_regions"]["first_check"] = runs[0]["check"]
        print(json.dumps({"yardstick_regions": out["yardstick_regions"]["scan_ms"]}), file=sys.stderr, flush=True)
        runs = [coding_run(s, model, contigs, ann, splice) for _ in range(reps + 1)][1:]
        out["coding"] = median_of(runs, ("scan_ms", "wall_s"))
        out["coding"]["pairs_per_s"] = round(out["coding"]["pairs"] / (out["coding"]["scan_ms"] * 1e-3), 0)
        print(json.dumps(out["coding"]), file=sys.stderr, flush=True)
        runs = [coding_run(s, model, contigs, ann, 0) for _ in range(reps + 1)][1:]
        out["coding_without_splice"] = median_of(runs, ("scan_ms", "wall_s"))
        out["scan_ratio_coding_over_regions"] = round(out["coding"]["scan_ms"] / out["yardstick_regions"]["scan_ms"], 3)
        out["scan_ratio_without_splice"] = round(out["coding_without_splice"]["scan_ms"] / out["yardstick_regions"]["scan_ms"], 3)
        out["wall_ratio_coding_over_regions"] = round(out["coding"]["wall_s"] / out["yardstick_regions"]["wall_s"], 3)
        # a yardstick call after the coding calls: the session's table is intact
        first_check = out["yardstick_regions"].pop("first_check")
        out["yardstick_after_same"] = yardstick_run(s, model, contigs, ann)["check"] == first_check
        seq, txs = contigs[0][1], ann[0][:HOST_TX]
        dres = s.spec_coding(seq, txs, splice, model.rates)
    host = engine.HostSpec()
    host.spec_begin(model.k, model.words(), model.ptype, True)
    try:
        t0 = time.perf_counter()
        hres = host.spec_coding(seq, txs, splice, model.rates)
        sec = time.perf_counter() - t0
        pairs = host.spec_coding_stats()["pairs"]
    finally:
        host.spec_end()
    out["host_one_core"] = {"transcripts": len(txs), "pairs": pairs, "seconds": round(sec, 4),
                            "ns_per_pair": round(sec * 1e9 / max(pairs, 1), 2),
                            "equals_device": all(h.tobytes() == d.tobytes() for h, d in zip(hres, dres))}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--transcripts", type=int, default=TRANSCRIPTS)
    ap.add_argument("--splice", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=500, help="time limit of the measuring process, seconds")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2, a.reps, a.transcripts, a.splice)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2), "--reps", str(a.reps),
           "--transcripts", str(a.transcripts), "--splice", str(a.splice)]
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
