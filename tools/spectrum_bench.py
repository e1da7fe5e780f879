#!/usr/bin/env python3
"""Measure the whole mutation spectrum in one genome pass (kp_spec_*, kmerpapa_amd.spectrum)
against today's way: six kp_pred sessions, one per mutation type.

Input: the synthetic genome and mutations of tools/predict_bench.py (2^LOG2 bases, eight contigs,
about 2 * 10^6 sites); every site gets a random ALT other than its base.  The six-type 9-mer model
is one greedy partition per type (Device.greedy under NNNNANNNN / NNNNCNNNN on the typed count
tables, as predict_bench fits its one partition); the 13-mer model is the same patterns with NN
added on both sides, over a 4^13-entry table.

Measured per k, after one warm-up session that allocates, as the median of REPS sessions, over
whole contigs, 100-kb tiles and about 200,000 exon-like regions:
  * the spectrum session: table build (HIP events), scan kernel time, wall-clock of the calls;
  * the same for six kp_pred sessions, one per type's partition, run one after the other in the
    same process on the same genome, summed.  This is the yardstick.
And once: typed counting of the sites (one kp_seq_sites_typed per contig) against six
kp_seq_sites passes over the sites filtered to one type each, wall-clock.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/spectrum_bench.py --out profiles/spectrum/mi355x.json
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
from tools.predict_bench import BUDGET, shapes, synthetic_sites  # noqa: E402

KNOBS = ("KP_PRED_GLOBAL", "KP_PRED_LDS_P", "KP_PRED_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")


def with_alts(contigs, sites, seed=13):
    """{contig: (pos, alt)}: a random base other than the one at the site (any base at an invalid byte)."""
    rng = np.random.RandomState(seed)
    digit = np.full(256, 0, np.int64)
    for i, ch in enumerate(b"ACGT"):
        digit[ch] = digit[ch | 0x20] = i
    out = {}
    for name, seq in contigs:
        pos = sites[name]
        alt = (digit[seq[pos.astype(np.intp)]] + rng.randint(1, 4, size=pos.shape[0])) % 4
        out[name] = (pos, np.frombuffer(b"ACGT", np.uint8)[alt])
    return out


def fit_model(dev, contigs, sites):
    """One greedy 9-mer partition per type: {type: (names sorted, rates)}."""
    from kmerpapa_amd import engine, score_utils, spectrum
    from kmerpapa_amd.papa import PatternPartition
    alpha, penalty = 2.0, 4.0
    parts = {}
    for kind, table in spectrum.count_tables(contigs, 9, sites=sites).items():
        gp = spectrum.super_pattern(kind, 9)
        full = table.zero_filled(gp)
        _, M, U = full.match_rows(gp)
        beta = score_utils.get_betas(alpha, int(sum(M)), int(sum(U)))
        dev.greedy(gp, np.array(M, np.uint64), np.array(U, np.uint64), [(-1, -1, alpha, beta, penalty)])
        names = sorted(engine.word_pattern(w, 9) for w in dev.greedy_leaves(0))
        counts = PatternPartition(list(names), superPattern=gp).counts(full)
        parts[kind] = (names, [(m + 0.5) / (m + u + 1.0) for m, u in counts])
    return parts


def spec_session(dev, model, contigs, regions):
    from kmerpapa_amd import spectrum
    t0 = time.perf_counter()
    calls, check = 0.0, 0.0
    with spectrum.session(model, True) as s:
        for name, seq in contigs:
            t1 = time.perf_counter()
            _, _, exp = spectrum._contig_regions(s, seq, regions[name], len(model.names), model.rates, False, BUDGET)
            calls += time.perf_counter() - t1
            check += float(exp.sum())
        st = s.spec_stats()
    return st, calls, time.perf_counter() - t0, check


def pred_sessions(dev, parts, contigs, regions):
    """The six single-type sessions one after the other: their figures summed."""
    from kmerpapa_amd import predict
    t0 = time.perf_counter()
    st = {"scan_ms": 0.0, "lut_ms": 0.0, "lut_bytes": 0, "items": 0}
    calls, check = 0.0, 0.0
    for names, rates in parts.values():
        with predict.session(names, True) as s:
            for name, seq in contigs:
                t1 = time.perf_counter()
                _, _, exp = predict._contig_regions(s, seq, regions[name], len(names), rates, False, BUDGET)
                calls += time.perf_counter() - t1
                check += float(exp.sum())
            one = s.pred_stats()
        for key in st:
            st[key] += one[key]
    return st, calls, time.perf_counter() - t0, check


def measure(run, reps=3):
    for key in KNOBS:
        os.environ.pop(key, None)
    runs = [run() for _ in range(reps + 1)][1:]  # the first allocates
    st = runs[-1][0]
    return {"kernel_ms": round(statistics.median(r[0]["scan_ms"] for r in runs), 3),
            "calls_s": round(statistics.median(r[1] for r in runs), 4),
            "session_s": round(statistics.median(r[2] for r in runs), 4),
            "lut_ms": round(statistics.median(r[0]["lut_ms"] for r in runs), 3), "lut_bytes": st["lut_bytes"],
            "items": st["items"], "same_result_every_run": len({r[3] for r in runs}) == 1, "checksum": runs[-1][3]}


def counting(dev, contigs, sites, k=9, reps=3):
    """Wall-clock of counting the sites: one typed session against six plain ones."""
    from kmerpapa_amd import spectrum
    digit = np.full(256, 4, np.int64)
    for i, ch in enumerate(b"ACGT"):
        digit[ch] = digit[ch | 0x20] = i
    by_type = {t: {} for t in range(6)}
    for name, seq in contigs:
        pos, alt = sites[name]
        r, a = digit[seq[pos.astype(np.intp)]], digit[alt]
        flip = (r >= 2) & (r < 4)
        r, a = np.where(flip, 3 - r, r), np.where(flip, 3 - a, a)
        t = np.where(r < 2, 3 * r + np.where(a < r, a, a - 1), -1)
        for x in range(6):
            by_type[x][name] = pos[t == x]
    typed, plain = [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        pos3, _, st3 = dev.seq_count_typed(k, True, [(seq, False, sites[name]) for name, seq in contigs])
        typed.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        cols = [dev.seq_count(k, True, [(seq, False, by_type[x][name]) for name, seq in contigs])[0] for x in range(6)]
        plain.append(time.perf_counter() - t0)
    equal = all(np.array_equal(spectrum.type_column(k, pos3, kind), cols[x]) for x, kind in enumerate(spectrum.TYPES(True)))
    return {"k": k, "sites": int(st3["sites"]), "typed_session_s": round(statistics.median(typed[1:]), 4),
            "six_plain_sessions_s": round(statistics.median(plain[1:]), 4), "equal": bool(equal)}


def child(log2):
    from kmerpapa_amd import engine, spectrum
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag()}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    dev = engine.get_device(engine.visible_devices()[0])
    sites = with_alts(contigs, synthetic_sites(contigs, 2_000_000))
    parts9 = fit_model(dev, contigs, sites)
    reg = shapes(contigs)
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs),
               patterns={kind: len(p[0]) for kind, p in parts9.items()}, setup_s=round(time.perf_counter() - t0, 2),
               regions={key: int(sum(v.shape[0] for v in r.values())) for key, r in reg.items()})
    print(json.dumps(out), file=sys.stderr, flush=True)
    out["counting"] = counting(dev, contigs, sites)
    print(json.dumps(out["counting"]), file=sys.stderr, flush=True)
    out["runs"] = []
    for k in (9, 13):
        pad = "N" * ((k - 9) // 2)
        parts = {kind: ([pad + x + pad for x in names], rates) for kind, (names, rates) in parts9.items()}
        model = spectrum.Model.from_partitions({kind: (n, [(0, 0)] * len(n), r) for kind, (n, r) in parts.items()})
        rec = {"k": k, "patterns": len(model.names)}
        for shape in ("whole", "tiles_100kb", "exons_150b"):
            one = measure(lambda: spec_session(dev, model, contigs, reg[shape]))
            six = measure(lambda: pred_sessions(dev, parts, contigs, reg[shape]))
            rec[shape] = {"spectrum": one, "six_pred_sessions": six,
                          "kernel_ratio_six_over_one": round(six["kernel_ms"] / one["kernel_ms"], 3),
                          "calls_ratio_six_over_one": round(six["calls_s"] / one["calls_s"], 3),
                          "same_expected_total": abs(one["checksum"] - six["checksum"]) <= 1e-9 * abs(six["checksum"])}
        out["runs"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2)]
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
