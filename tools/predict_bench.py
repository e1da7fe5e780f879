#!/usr/bin/env python3
"""Measure taking a fitted partition back to the genome (kp_pred_*, kmerpapa_amd.predict).

Input: the synthetic genome of tools/count_bench.py (2^LOG2 bases, default 2^30, eight contigs)
and about 2 * 10^6 synthetic mutations whose rate depends on the four bases around the site
(a factor per flanking base) and is ten times as high at CpG sites, so that the fit splits.  The 9-mer partition is
fitted on the GPU from the genome's own count table (count.count_table, Device.greedy under
NNNNMNNNN); the 13-mer one is that partition with NN added on both sides -- the same patterns
over a 4^13-entry lookup table, which is what the 13-mer run is there to measure (the gather from
a table larger than the Infinity Cache).

Measured per k, after one warm-up session that allocates, as the median of REPS sessions:
  * the lookup table: build time (HIP events) and bytes;
  * kp_seq_scan of the same genome at the same k (the yardstick: the same loads and roll, a
    global atomic per window in place of a gather and an LDS add): kernel time;
  * four shapes -- one whole-contig region per contig, 100-kb tiling windows, about 200,000
    exon-like regions of 100..200 bases, and the track of every contig: kernel time (HIP events)
    beside the wall-clock of the calls with upload and read-back;
  * the first contig whole with KP_PRED_GLOBAL=1 (global atomics in place of LDS counters).
And at k = 9 on the first contig: a one-core numpy baseline (sliding forward and reverse-complement
codes, a table gather, np.bincount) against the GPU call, with equal histograms.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/predict_bench.py --out profiles/predict/mi355x.json
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

KNOBS = ("KP_PRED_GLOBAL", "KP_PRED_LDS_P", "KP_PRED_GRID")
BUDGET = 1 << 27  # counters per regions call (predict.DEFAULT_BUDGET)


# factor of a flanking base by (byte & 7): A = 1, C = 3, G = 7, T = 4 in either case; an invalid byte 1.0
FLANK = [np.array([1.0, a, 1.0, c, t, 1.0, 1.0, g]) for a, c, g, t in
         ((1.0, 0.6, 0.8, 0.4), (0.5, 1.0, 0.3, 0.7), (0.9, 0.4, 1.0, 0.6), (0.7, 1.0, 0.5, 0.8))]


def synthetic_sites(contigs, n_sites, seed=5):
    """Positions per contig: ten times ``n_sites`` candidates over the genome, each kept with a
    probability that is a product of one factor per base at offsets -2, -1, 1 and 2 (strand
    symmetry is not modelled), times ten at a CpG."""
    rng = np.random.RandomState(seed)
    total = sum(s.shape[0] for _, s in contigs)
    out = {}
    for name, seq in contigs:
        cand = rng.randint(1, seq.shape[0] - 1, size=10 * n_sites * seq.shape[0] // total)
        b, nxt, prv = seq[cand] & 0xDF, seq[cand + 1] & 0xDF, seq[cand - 1] & 0xDF
        cpg = ((b == ord("C")) & (nxt == ord("G"))) | ((b == ord("G")) & (prv == ord("C")))
        p = np.where(cpg, 1.0, 0.1)
        for off, factor in zip((-2, -1, 1, 2), FLANK):
            p = p * factor[seq[np.clip(cand + off, 0, seq.shape[0] - 1)] & 0x7]
        out[name] = cand[rng.random_sample(cand.shape[0]) < p].astype(np.uint64)
    return out


def fit_partition(dev, contigs, sites):
    """The greedy 9-mer partition of the genome's own counts: (patterns sorted, rates)."""
    from kmerpapa_amd import count, engine, score_utils
    from kmerpapa_amd.papa import PatternPartition
    gp, alpha, penalty = "NNNNMNNNN", 2.0, 4.0
    full = count.count_table(contigs, 9, sites=sites).zero_filled(gp)
    _, M, U = full.match_rows(gp)
    beta = score_utils.get_betas(alpha, int(sum(M)), int(sum(U)))
    dev.greedy(gp, np.array(M, np.uint64), np.array(U, np.uint64), [(-1, -1, alpha, beta, penalty)])
    names = sorted(engine.word_pattern(w, 9) for w in dev.greedy_leaves(0))
    counts = PatternPartition(list(names), superPattern=gp).counts(full)
    return names, [(m + 0.5) / (m + u + 1.0) for m, u in counts]


def shapes(contigs, seed=9):
    """{shape: {contig: regions [m, 2]}}"""
    rng = np.random.RandomState(seed)
    total = sum(s.shape[0] for _, s in contigs)
    out = {"whole": {}, "tiles_100kb": {}, "exons_150b": {}}
    for name, seq in contigs:
        n = seq.shape[0]
        out["whole"][name] = np.array([(0, n)], np.uint64)
        b = np.arange(0, n, 100_000)
        out["tiles_100kb"][name] = np.stack([b, np.minimum(b + 100_000, n)], axis=1).astype(np.uint64)
        b = rng.randint(0, n - 200, size=200_000 * n // total)
        out["exons_150b"][name] = np.stack([b, b + rng.randint(100, 201, size=b.shape[0])], axis=1).astype(np.uint64)
    return out


def one_session(dev, names, rates, contigs, regions, track):
    """(stats, seconds in the calls, seconds of the session, a checksum of the results)"""
    from kmerpapa_amd import predict
    t0 = time.perf_counter()
    calls = 0.0
    check = 0.0
    with predict.session(names, True) as s:
        for name, seq in contigs:
            t1 = time.perf_counter()
            if track:
                pid = s.pred_track(seq)
                calls += time.perf_counter() - t1
                check += float((pid >= 0).sum())
            else:
                _, other, exp = predict._contig_regions(s, seq, regions[name], len(names), rates, False, BUDGET)
                calls += time.perf_counter() - t1
                check += float(exp.sum())
        st = s.pred_stats()
    assert s is dev
    return st, calls, time.perf_counter() - t0, check


def measure(dev, names, rates, contigs, regions=None, track=False, env=None, reps=3):
    for key in KNOBS:
        os.environ.pop(key, None)
    os.environ.update(env or {})
    runs = [one_session(dev, names, rates, contigs, regions, track) for _ in range(reps + 1)][1:]  # the first allocates
    for key in KNOBS:
        os.environ.pop(key, None)
    st = runs[-1][0]
    bases = sum(s.shape[0] for _, s in contigs)
    kernel_ms = statistics.median(r[0]["scan_ms"] for r in runs)
    return {"kernel_ms": round(kernel_ms, 3), "bases_per_s_kernel": bases / (kernel_ms * 1e-3) if kernel_ms > 0 else None,
            "calls_s": round(statistics.median(r[1] for r in runs), 4),
            "session_s": round(statistics.median(r[2] for r in runs), 4),
            "lut_ms": round(statistics.median(r[0]["lut_ms"] for r in runs), 3), "lut_bytes": st["lut_bytes"],
            "path": {0: "none", 1: "lds", 2: "global"}[st["path"]], "items": st["items"], "assigned": st["assigned"],
            "unmatched": st["unmatched"], "invalid": st["invalid"], "same_result_every_run": len({r[3] for r in runs}) == 1,
            "checksum": runs[-1][3]}


def seq_scan_ms(dev, k, contigs, reps=3):
    ms = []
    for _ in range(reps + 1):
        _, _, st = dev.seq_count(k, True, [(s, None, None) for _, s in contigs])
        ms.append(st["scan_ms"])
    return round(statistics.median(ms[1:]), 3)


def numpy_hist(seq, names, k=9):
    """The whole-contig histogram of one contig on one core: digits, k shifted adds for the forward
    and for the reverse-complement code, the fold, a gather from a table numpy built by matching
    every code's one-hot word against the pattern words, np.bincount.  Chunks of 2^24 windows."""
    from kmerpapa_amd import engine
    words = np.array([engine.pattern_word(x) for x in names], np.uint64)
    codes = np.arange(4 ** k, dtype=np.uint64)
    onehot = np.zeros(4 ** k, np.uint64)
    for i in range(k):
        onehot |= np.uint64(1) << (np.uint64(4 * i) + ((codes >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)))
    table = np.full(4 ** k, -1, np.int32)
    for j, w in enumerate(words):
        table[(onehot & ~w) == 0] = j
    digit = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        digit[ch] = digit[ch | 0x20] = i
    hist = np.zeros(len(names), np.int64)
    step = 1 << 24
    for lo in range(0, max(0, seq.shape[0] - k + 1), step):
        d = digit[seq[lo:lo + step + k - 1]]
        m = d.shape[0] - k + 1
        fwd = np.zeros(m, np.int64)
        rc = np.zeros(m, np.int64)
        bad = np.zeros(m, bool)
        for j in range(k):
            dj = d[j:j + m]
            fwd = fwd * 4 + dj
            rc += (3 - dj.astype(np.int64)) << (2 * j)
            bad |= dj == 4
        code = np.where(d[k // 2:k // 2 + m] >= 2, rc, fwd)[~bad]
        pid = table[code]
        hist += np.bincount(pid[pid >= 0], minlength=len(names))
    return hist


def child(log2):
    from kmerpapa_amd import engine, predict
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag()}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    bases = sum(s.shape[0] for _, s in contigs)
    dev = engine.get_device(engine.visible_devices()[0])
    names9, rates = fit_partition(dev, contigs, synthetic_sites(contigs, 2_000_000))
    reg = shapes(contigs)
    out.update(bases=bases, contigs=len(contigs), patterns=len(names9), setup_s=round(time.perf_counter() - t0, 2),
               regions={key: int(sum(v.shape[0] for v in r.values())) for key, r in reg.items()})
    print(json.dumps(out), file=sys.stderr, flush=True)
    out["runs"] = []
    for k, names in ((9, names9), (13, ["NN" + x + "NN" for x in names9])):
        rec = {"k": k, "kp_seq_scan_kernel_ms": seq_scan_ms(dev, k, contigs)}
        for shape in ("whole", "tiles_100kb", "exons_150b"):
            rec[shape] = measure(dev, names, rates, contigs, reg[shape])
        rec["track"] = measure(dev, names, rates, contigs, track=True)
        rec["contig1"] = measure(dev, names, rates, contigs[:1], reg["whole"])
        rec["contig1_global_atomics"] = measure(dev, names, rates, contigs[:1], reg["whole"], env={"KP_PRED_GLOBAL": "1"}, reps=1)
        rec["whole_over_kp_seq_scan"] = round(rec["whole"]["kernel_ms"] / rec["kp_seq_scan_kernel_ms"], 3)
        out["runs"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    name0, seq0 = contigs[0]
    t0 = time.perf_counter()
    ref = numpy_hist(seq0, names9)
    numpy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = predict.region_counts([(name0, seq0)], names9, {name0: [(0, seq0.shape[0])]}, rates)[name0]
    gpu_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = predict.region_counts([(name0, seq0)], names9, {name0: [(0, seq0.shape[0])]}, rates)[name0]
    gpu_s = min(gpu_s, time.perf_counter() - t0)
    out["numpy_k9_contig1"] = {"bases": int(seq0.shape[0]), "numpy_one_core_s": round(numpy_s, 3),
                               "gpu_call_s": round(gpu_s, 4), "speedup": round(numpy_s / gpu_s, 1),
                               "equal": bool(np.array_equal(got[0][0].astype(np.int64), ref))}
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
