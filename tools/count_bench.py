#!/usr/bin/env python3
"""Measure the k-mer context counting of a genome (kp_seq_*, kmerpapa_amd.count) against the
host paths a user would otherwise run.

Input: a seeded synthetic genome of 2^LOG2 bases (default 2^30) in eight contigs, each with N
runs at its ends and inside; the first contig ("repeat-rich") also holds 4 Mb of
low-complexity sequence: homopolymers and tandem repeats of period 2..6, 1..50 kb each.  A BED
of 100,000 random regions, 10^7 random sites.

Measured, each as the faster of two sessions (the first allocates):
  * the scan at k = 5, 9, 13, whole genome and BED: device time of the scan kernels (HIP
    events), bases per second and that as a fraction of 8 TB/s at 1 B per base, wall-clock of
    the scan calls (upload of the contig, work items, kernel) and of the whole session (begin
    to the table's read-back), the path taken;
  * the same session serially on one core (engine.seq_host), and that both give equal counts;
  * a numpy sliding-window count of the repeat-rich contig at k = 9 (unfolded), against the GPU
    call on that contig;
  * k = 7: LDS counters against global atomics;
  * k = 9, 13 on the repeat-rich contig: global atomics with the per-wave merge of equal codes
    (the default: lanes that hold the wave's first code add once, together) against
    KP_SEQ_MERGE=0 (every lane adds on its own);
  * 10^7 sites at k = 9.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/count_bench.py --out profiles/count/mi355x.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

KNOBS = ("KP_SEQ_GLOBAL", "KP_SEQ_LDS_K", "KP_SEQ_GRID", "KP_SEQ_MERGE")
HBM_PEAK = 8e12  # bytes per second


def synthetic_genome(log2, seed=2026):
    """Eight contigs of together 2^log2 bases."""
    rng = np.random.RandomState(seed)
    total = 1 << log2
    shares = np.array([24, 20, 18, 16, 14, 12, 12, 12], np.int64)
    sizes = (total * shares // shares.sum()).tolist()
    sizes[0] += total - sum(sizes)
    letters = np.frombuffer(b"ACGTacgt", np.uint8)
    contigs = []
    for ci, n in enumerate(sizes):
        seq = letters[rng.randint(0, 5, size=n, dtype=np.uint8) + rng.randint(0, 2, size=n, dtype=np.uint8) * 3]
        edge = min(10_000, n // 100)
        seq[:edge] = ord("N")
        seq[n - edge:] = ord("N")
        for _ in range(20):  # gaps
            length = int(rng.randint(1, max(2, n // 2000)))
            at = int(rng.randint(0, n - length))
            seq[at:at + length] = ord("N")
        if ci == 0:
            left = min(4_000_000, n // 50)
            while left > 0:
                length = int(min(left, rng.randint(1000, 50_000)))
                unit = letters[rng.randint(0, 4, size=int(rng.randint(1, 7)))]
                at = int(rng.randint(edge, n - edge - length))
                seq[at:at + length] = np.resize(unit, length)
                left -= length
        contigs.append((f"chr{ci + 1}", seq))
    return contigs


def random_bed(contigs, n_regions, seed=7):
    """``n_regions`` regions of 100..2,000 bases spread over the contigs by size, merged."""
    from kmerpapa_amd.seqio import merge_regions
    rng = np.random.RandomState(seed)
    total = sum(s.shape[0] for _, s in contigs)
    out = {}
    for name, seq in contigs:
        m = max(1, n_regions * seq.shape[0] // total)
        start = rng.randint(0, max(1, seq.shape[0] - 2_000), size=m)
        out[name] = merge_regions(np.stack([start, start + rng.randint(100, 2_000, size=m)], axis=1))
    return out


def numpy_count(seq, k):
    """Unfolded k-mer counts of one contig with numpy: digits, k shifted adds, bincount; in
    chunks of 2^24 window starts."""
    lut = np.full(256, 4, np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = lut[ch | 0x20] = i
    out = np.zeros(4 ** k, np.int64)
    step = 1 << 24
    for lo in range(0, max(0, seq.shape[0] - k + 1), step):
        d = lut[seq[lo:lo + step + k - 1]]
        m = d.shape[0] - k + 1
        code = np.zeros(m, np.int64)
        bad = np.zeros(m, bool)
        for j in range(k):
            code = code * 4 + d[j:j + m]
            bad |= d[j:j + m] == 4
        out += np.bincount(code[~bad], minlength=4 ** k)
    return out


def session(dev, k, fold, jobs):
    """One session timed: (pos, bg, stats, seconds in the scan calls, seconds in the site calls,
    seconds of the whole session)."""
    t0 = time.perf_counter()
    dev.seq_begin(k, fold)
    scan_s = sites_s = 0.0
    try:
        for seq, regions, sites in jobs:
            t1 = time.perf_counter()
            if regions is not False:
                dev.seq_scan(seq, regions)
            t2 = time.perf_counter()
            if sites is not None:
                dev.seq_sites(seq, sites)
            scan_s += t2 - t1
            sites_s += time.perf_counter() - t2
    except BaseException:
        dev.seq_end(False, False)
        raise
    pos, bg = dev.seq_end()
    return pos, bg, dev.seq_stats(), scan_s, sites_s, time.perf_counter() - t0


def best_of(dev, k, fold, jobs, env=None, reps=2):
    for key in KNOBS:
        os.environ.pop(key, None)
    os.environ.update(env or {})
    best = None
    for _ in range(reps):
        r = session(dev, k, fold, jobs)
        if best is None or r[5] < best[5]:
            best = r
    for key in KNOBS:
        os.environ.pop(key, None)
    return best


def record(r, bases):
    pos, bg, st, scan_s, sites_s, total_s = r
    per_s = bases / (st["scan_ms"] * 1e-3) if st["scan_ms"] > 0 else None
    return {"scan_kernel_ms": round(st["scan_ms"], 3), "bases_per_s_kernel": per_s,
            "fraction_of_8TBps_at_1B_per_base": round(per_s / HBM_PEAK, 4) if per_s else None,
            "scan_calls_s": round(scan_s, 4), "session_s": round(total_s, 4),
            "path": {0: "none", 1: "lds", 2: "global"}[st["path"]], "items": st["items"], "windows": st["windows"],
            "windows_invalid": st["windows_invalid"]}


def child(log2, host_only):
    from kmerpapa_amd import engine
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag()}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    bases = sum(s.shape[0] for _, s in contigs)
    bed = random_bed(contigs, 100_000)
    bed_bases = int(sum(int((r[:, 1] - r[:, 0]).sum()) for r in bed.values()))
    out.update(bases=bases, contigs=len(contigs), bed_regions_merged=int(sum(r.shape[0] for r in bed.values())),
               bed_bases=bed_bases, setup_s=round(time.perf_counter() - t0, 2))
    whole = [(s, None, None) for _, s in contigs]
    inbed = [(s, bed[n], None) for n, s in contigs]
    dev = None if host_only else engine.get_device(engine.visible_devices()[0])
    host = engine.HostSeq()
    out["scan"] = []
    for k in (5, 9, 13):
        rec = {"k": k}
        t0 = time.perf_counter()
        h = session(host, k, True, whole)
        rec["host_one_core_s"] = round(time.perf_counter() - t0, 3)
        if dev is not None:
            g = best_of(dev, k, True, whole)
            rec["whole"] = record(g, bases)
            rec["equal_to_host"] = bool(np.array_equal(g[1], h[1]) and g[2]["windows"] == h[2]["windows"])
            rec["speedup_scan_calls_vs_host"] = round(rec["host_one_core_s"] / rec["whole"]["scan_calls_s"], 1)
            rec["speedup_session_vs_host"] = round(rec["host_one_core_s"] / rec["whole"]["session_s"], 1)
            gb = best_of(dev, k, True, inbed)
            rec["bed"] = record(gb, bed_bases)
        out["scan"].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
        del h
    name0, seq0 = contigs[0]
    t0 = time.perf_counter()
    ref = numpy_count(seq0, 9)
    out["numpy_k9_contig1"] = {"bases": int(seq0.shape[0]), "numpy_s": round(time.perf_counter() - t0, 3)}
    t0 = time.perf_counter()
    h0 = session(host, 9, False, [(seq0, None, None)])
    out["numpy_k9_contig1"]["host_one_core_s"] = round(time.perf_counter() - t0, 3)
    out["numpy_k9_contig1"]["host_equal_to_numpy"] = bool(np.array_equal(h0[1].astype(np.int64), ref))
    if dev is not None:
        g = best_of(dev, 9, False, [(seq0, None, None)])
        out["numpy_k9_contig1"].update(gpu=record(g, seq0.shape[0]), gpu_equal_to_numpy=bool(np.array_equal(g[1].astype(np.int64), ref)))
        out["k7_lds_vs_global"] = {name: record(best_of(dev, 7, True, whole, env), bases)
                                   for name, env in (("lds", {}), ("global", {"KP_SEQ_GLOBAL": "1"}))}
        out["wave_merge_repeat_rich_contig"] = []
        for k in (9, 13):
            a = best_of(dev, k, True, [(seq0, None, None)], {"KP_SEQ_MERGE": "0"})
            b = best_of(dev, k, True, [(seq0, None, None)])
            out["wave_merge_repeat_rich_contig"].append(
                {"k": k, "unmerged": record(a, seq0.shape[0]), "merged_default": record(b, seq0.shape[0]),
                 "equal": bool(np.array_equal(a[1], b[1]))})
        rng = np.random.RandomState(11)
        sites = [(s, False, rng.randint(0, s.shape[0], size=10_000_000 * s.shape[0] // bases).astype(np.uint64))
                 for _, s in contigs]
        g = best_of(dev, 9, True, sites)
        t0 = time.perf_counter()
        h = session(host, 9, True, sites)
        out["sites_k9"] = {"sites": int(sum(x[2].shape[0] for x in sites)), "gpu_site_calls_s": round(g[4], 4),
                           "gpu_session_s": round(g[5], 4), "host_one_core_s": round(time.perf_counter() - t0, 3),
                           "counted": g[2]["sites"], "skipped": g[2]["sites_skipped"],
                           "equal_to_host": bool(np.array_equal(g[0], h[0]) and g[2]["sites"] == h[2]["sites"])}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=900, help="time limit of the measuring process, seconds")
    ap.add_argument("--host-only", action="store_true", help="no GPU: the host figures only (a check of the tool)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.log2, a.host_only)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--log2", str(a.log2)] + (["--host-only"] if a.host_only else [])
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
