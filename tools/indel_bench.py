#!/usr/bin/env python3
"""Measure the indel counting (kp_seq_begin_indel / kp_seq_begin_strands / kp_seq_indels, kp_indel.h)
on the synthetic genome of tools/count_bench.py (2^LOG2 bases, default 2^30, eight contigs).

Measured:
  * the both-strand scan against the forward scan of the same build (kp_seq_begin_strands with both
    = 1 and 0), k = 6 (LDS counters) and k = 10 (global atomics), whole genome: device time of the
    scan kernels (HIP events), the faster of REPS sessions each, and their ratio;
  * kp_seq_indels at k = 8 on 10^6 synthetic indels of the first contig, a hundredth of them inside
    tandem repeats of 1,000 bases or more (planted for this purpose, periods 1..6): wall-clock of
    the call (upload, kernel, read-back of `resolved`), sites per second, and the host session of
    the same sites on one core beside it; both must give equal tables and rows;
  * with --parent-lib: the folded one-strand scan that existed before (kp_seq_begin, k = 5 and 9,
    whole genome) on this build and on the build given, REPS sessions each in alternating child
    processes: minimum, maximum, and whether min(new) <= min(parent) * (1 + the parent's own
    (max - min) / min).
Every measurement runs in a child process under a time limit; the parent writes the JSON.

Usage: python tools/indel_bench.py --out profiles/indel/mi355x.json [--parent-lib PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

KNOBS = ("KP_SEQ_GLOBAL", "KP_SEQ_LDS_K", "KP_SEQ_GRID", "KP_SEQ_MERGE", "KP_SEQ_BOTH_STEPS")


def load_genome(path):
    with np.load(path) as z:
        return [(f"chr{i + 1}", z[f"c{i}"]) for i in range(len(z.files))]


def scan_ms(calls, begin, jobs, reps):
    """Device milliseconds of the scan kernels of `reps` sessions, and the last table."""
    out = []
    for _ in range(reps):
        begin()
        try:
            for seq in jobs:
                calls.seq_scan(seq)
        except BaseException:
            calls.seq_end(False, False)
            raise
        _, bg = calls.seq_end(False, True)
        out.append(calls.seq_stats()["scan_ms"])
    return out, bg


def synthetic_indels(seq, n_sites, in_runs, seed=5):
    """`n_sites` indels of the contig `seq`: random insertions of 1..3 bases and deletions of 1..3,
    and `in_runs` of them inside tandem repeats of 1,000..4,000 bases planted here (one unit
    inserted or deleted).  Returns the changed contig and engine.indel_sites arrays."""
    from kmerpapa_amd import engine
    rng = np.random.RandomState(seed)
    seq = seq.copy()
    n = seq.shape[0]
    letters = np.frombuffer(b"ACGT", np.uint8)
    runs = []
    for at in np.linspace(n // 10, n - n // 10, 400).astype(np.int64).tolist():
        unit = letters[rng.randint(0, 4, size=int(rng.randint(1, 7)))]
        length = int(rng.randint(1000, 4001))
        seq[at:at + length] = np.resize(unit, length)
        runs.append((at, length, unit))
    pos = rng.randint(20_000, n - 20_000, size=n_sites).astype(np.uint64)
    length = rng.randint(1, 4, size=n_sites)
    is_del = rng.random_sample(n_sites) < 0.5
    random_ins = rng.random_sample(n_sites) < 0.5
    for i in rng.choice(n_sites, size=in_runs, replace=False).tolist():
        at, run_len, unit = runs[int(rng.randint(len(runs)))]
        pos[i] = at + int(rng.randint(0, run_len - 6))
        length[i] = unit.shape[0]
        random_ins[i] = False  # (in a run: one unit, in phase, so the site can sit anywhere along it)
    del_len = np.where(is_del, length, 0).astype(np.uint64)
    ins_len = np.where(is_del, 0, length)
    ins_off = np.concatenate([[0], np.cumsum(ins_len)]).astype(np.uint64)
    # an insertion repeats the bases after its breakpoint (in a run: one unit, in phase), or is random
    idx = np.repeat(pos[~is_del].astype(np.int64), ins_len[~is_del]) + \
        (np.arange(int(ins_len.sum())) - np.repeat(ins_off[:-1][~is_del].astype(np.int64), ins_len[~is_del]))
    ins = seq[idx].copy()
    bad = ~np.isin(ins & 0xDF, letters)
    ins[bad] = ord("A")
    redraw = np.repeat(random_ins[~is_del], ins_len[~is_del])
    ins[redraw] = letters[rng.randint(0, 4, size=int(redraw.sum()))]
    return seq, engine.indel_sites(pos, del_len, (ins, ins_off), np.arange(n_sites, dtype=np.uint64))


def child_indel(genome, reps, host_only):
    from kmerpapa_amd import engine
    contigs = load_genome(genome)
    jobs = [s for _, s in contigs]
    bases = int(sum(s.shape[0] for s in jobs))
    out = {"bases": bases, "kernel_tag": engine.kernel_tag(), "reps": reps}
    host = engine.HostSeq()
    dev = None if host_only else engine.get_device(engine.visible_devices()[0])
    for key in KNOBS:
        os.environ.pop(key, None)
    if dev is not None:
        out["scan_both_vs_forward"] = []
        for k in (6, 10):
            scan_ms(dev, lambda: dev.seq_begin_strands(k, False), jobs[-1:], 1)  # (first use allocates)
            fwd, bg_f = scan_ms(dev, lambda: dev.seq_begin_strands(k, False), jobs, reps)
            both, bg_b = scan_ms(dev, lambda: dev.seq_begin_strands(k, True), jobs, reps)
            st = dev.seq_stats()
            rec = {"k": k, "path": {1: "lds", 2: "global"}[st["path"]], "forward_ms": [round(x, 3) for x in fwd],
                   "both_ms": [round(x, 3) for x in both], "ratio_of_minima": round(min(both) / min(fwd), 4),
                   "forward_bases_per_s": bases / (min(fwd) * 1e-3), "both_bases_per_s": bases / (min(both) * 1e-3),
                   "both_sums_to_twice_forward": bool(int(bg_b.sum()) == 2 * int(bg_f.sum()) == 2 * st["windows"])}
            out["scan_both_vs_forward"].append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    n_sites = 1_000_000 if jobs[0].shape[0] > 50_000_000 else 50_000
    seq, sites = synthetic_indels(jobs[0], n_sites, n_sites // 100)
    rec = {"k": 8, "sites": n_sites, "in_runs_of_1000_or_more": n_sites // 100, "contig_bases": int(seq.shape[0])}
    t0 = time.perf_counter()
    host.seq_begin_indel(8, True)
    t1 = time.perf_counter()
    h_res = host.seq_indels(seq, 0, sites, "left", 0)
    rec["host_one_core_s"] = round(time.perf_counter() - t1, 4)
    h_cols, _ = host.seq_end_typed(True, False)
    st = host.seq_stats()
    rec.update(host_sites_per_s=n_sites / rec["host_one_core_s"], counted=st["sites"], skipped=st["sites_skipped"],
               ambiguous=int((h_res[:, 1] > h_res[:, 0]).sum()), span_1000_or_more=int((h_res[:, 1] - h_res[:, 0] >= 1000).sum()))
    if dev is not None:
        calls = []
        for _ in range(reps + 1):  # (the first allocates)
            dev.seq_begin_indel(8, True)
            try:
                t1 = time.perf_counter()
                g_res = dev.seq_indels(seq, 0, sites, "left", 0)
                calls.append(time.perf_counter() - t1)
            finally:
                g_cols, _ = dev.seq_end_typed(True, False)
        rec.update(gpu_call_s=[round(x, 5) for x in calls[1:]], gpu_sites_per_s=n_sites / min(calls[1:]),
                   equal_to_host=bool(np.array_equal(g_cols, h_cols) and np.array_equal(g_res, h_res)))
    out["indels"] = rec
    print(json.dumps(out), flush=True)


def child_existing(genome, reps):
    from kmerpapa_amd import engine
    jobs = [s for _, s in load_genome(genome)]
    dev = engine.get_device(engine.visible_devices()[0])
    for key in KNOBS:
        os.environ.pop(key, None)
    out = {"lib": engine.LIB_PATH}
    for k in (5, 9):
        scan_ms(dev, lambda: dev.seq_begin(k, True), jobs[-1:], 1)
        ms, bg = scan_ms(dev, lambda: dev.seq_begin(k, True), jobs, reps)
        out[f"k{k}_ms"] = [round(x, 3) for x in ms]
        out[f"k{k}_sum"] = int(bg.sum())
    print(json.dumps(out), flush=True)


def run_child(args, limit, env=None):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True, timeout=limit,
                       env=dict(os.environ, **(env or {})))
    if p.returncode:
        raise SystemExit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=600, help="time limit of each measuring process, seconds")
    ap.add_argument("--parent-lib", default=None, help="an earlier build of the library, for the existing scan's A/B")
    ap.add_argument("--host-only", action="store_true", help="no GPU: the host figures only (a check of the tool)")
    ap.add_argument("--child", choices=("indel", "existing"))
    ap.add_argument("--genome")
    a = ap.parse_args()
    if a.child == "indel":
        child_indel(a.genome, a.reps, a.host_only)
        return 0
    if a.child == "existing":
        child_existing(a.genome, a.reps)
        return 0
    from count_bench import synthetic_genome
    with tempfile.TemporaryDirectory() as tmp:
        genome = os.path.join(tmp, "genome.npz")
        np.savez(genome, **{f"c{i}": s for i, (_, s) in enumerate(synthetic_genome(a.log2))})
        common = ["--genome", genome, "--reps", str(a.reps)]
        try:
            result = run_child(["--child", "indel"] + common + (["--host-only"] if a.host_only else []), a.limit)
            if a.parent_lib and not a.host_only:
                half = (a.reps + 1) // 2
                runs = {"new": [], "parent": []}
                for which in ("new", "parent", "new", "parent"):  # alternating, two processes each
                    env = {"KMERPAPA_LIB": os.path.abspath(a.parent_lib)} if which == "parent" else {}
                    runs[which].append(run_child(["--child", "existing", "--genome", genome, "--reps", str(half)], a.limit, env))
                ab = {}
                for k in (5, 9):
                    new = [x for r in runs["new"] for x in r[f"k{k}_ms"]]
                    old = [x for r in runs["parent"] for x in r[f"k{k}_ms"]]
                    bound = min(old) * (1 + (max(old) - min(old)) / min(old))
                    ab[f"k{k}"] = {"new_ms": new, "parent_ms": old, "bound_ms": round(bound, 3), "accepted": bool(min(new) <= bound),
                                   "equal_counts": len({r[f"k{k}_sum"] for rs in runs.values() for r in rs}) == 1}
                result["existing_scan_new_vs_parent"] = ab
        except subprocess.TimeoutExpired:
            print(f"time limit of {a.limit} s", file=sys.stderr)
            return 1
    doc = {"date": time.strftime("%Y-%m-%d"), "measured": not a.host_only, "result": result}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
