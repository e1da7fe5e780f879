#!/usr/bin/env python3
"""Measure a fitted partition applied to a count table (kp_apply) against the host path it
replaces (``KmerCounts.pattern_counts``: numpy enumeration of every k-mer of every pattern).

Shapes (each in a child process of its own under its own time limit; after a step that fails
or times out nothing more is started):
  7    NNNNNNN, full table (a quick check of the tool itself)
  11   NNNNNNNNNNN, full table (4.2e6 rows) against its greedy partition (alpha 1, c 5)
  13   NNNNNNNNNNNNN, full table (6.7e7 rows) against its greedy partition (alpha 1, c 5)
  16   1,000,000 random 16-mers (a sparse table: no full table exists) against a seeded
       random partition of N x 16 into 6,000 patterns
The full tables are the benchmark's seeded synthetic counts (tools/greedy_bench.py).

Reported per shape and launch configuration (the KP_APPLY_* knobs; every one gives the same
results, which the tool checks): ``assign_ms`` (device time of kp_apply_assign, HIP events),
``call_s`` (wall-clock of the whole Device.apply call: argument checks, copies, all kernels),
rows x patterns per second of the kernel; for the full tables the host path's time and that
both give the same counts.

Usage: python tools/apply_bench.py --runs 11,13,16 --out profiles/apply/mi355x.json
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

RUNS = {"7": ("NNNNNNN", 120), "11": ("NNNNNNNNNNN", 300), "13": ("NNNNNNNNNNNNN", 560), "16": (None, 300)}
CONFIGS = [("default", {}), ("lds", {"KP_APPLY_LDS": "1"}), ("global", {"KP_APPLY_GLOBAL": "1"}),
           ("tile256", {"KP_APPLY_TILE": "256"}), ("tile4096", {"KP_APPLY_TILE": "4096"}),
           ("scalar", {"KP_APPLY_TILE": "0"})]
KNOBS = ("KP_APPLY_TILE", "KP_APPLY_GLOBAL", "KP_APPLY_LDS", "KP_APPLY_GRID")


def full_table(gen_pat):
    """The synthetic counts of an all-N ``gen_pat`` as a KmerCounts table (rows in code order;
    the synthetic table's rows are in matches() order, position 0 fastest) and the (M, U)
    columns in matches() order for kp_greedy."""
    from kmerpapa_amd.io_utils import KmerCounts
    from tools.greedy_bench import synthetic_table
    assert set(gen_pat) == {"N"}
    k = len(gen_pat)
    tab = synthetic_table(gen_pat)
    row = np.arange(tab.shape[0], dtype=np.int64)
    code = np.zeros_like(row)
    for i in range(k):  # position i of the row index is letter i of the code
        code |= ((row >> (2 * i)) & 3) << (2 * (k - 1 - i))
    M = np.empty(tab.shape[0], np.int64)
    U = np.empty(tab.shape[0], np.int64)
    M[code] = tab[:, 0]
    U[code] = tab[:, 1]
    return KmerCounts(k, row.astype(np.uint64), M, U), np.ascontiguousarray(tab[:, 0]), np.ascontiguousarray(tab[:, 1])


def random_partition(k, target, seed=6000):
    """Pattern words of a seeded random partition of N x k: a random pattern is split at a
    random position into a random pair of complementary nucleotide sets, ``target`` - 1 times."""
    rng = np.random.RandomState(seed)
    parts = [[15] * k]
    while len(parts) < target:
        j = int(rng.randint(len(parts)))
        pos = [i for i, m in enumerate(parts[j]) if m & (m - 1)]
        if not pos:
            continue
        p = parts.pop(j)
        i = pos[int(rng.randint(len(pos)))]
        subsets = [a for a in range(1, p[i]) if a & p[i] == a]
        a = subsets[int(rng.randint(len(subsets)))]
        parts += [p[:i] + [a] + p[i + 1:], p[:i] + [p[i] ^ a] + p[i + 1:]]
    return [sum(m << (4 * i) for i, m in enumerate(p)) for p in parts]


def measure(dev, k, words, super_word, table, rates):
    """Every launch configuration on one table: a list of records, all with equal results."""
    out, first = [], None
    n, P = len(table), len(words)
    for name, env in CONFIGS:
        for key in KNOBS:
            os.environ.pop(key, None)
        os.environ.update(env)
        best = None
        for rep in range(3):  # the first call of a process may allocate; keep the fastest
            t0 = time.perf_counter()
            pid, pM, pU, ll, st = dev.apply(k, words, super_word, table.codes, table.M, table.U, rates, want_pid=False)
            call = time.perf_counter() - t0
            if best is None or call < best[0]:
                best = (call, st)
        res = (pM.tobytes(), pU.tobytes(), ll.tobytes(), st["unmatched"], st["multi"], st["overlap_pairs"])
        first = first or res
        call, st = best
        out.append({"config": name, "env": env, "assign_ms": round(st["assign_ms"], 3), "call_s": round(call, 4),
                    "tiles": st["tiles"], "lds_counters": st["lds_counters"],
                    "tests_per_s": (n * P / (st["assign_ms"] * 1e-3)) if st["assign_ms"] > 0 else None,
                    "same_results_as_default": res == first})
    for key in KNOBS:
        os.environ.pop(key, None)
    t0 = time.perf_counter()
    pid = dev.apply(k, words, super_word, table.codes, table.M, table.U, rates, want_pid=True)[0]
    with_pid = time.perf_counter() - t0
    return out, round(with_pid, 4), pid


def child(run, dev=None):
    from kmerpapa_amd import engine
    from kmerpapa_amd.io_utils import KmerCounts
    from kmerpapa_amd.score_utils import get_betas
    dev = dev or engine.get_device(engine.visible_devices()[0])
    gen_pat, _ = RUNS[run]
    out = {"run": run, "kernel_tag": engine.kernel_tag()}
    t0 = time.perf_counter()
    if gen_pat is None:
        k = 16
        rng = np.random.RandomState(16)
        codes = np.unique(rng.randint(0, 1 << 32, size=1000000, dtype=np.int64).astype(np.uint64))
        table = KmerCounts(k, codes, rng.poisson(0.4, size=codes.shape[0]), rng.poisson(1.5e4, size=codes.shape[0]))
        words = random_partition(k, 6000)
        rates = np.full(len(words), 2.7e-5)
        out.update(table="1,000,000 random 16-mers drawn with repeats, unique kept", partition="seeded random, 6,000 patterns")
    else:
        k = len(gen_pat)
        alpha, penalty = 1.0, 5.0
        table, Mrow, Urow = full_table(gen_pat)
        beta = get_betas(alpha, int(Mrow.sum()), int(Urow.sum()))
        t1 = time.perf_counter()
        dev.greedy(gen_pat, Mrow, Urow, [(-1, -1, alpha, beta, penalty)])
        words = [int(w) for w in dev.greedy_leaves(0)]
        out.update(gen_pat=gen_pat, partition="greedy, alpha 1, c 5", greedy_fit_s=round(time.perf_counter() - t1, 3))
        del Mrow, Urow
    out.update(k=k, rows=len(table), patterns=len(words), setup_s=round(time.perf_counter() - t0, 3))
    super_word = (1 << (4 * k)) - 1
    if gen_pat is not None:
        names = [engine.word_pattern(w, k) for w in words]
        t0 = time.perf_counter()
        counts = table.pattern_counts(names)  # the parent commit's host path (cli.py's `counts`)
        out["host_pattern_counts_s"] = round(time.perf_counter() - t0, 3)
        rates = np.array([(m + alpha) / (m + u + alpha + beta) for m, u in counts])
    out["configs"], out["call_with_pid_s"], pid = measure(dev, k, words, super_word, table, rates)
    _, pM, pU, ll, st = dev.apply(k, words, super_word, table.codes, table.M, table.U, rates, want_pid=False)
    out.update(unmatched=st["unmatched"], multi=st["multi"], overlap_pairs=st["overlap_pairs"], ll=float(ll[0]),
               pid_min=int(pid.min()), rows_times_patterns=len(table) * len(words))
    if gen_pat is not None:
        out["counts_equal_host_path"] = list(zip(pM.tolist(), pU.tolist())) == counts
        d = out["configs"][0]
        out["speedup_default_call_vs_host_path"] = round(out["host_pattern_counts_s"] / d["call_s"], 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="7")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child)
        return 0
    results = []
    rc = 0
    for run in a.runs.split(","):
        limit = RUNS[run][1]
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
    doc = {"date": time.strftime("%Y-%m-%d"), "measured": True, "results": results}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
    if rc:
        print(json.dumps(results[-1]), file=sys.stderr)
    return rc


if __name__ == "__main__":
    sys.exit(main())
