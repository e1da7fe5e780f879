#!/usr/bin/env python3
"""Measure the indel-model session (kp_ispec_*, kmerpapa_amd.indel) beside its counterparts.

Input: the synthetic genome of tools/count_bench.py (2^LOG2 bases, eight contigs) and the three
region sets of tools/predict_bench.py (whole contigs, 100-kb tiles, about 200,000 exon-like regions),
as tools/spectrum_bench.py uses them.  Both models are random partitions with that bench's pattern
count (1,290) at k = 8: 645 insertion and 645 deletion patterns for the indel model, 12 types of
107 or 108 patterns (the centre base fixed) for the unfolded spectrum model.

Measured, in one process, after one warm-up session each that allocates, over REPS sessions each,
the two kinds of session alternating:
  * kp_ispec_regions beside kp_spec_regions (k = 8, fold = 0) per region set: the scan kernels' time
    (HIP events) and the wall-clock of the calls (uploads and read-back included), medians, minima
    and maxima, and the ratio of the medians;
  * kp_ispec_sites beside kp_seq_indels (k = 8, both strands) on the 10^6 synthetic indels of
    tools/indel_bench.py: wall-clock of the call (uploads, kernel, read-back), the same figures; the
    kernel time of kp_ispec_sites (HIP events) apart -- kp_seq_indels reports none.  Both must
    resolve every site alike.
The measurements run in one child process under a time limit; the parent writes the JSON.

Usage: python tools/indel_model_bench.py --out profiles/indel_model/mi355x.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

KNOBS = ("KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID", "KP_ISPEC_GLOBAL", "KP_ISPEC_LDS_P", "KP_ISPEC_GRID",
         "KP_SEQ_GLOBAL", "KP_SEQ_LDS_K", "KP_SEQ_GRID", "KP_SEQ_MERGE", "KP_SEQ_BOTH_STEPS")
PATTERNS = 1290  # of the model of tools/spectrum_bench.py (profiles/spectrum/mi355x.json)
K = 8


def partition(rng, start, leaves):
    """Exactly ``leaves`` IUPAC patterns that partition ``start``: an N becomes its four bases or R
    and Y, an R or Y its two bases."""
    pats = [start]
    while len(pats) < leaves:
        i = int(rng.randint(len(pats)))
        free = [j for j, c in enumerate(pats[i]) if c in "NRY"]
        if not free:
            continue
        p = pats.pop(i)
        j = free[int(rng.randint(len(free)))]
        four = p[j] == "N" and leaves - len(pats) - 1 >= 3 and rng.rand() < 0.5
        parts = "ACGT" if four else {"N": "RY", "R": "AG", "Y": "CT"}[p[j]]
        pats += [p[:j] + c + p[j + 1:] for c in parts]
    return sorted(pats)


def models(seed=17):
    """``(indel.Model, spectrum.Model)`` of PATTERNS patterns each at k = K."""
    from kmerpapa_amd import indel, spectrum
    rng = np.random.RandomState(seed)
    half = PATTERNS // 2
    parts = {kind: partition(rng, "N" * K, n) for kind, n in (("ins", half), ("del", PATTERNS - half))}
    imodel = indel.Model.from_partitions({kind: (n, [(0, 0)] * len(n), (rng.rand(len(n)) * 1e-3).tolist())
                                          for kind, n in parts.items()})
    types = spectrum.TYPES(False)
    sparts = {}
    for t, kind in enumerate(types):
        n = PATTERNS // 12 + (t < PATTERNS % 12)
        names = partition(rng, "N" * (K // 2) + kind[0] + "N" * (K - 1 - K // 2), n)
        sparts[kind] = (names, [(0, 0)] * n, (rng.rand(n) * 1e-3).tolist())
    smodel = spectrum.Model.from_partitions(sparts)
    assert len(imodel.names) == len(smodel.names) == PATTERNS
    return imodel, smodel


def ispec_session(model, contigs, regions, budget):
    from kmerpapa_amd import indel
    t0 = time.perf_counter()
    calls, check = 0.0, 0.0
    with indel.session(model) as s:
        for name, seq in contigs:
            t1 = time.perf_counter()
            _, _, exp = s.ispec_regions(seq, regions[name], model.rates, False, budget)
            calls += time.perf_counter() - t1
            check += float(exp.sum())
        st = s.ispec_stats()
    return st, calls, time.perf_counter() - t0, check


def spec_session(model, contigs, regions, budget):
    from kmerpapa_amd import spectrum
    t0 = time.perf_counter()
    calls, check = 0.0, 0.0
    with spectrum.session(model, False) as s:
        for name, seq in contigs:
            t1 = time.perf_counter()
            _, _, exp = spectrum._contig_regions(s, seq, regions[name], len(model.names), model.rates, False, budget)
            calls += time.perf_counter() - t1
            check += float(exp.sum())
        st = s.spec_stats()
    return st, calls, time.perf_counter() - t0, check


def spread(xs, digits):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def summary(runs):
    st = runs[-1][0]
    return {"kernel_ms": spread([r[0]["scan_ms"] for r in runs], 3), "calls_s": spread([r[1] for r in runs], 4),
            "session_s": spread([r[2] for r in runs], 4), "lut_ms": spread([r[0]["lut_ms"] for r in runs], 3),
            "lut_bytes": st["lut_bytes"], "items": st["items"], "path": {0: "none", 1: "lds", 2: "global"}[st["path"]],
            "same_result_every_run": len({r[3] for r in runs}) == 1}


def regions_pair(imodel, smodel, contigs, regions, budget, reps):
    ispec_session(imodel, contigs, regions, budget)  # the first of each kind allocates
    spec_session(smodel, contigs, regions, budget)
    a, b = [], []
    for _ in range(reps):
        a.append(ispec_session(imodel, contigs, regions, budget))
        b.append(spec_session(smodel, contigs, regions, budget))
    one, other = summary(a), summary(b)
    return {"ispec": one, "spec_unfolded": other,
            "kernel_ratio_ispec_over_spec": round(one["kernel_ms"]["median"] / other["kernel_ms"]["median"], 3),
            "calls_ratio_ispec_over_spec": round(one["calls_s"]["median"] / other["calls_s"]["median"], 3)}


def sites_pair(dev, imodel, seq, n_sites, reps):
    from indel_bench import synthetic_indels
    seq, sites = synthetic_indels(seq, n_sites, n_sites // 100)
    new, old, kernel = [], [], []
    for i in range(reps + 1):  # (the first of each allocates)
        dev.ispec_begin(imodel.k, imodel.words(), imodel.pkind)
        try:
            before = dev.ispec_stats()["sites_ms"]
            t1 = time.perf_counter()
            pid, res = dev.ispec_sites(seq, 0, sites, "left", 0)
            new.append(time.perf_counter() - t1)
            kernel.append(dev.ispec_stats()["sites_ms"] - before)
            st = dev.ispec_stats()
        finally:
            dev.ispec_end()
        dev.seq_begin_indel(K, True)
        try:
            t1 = time.perf_counter()
            cres = dev.seq_indels(seq, 0, sites, "left", 0)
            old.append(time.perf_counter() - t1)
        finally:
            dev.seq_end_typed(False, False)
        cst = dev.seq_stats()
    one, other = spread(new[1:], 5), spread(old[1:], 5)
    return {"k": K, "sites": n_sites, "in_runs_of_1000_or_more": n_sites // 100, "contig_bases": int(seq.shape[0]),
            "ispec_sites_call_s": one, "seq_indels_call_s": other, "ispec_sites_kernel_ms": spread(kernel[1:], 3),
            "call_ratio_ispec_over_seq_indels": round(one["median"] / other["median"], 3),
            "kept": int((pid[:, 0] != -2).sum()), "kept_by_the_session_stats": st["sites"], "counted_by_seq_indels": cst["sites"],
            "ambiguous": int((res[:, 1] > res[:, 0]).sum()), "with_both_patterns": int((pid >= 0).all(axis=1).sum()),
            "resolved_equal": bool(np.array_equal(res, cres))}


def child(log2, reps):
    from count_bench import synthetic_genome
    from predict_bench import BUDGET, shapes

    from kmerpapa_amd import engine
    for key in KNOBS:
        os.environ.pop(key, None)
    out = {"genome_log2": log2, "kernel_tag": engine.kernel_tag(), "k": K, "patterns": PATTERNS, "reps": reps}
    t0 = time.perf_counter()
    contigs = synthetic_genome(log2)
    dev = engine.get_device(engine.visible_devices()[0])
    imodel, smodel = models()
    reg = shapes(contigs)
    out.update(bases=sum(s.shape[0] for _, s in contigs), contigs=len(contigs), setup_s=round(time.perf_counter() - t0, 2),
               regions={key: int(sum(v.shape[0] for v in r.values())) for key, r in reg.items()})
    print(json.dumps(out), file=sys.stderr, flush=True)
    out["regions_runs"] = {}
    for shape in ("whole", "tiles_100kb", "exons_150b"):
        out["regions_runs"][shape] = regions_pair(imodel, smodel, contigs, reg[shape], BUDGET, reps)
        print(json.dumps({shape: out["regions_runs"][shape]}), file=sys.stderr, flush=True)
    n_sites = 1_000_000 if contigs[0][1].shape[0] > 50_000_000 else 50_000
    out["sites"] = sites_pair(dev, imodel, contigs[0][1], n_sites, reps)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=30, help="genome of 2^LOG2 bases")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--limit", type=int, default=600, help="time limit of the measuring process, seconds")
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
