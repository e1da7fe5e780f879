"""Mutation sets drawn from a spectrum model (kp_spec_simulate, kp_sim.h) on the host session
(engine.HostSpec: the kernels' per-position functions run serially) against the independent
oracle tests/sim_ref.py, pinned to the merged calls (spec_sites, seq_count_typed, regions
--observed), with the error codes, the overflow protocol, the statistics of a draw and the command
line.  Every comparison but the statistical one is exact equality.

The Philox known answers: the oracle reproduces all three.  The library takes its counter from
(position, contig_id, replicate) with the position's high word always 0 (a contig is shorter than
2^32 bases), so only the all-zero known answer is a counter it can be given; it is pinned through
the hit / no-hit outcome around that u.  The words of the other two go through the library as
seed, contig_id and replicate at small positions, against the oracle's u."""
import ctypes
import math

import numpy as np
import pytest

from kmerpapa_amd import engine, predict, spectrum
from tests import sim_ref as S
from tests import spec_ref as R

word = engine.pattern_word
ARG, STATE = -1, -4

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _model(seed, k, fold, n_types, leaves, empty, lo, hi):
    """A random model with rates uniform in [lo, hi]."""
    rng = np.random.RandomState(seed)
    names, ptype, _ = R.random_model(rng, k, fold, n_types, leaves, empty)
    return names, ptype, rng.uniform(lo, hi, size=len(names))


class _Session:
    def __init__(self, k, names, ptype, fold):
        self.args = (k, [word(x) for x in names], ptype, fold)

    def __enter__(self):
        self.s = engine.HostSpec()
        self.s.spec_begin(*self.args)
        return self.s

    def __exit__(self, *exc):
        self.s.spec_end()


def _raw(s, seq, regions, rates, seed, cap, contig_id=0, replicate=0, scale=1.0, fill=0x5A):
    """kp_spec_simulate itself: ``(rc, n_hits, pos, alt, pid)`` with the outputs pre-filled."""
    seq = np.ascontiguousarray(seq, np.uint8)
    reg = np.asarray(regions, np.uint64).reshape(-1, 2)
    rb, re = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    rates = np.ascontiguousarray(rates, np.float64)
    pos, alt, pid = np.full(cap + 1, fill, np.uint64), np.full(cap + 1, fill, np.uint8), np.full(cap + 1, fill, np.int32)
    n_hits = ctypes.c_uint64(12345)
    p = engine._ptr
    rc = engine.load().kp_spec_simulate(s._h, p(seq), ctypes.c_uint64(seq.shape[0]), ctypes.c_uint32(contig_id), p(rb), p(re),
                                        ctypes.c_uint64(reg.shape[0]), p(rates), ctypes.c_double(scale), ctypes.c_uint64(seed),
                                        ctypes.c_uint32(replicate), ctypes.c_uint64(cap), p(pos), p(alt), p(pid),
                                        ctypes.byref(n_hits))
    return rc, n_hits.value, pos, alt, pid


def _u(x):
    return float((x[1] << 32 | x[0]) >> 11) * 2.0 ** -53


def _hit(s, seq, pos, rate, seed, contig_id, replicate):
    got = s.spec_simulate(seq, [(pos, pos + 1)], [rate], seed, contig_id, replicate)
    return got[0].tolist() == [pos]


def test_philox_known_answers():
    for counter, key, want in KNOWN:
        assert " ".join(f"{x:08x}" for x in S.philox(counter, key)) == want
    assert S.uniform(0, 0, 0, 0) == _u((0x6627E8D5, 0xE169C58D))
    # one pattern A (type A>C) of rate r on a contig of A's: position p is hit exactly if u(p) < r
    seq = np.full(64, ord("A"), np.uint8)
    with _Session(1, ["A"], [0], False) as s:
        u = _u((0x6627E8D5, 0xE169C58D))
        assert 0.0 < u < 1.0
        assert not _hit(s, seq, 0, u, 0, 0, 0) and _hit(s, seq, 0, math.nextafter(u, 1.0), 0, 0, 0)
        # the words of the other known answers as seed, contig and replicate
        for seed, contig, rep in ((0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x299F31D0A4093822, 0x13198A2E, 0x03707344),
                                  (1 << 32, 0, 1), (1, 1, 0)):
            for pos in (0, 1, 63):
                u = _u(S.philox((pos, 0, contig, rep), (seed & 0xFFFFFFFF, seed >> 32)))
                assert u == S.uniform(seed, contig, pos, rep)
                assert not _hit(s, seq, pos, u, seed, contig, rep), (seed, pos)
                assert _hit(s, seq, pos, math.nextafter(u, 1.0), seed, contig, rep), (seed, pos)


def _regions(n, k):
    """Ascending and disjoint: clipped at both contig ends, empty, adjacent, shorter than k."""
    regs = [(0, 0), (0, 1), (1, k + 3), (k + 3, k + 3), (k + 3, 200), (200, 201), (250, 250 + max(k - 1, 1)), (300, 300),
            (n // 2, n - 7), (n - 7, n - 7), (n - 2, n), (n, n)]
    return np.array(regs, np.uint64)


CASES = [(1, False, 6, 1, 3), (1, True, 2, 1, 0), (3, True, 6, 5, 4), (3, False, 4, 4, 1), (5, True, 5, 9, 2), (5, False, 6, 7, 5),
         (5, True, 3, 9, 1)]


@pytest.mark.parametrize("k,fold,n_types,leaves,empty", CASES, ids=[f"k{c[0]}_fold{int(c[1])}_T{c[2]}" for c in CASES])
def test_host_session_equals_the_oracle(k, fold, n_types, leaves, empty):
    rng = np.random.RandomState(10 * k + n_types)
    n = 3001
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.01)
    regs = _regions(n, k)
    hits = 0
    for tag, lo, hi in (("dense", 0.05, 0.3), ("sparse", 1e-4, 1e-4)):
        names, ptype, rates = _model(k + n_types, k, fold, n_types, leaves, empty, lo, hi)
        assert len(set(ptype)) == n_types - 1
        track = R.track(seq, names, ptype, fold)
        with _Session(k, names, ptype, fold) as s:
            for seed, contig, rep, scale in ((7, 0, 0, 1.0), (2 ** 63 + 5, 3, 9, 1.0 if tag == "dense" else 50.0)):
                got = s.spec_simulate(seq, regs, rates, seed, contig, rep, scale)
                st = s.spec_sim_stats()
                ref = S.simulate(seq, names, ptype, rates, fold, regs.tolist(), seed, contig, rep, scale, pid=track)
                for g, r in zip(got, ref[:3]):
                    assert g.dtype == r.dtype and g.tobytes() == r.tobytes(), (tag, seed)
                assert st["windows"] == ref[3] and st["hits"] == len(ref[0]) and st["count_ms"] == st["write_ms"] == 0.0
                assert np.all(np.diff(got[0].astype(np.int64)) > 0) and set(got[1].tolist()) <= set(b"ACGT")
                hits += len(ref[0]) if tag == "dense" else 0
    assert hits > 100  # (the comparison is not one of empty sets)


@pytest.mark.parametrize("k,fold", [(3, True), (3, False), (5, True)])
def test_rate_one_hits_every_position_of_the_type(k, fold):
    rng = np.random.RandomState(k + fold)
    names, ptype, _ = R.random_model(rng, k, fold, 6, 5, empty=3)
    seq = R.random_seq(rng, 2000, lower=0.2, invalid=0.01)
    track = R.track(seq, names, ptype, fold)
    with _Session(k, names, ptype, fold) as s:
        for t in sorted(set(ptype)):
            rates = np.array([1.0 if x == t else 0.0 for x in ptype])
            pos, alt, pid = s.spec_simulate(seq, [(0, 2000)], rates, 11)
            ids = track[t % 3]
            want = np.flatnonzero((ids >= 0) & (np.asarray(ptype)[np.maximum(ids, 0)] == t))
            assert len(want) > 50 and np.array_equal(pos, want) and np.array_equal(pid, ids[want])
            assert all(S.forward_alt(chr(seq[p]), t % 3, fold) == chr(a) for p, a in zip(pos.tolist(), alt.tolist()))
        got = s.spec_simulate(seq, [(0, 2000)], np.zeros(len(names)), 11)
        assert [len(x) for x in got] == [0, 0, 0] and s.spec_sim_stats()["hits"] == 0
        assert s.spec_sim_stats()["windows"] == int((track[0] != R.INVALID).sum())
        assert len(s.spec_simulate(seq, [(0, 2000)], np.ones(len(names)), 11, scale=0.0)[0]) == 0


def test_regions_arguments_and_repeats():
    k, fold = 5, True
    names, ptype, rates = _model(4, k, fold, 6, 9, 2, 0.02, 0.2)
    rng = np.random.RandomState(8)
    n = 4000
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.005)
    regs = np.array([(3, 90), (90, 91), (400, 1700), (1700, 1703), (2500, 2500), (3100, n)], np.uint64)
    with _Session(k, names, ptype, fold) as s:
        whole = s.spec_simulate(seq, [(0, n)], rates, 99, 2, 1)
        part = s.spec_simulate(seq, regs, rates, 99, 2, 1)
        inside = np.zeros(n, bool)
        for b, e in regs.tolist():
            inside[b:e] = True
        keep = inside[whole[0].astype(np.intp)]
        assert 100 < keep.sum() < len(keep)
        for w, p in zip(whole, part):
            assert w[keep].tobytes() == p.tobytes()
        again = s.spec_simulate(seq, [(0, n)], rates, 99, 2, 1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, again))
        for kw in (dict(seed=98), dict(contig_id=3), dict(replicate=0), dict(seed=99 + (1 << 32))):
            args = dict(seed=99, contig_id=2, replicate=1)
            args.update(kw)
            other = s.spec_simulate(seq, [(0, n)], rates, **args)
            assert other[0].tobytes() != whole[0].tobytes(), kw
            assert abs(len(other[0]) - len(whole[0])) < 200
        # every first `cap` gives the same set
        for cap in (0, 1, len(whole[0]) - 1, len(whole[0]), 10 * n):
            got = s.spec_simulate(seq, [(0, n)], rates, 99, 2, 1, cap=cap)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, got))


def test_cap_too_small_leaves_the_outputs_untouched():
    k, fold = 3, True
    names, ptype, rates = _model(5, k, fold, 6, 5, 0, 0.05, 0.3)
    seq = R.random_seq(np.random.RandomState(3), 1500, lower=0.2, invalid=0.01)
    with _Session(k, names, ptype, fold) as s:
        want = s.spec_simulate(seq, [(0, 1500)], rates, 5)
        h = len(want[0])
        assert h > 100
        rc, n_hits, pos, alt, pid = _raw(s, seq, [(0, 1500)], rates, 5, h - 1)
        assert rc == 0 and n_hits == h
        assert np.all(pos == 0x5A) and np.all(alt == 0x5A) and np.all(pid == 0x5A)
        assert s.spec_sim_stats()["hits"] == h
        rc, n_hits, pos, alt, pid = _raw(s, seq, [(0, 1500)], rates, 5, h)
        assert rc == 0 and n_hits == h
        assert pos[:h].tobytes() == want[0].tobytes() and alt[:h].tobytes() == want[1].tobytes() and pid[:h].tobytes() == want[2].tobytes()
        assert pos[h] == 0x5A and alt[h] == 0x5A and pid[h] == 0x5A
        rc, n_hits, pos, _, _ = _raw(s, seq, [(0, 1500)], rates, 5, 0)
        assert rc == 0 and n_hits == h and pos[0] == 0x5A


def _raises(code, call, text=None):
    with pytest.raises(engine.KPError) as e:
        call()
    assert e.value.code == code, str(e.value)
    if text is not None:
        assert text in str(e.value), str(e.value)


def test_errors():
    seq = R.random_seq(np.random.RandomState(1), 300)
    s = engine.HostSpec()
    _raises(STATE, lambda: s.spec_simulate(seq, [(0, 300)], [], 1))
    # types A>C (two patterns), A>G, C>T: REF A has the types 0 and 1, REF C the type 5
    names, ptype = ["AAN", "BAN", "NAN", "NCN"], [0, 0, 1, 5]
    with _Session(3, names, ptype, True) as s:
        ok = [0.2, 0.5, 0.5, 1.0]
        assert len(s.spec_simulate(seq, [(0, 300)], ok, 1)[0]) > 50  # 0.5 + 0.5 and 1.0: exactly 1 is allowed
        for bad, text in ((float("nan"), "pattern 1"), (float("inf"), "pattern 1"), (-1e-9, "pattern 1")):
            _raises(ARG, lambda: s.spec_simulate(seq, [(0, 300)], [0.1, bad, 0.1, 0.1], 1), text)
        for bad in (float("nan"), float("inf"), -1.0):
            _raises(ARG, lambda: s.spec_simulate(seq, [(0, 300)], ok, 1, scale=bad), "scale")
        _raises(ARG, lambda: s.spec_simulate(seq, [(0, 300)], [0.2, 0.5 + 2.0 ** -52, 0.5, 1.0], 1), "REF A")
        _raises(ARG, lambda: s.spec_simulate(seq, [(0, 300)], [0.2, 0.5, 0.5, math.nextafter(1.0, 2.0)], 1), "REF C")
        _raises(ARG, lambda: s.spec_simulate(seq, [(0, 300)], ok, 1, scale=1.0000001), "REF")
        assert len(s.spec_simulate(seq, [(0, 300)], [0.6, 0.1, 0.1, 0.1], 1, scale=1.25)[0]) > 50  # (0.75 + 0.125)
        _raises(ARG, lambda: s.spec_simulate(seq, [(10, 20), (5, 8)], ok, 1), "region 1")
        _raises(ARG, lambda: s.spec_simulate(seq, [(10, 20), (19, 30)], ok, 1), "region 1")
        _raises(ARG, lambda: s.spec_simulate(seq, [(0, 5), (20, 10)], ok, 1), "region 1")
        _raises(ARG, lambda: s.spec_simulate(seq, [(0, 301)], ok, 1), "region 0")
        assert len(s.spec_simulate(seq, [(10, 20), (20, 20), (20, 30)], ok, 1)[0]) > 0
        with pytest.raises(ValueError):
            s.spec_simulate(seq, [(0, 300)], ok[:3], 1)
        with pytest.raises(ValueError):
            s.spec_simulate(seq, [(0, 300)], ok, -1)
        with pytest.raises(ValueError):
            s.spec_simulate(seq, [(0, 300)], ok, 1, contig_id=1 << 32)
        # null pointers
        L = engine.load()
        u64, u32 = ctypes.c_uint64, ctypes.c_uint32
        assert L.kp_spec_simulate(None, engine._ptr(seq), u64(300), u32(0), None, None, u64(0), engine._ptr(np.array(ok)),
                                  ctypes.c_double(1.0), u64(1), u32(0), u64(0), None, None, None, None) == ARG
        assert L.kp_spec_last_sim(None, None) == ARG
    _raises(STATE, lambda: s.spec_simulate(seq, [(0, 300)], ok, 1))


@pytest.mark.parametrize("k,fold,n_types", [(3, True, 6), (5, True, 6), (3, False, 12), (1, False, 12)])
def test_consistent_with_sites_and_typed_counting(k, fold, n_types):
    """The pattern of a simulated site's own type is the pattern that produced it, and counting the
    simulated sites by type gives the hits per type: the ALT is on the forward strand."""
    rng = np.random.RandomState(17 * k + n_types)
    names, ptype, _ = R.random_model(rng, k, fold, n_types, 4 if k > 1 else 1)
    rates = rng.uniform(0.02, 0.3, size=len(names))
    seq = R.random_seq(rng, 3000, lower=0.3, invalid=0.01)
    with _Session(k, names, ptype, fold) as s:
        pos, alt, pid = s.spec_simulate(seq, [(0, 3000)], rates, 2024, 1)
        assert len(pos) > 500 and np.array_equal(s.spec_sites(seq, pos, alt), pid)
    per_type = np.bincount(np.asarray(ptype)[pid], minlength=12)
    assert (per_type > 0).sum() == n_types
    counts, _, st = engine.HostSpec().seq_count_typed(k, fold, [(seq, None, (pos, alt))])
    assert st["sites"] == len(pos) and st["sites_skipped"] == 0
    for t, kind in enumerate(R.types(fold)):
        assert int(spectrum.type_column(k, counts, kind).sum()) == per_type[R.ALL_TYPES.index(kind)], kind


def test_statistics_of_a_draw():
    """200,000 random bases under a k = 3 model with rates in 0.01 .. 0.05: per type the hits lie
    within five binomial standard deviations of the expectation, summed over the positions of the
    type's patterns.  (Seed 20240 was kept after the oracle alone was inside the bound for it.)"""
    rng = np.random.RandomState(42)
    names, ptype, _ = R.random_model(rng, 3, True, 6, 5)
    rates = rng.uniform(0.01, 0.05, size=len(names))
    seq = R.random_seq(rng, 200_000, lower=0.2, invalid=0.001)
    with _Session(3, names, ptype, True) as s:
        track = s.spec_track(seq)
        pos, alt, pid = s.spec_simulate(seq, [(0, 200_000)], rates, 20240)
    hits = np.bincount(np.asarray(ptype)[pid], minlength=6)
    for t in range(6):
        ids = track[t % 3]
        r = rates[ids[(ids >= 0) & (np.asarray(ptype)[np.maximum(ids, 0)] == t)]]
        mean, sd = float(r.sum()), math.sqrt(float((r * (1.0 - r)).sum()))
        assert mean > 500 and abs(int(hits[t]) - mean) <= 5.0 * sd, (t, int(hits[t]), mean, sd)


def test_command_line(tmp_path, capsys):
    rng = np.random.RandomState(12)
    contigs = [("chr1", R.random_seq(rng, 2500, lower=0.3, invalid=0.004)), ("chr2", R.random_seq(rng, 10)),
               ("chr3", R.random_seq(rng, 1200, lower=0.1))]
    genome = str(tmp_path / "g.fa")
    R.write_fasta(genome, contigs)
    names, ptype, rates = _model(31, 5, True, 6, 7, 4, 0.01, 0.2)
    model = spectrum.Model(names, ptype, rates)
    model_file = str(tmp_path / "model.txt")
    model.write(model_file)
    base = ["--model", model_file, "--verbosity", "0"]
    out, out2 = str(tmp_path / "sim.txt"), str(tmp_path / "sim2.txt")
    assert spectrum.main(["simulate", genome, "--seed", "77", "-o", out, "--model", model_file], host=True) == 0
    err = capsys.readouterr().err
    rows, skipped = predict._site_lines(out)
    assert skipped == 0 and len(rows) > 300 and f"hits={len(rows)}\n" in err and "windows=" in err and "hits_A>C=" in err
    assert "hits_C>G=" not in err  # (type 4 has no pattern)
    seqs = dict(contigs)
    order = {"chr1": 0, "chr2": 1, "chr3": 2}
    keys = [(order[c], p) for c, p, _, _ in rows]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(chr(seqs[c][p - 1]).upper() == r and a in "ACGT" and a != r for c, p, r, a in rows)
    assert spectrum.main(["simulate", genome, "--seed", "77", "-o", out2] + base, host=True) == 0
    assert open(out, "rb").read() == open(out2, "rb").read()
    # the API gives the same sites; the contig id is the index in genome order
    api = list(spectrum.simulate(contigs, model, 77, host=True))
    assert [x[0] for x in api] == ["chr1", "chr2", "chr3"]
    assert [(c, int(p) + 1, chr(a)) for c, pos, alt, _ in api for p, a in zip(pos, alt)] == [(c, p, a) for c, p, _, a in rows]
    with _Session(5, names, ptype, True) as s:
        assert s.spec_simulate(contigs[2][1], [(0, 1200)], rates, 77, contig_id=2)[0].tobytes() == api[2][1].tobytes()
    # regions --observed counts every line
    with open(tmp_path / "all.bed", "w") as f:
        f.write("chr1 0 2500\nchr2 0 10\nchr3 0 1200\n")
    table = str(tmp_path / "table.txt")
    assert spectrum.main(["regions", genome, "--bed", str(tmp_path / "all.bed"), "--observed", out, "-o", table] + base,
                         host=True) == 0
    lines = [x.split() for x in open(table).read().splitlines()]
    col = lines[0].index("obs_total")
    assert sum(int(x[col]) for x in lines[1:]) == len(rows)
    # a --bed subset (overlapping regions, merged) changes no draw: the full run's lines inside it
    with open(tmp_path / "sub.bed", "w") as f:
        f.write("chr3 100 600\nchr1 1000 1500\nchr1 1400 2000\nchrX 0 5\nchr3 600 601\n")
    assert spectrum.main(["simulate", genome, "--seed", "77", "--bed", str(tmp_path / "sub.bed"), "-o", out2] + base,
                         host=True) == 0
    inside = [(c, p, r, a) for c, p, r, a in rows if (c == "chr1" and 1000 <= p - 1 < 2000) or (c == "chr3" and 100 <= p - 1 < 601)]
    assert predict._site_lines(out2)[0] == inside and len(inside) > 50
    # another replicate, another seed, a scale
    texts = set()
    for extra in (["--seed", "77", "--replicate", "1"], ["--seed", "78"], ["--seed", "77", "--scale", "0.5"]):
        assert spectrum.main(["simulate", genome, "-o", out2] + extra + base, host=True) == 0
        texts.add(open(out2).read())
    assert len(texts) == 3 and open(out).read() not in texts
    # errors: no seed; a scale that takes a REF base's rates above 1; a region past the contig
    with pytest.raises(SystemExit):
        spectrum.main(["simulate", genome, "-o", out2] + base, host=True)
    capsys.readouterr()
    assert spectrum.main(["simulate", genome, "--seed", "1", "--scale", "100", "-o", out2] + base, host=True) == 2
    assert "more than 1" in capsys.readouterr().err
    with open(tmp_path / "past.bed", "w") as f:
        f.write("chr2 0 11\n")
    assert spectrum.main(["simulate", genome, "--seed", "1", "--bed", str(tmp_path / "past.bed"), "-o", out2] + base,
                         host=True) == 2
