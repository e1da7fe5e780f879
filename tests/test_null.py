"""Per-region null tables (kp_spec_null, kp_null.h) on the host session (engine.HostSpec: the
kernel's per-window functions run serially) against the independent oracle tests/null_ref.py --
which bins tests/sim_ref.py's mutation sets, replicate by replicate -- with the identities the
header states (columns, regions, type sums), closed forms, the statistics of a table, the error
codes, ``null_summary`` and the command line.  Every comparison but the statistical one is exact
equality."""
import ctypes
import math

import numpy as np
import pytest

from kmerpapa_amd import engine, predict, spectrum
from tests import null_ref as N
from tests import sim_ref as S
from tests import spec_ref as R
from tests.test_simulate import CASES, _model, _raises, _Session

ARG, STATE = -1, -4


def _regions(n, k):
    """Overlapping, unordered, empty, touching both contig ends, shorter than k, repeated."""
    return np.array([(n // 2, n - 7), (0, 0), (0, k + 3), (5, 200), (100, 101), (300, 300), (n - 2, n), (5, 200), (0, n),
                     (n, n), (250, 250 + max(k - 1, 1)), (150, n // 2 + 9)], np.uint64)


@pytest.mark.parametrize("k,fold,n_types,leaves,empty", CASES, ids=[f"k{c[0]}_fold{int(c[1])}_T{c[2]}" for c in CASES])
def test_host_session_equals_the_oracle(k, fold, n_types, leaves, empty):
    rng = np.random.RandomState(10 * k + n_types)
    n = 1501
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.01)
    regs = _regions(n, k)
    hits = 0
    for tag, lo, hi in (("dense", 0.05, 0.3), ("sparse", 1e-4, 1e-4)):
        names, ptype, rates = _model(k + n_types, k, fold, n_types, leaves, empty, lo, hi)
        track = R.track(seq, names, ptype, fold)
        windows = sum(int((track[0, b:e] != R.INVALID).sum()) for b, e in regs.tolist())
        with _Session(k, names, ptype, fold) as s:
            for seed, contig, first, reps, scale in ((7, 0, 0, 3, 1.0), (2 ** 63 + 5, 3, 9, 2, 1.0 if tag == "dense" else 50.0)):
                ref = N.table(seq, names, ptype, rates, fold, regs, seed, contig, first, reps, scale, True, pid=track)
                for by_type in (False, True):
                    got = s.spec_null(seq, regs, rates, seed, contig, first, reps, scale, by_type)
                    want = ref if by_type else ref.sum(axis=2, dtype=np.uint32)
                    assert got.dtype == np.uint32 and got.shape == want.shape and got.tobytes() == want.tobytes(), (tag, seed)
                    st = s.spec_null_stats()
                    assert st["windows"] == windows and st["hits"] == int(ref.sum()) and st["null_ms"] == 0.0
                    assert st["draws"] % reps == 0 and st["draws"] <= windows * reps
                if fold:
                    assert not ref[:, :, 6:].any()
                hits += int(ref.sum()) if tag == "dense" else 0
    assert hits > 100  # (the comparison is not one of empty tables)


def _setup(seed=4, k=5, fold=True, n=4000, lo=0.02, hi=0.2):
    names, ptype, rates = _model(seed, k, fold, 6, 9, 2, lo, hi)
    seq = R.random_seq(np.random.RandomState(seed + 4), n, lower=0.3, invalid=0.005)
    return k, fold, names, ptype, rates, seq


def test_columns_regions_and_type_sums():
    k, fold, names, ptype, rates, seq = _setup()
    n = seq.shape[0]
    regs = _regions(n, k)
    with _Session(k, names, ptype, fold) as s:
        whole = s.spec_null(seq, regs, rates, 99, 2, 0, 5)
        assert whole.sum() > 500
        # a batch of replicates is a range of columns
        assert np.array_equal(s.spec_null(seq, regs, rates, 99, 2, 3, 2), whole[:, 3:5])
        assert np.array_equal(s.spec_null(seq, regs, rates, 99, 2, 4, 1), whole[:, 4:5])
        # a region's row does not depend on the other regions
        for r in (0, 3, 8, 11):
            assert np.array_equal(s.spec_null(seq, regs[r:r + 1], rates, 99, 2, 0, 5), whole[r:r + 1])
        assert np.array_equal(whole[3], whole[7]) and not whole[[1, 5, 9]].any()
        # the typed table sums to the untyped one
        typed = s.spec_null(seq, regs, rates, 99, 2, 0, 5, by_type=True)
        assert typed.shape == (len(regs), 5, 12) and np.array_equal(typed.sum(axis=2), whole) and not typed[:, :, 6:].any()
        assert (typed.sum(axis=(0, 1)) > 0).sum() == len(set(ptype))
        # column j is the simulate call of replicate j, binned
        for j in (0, 4):
            pos = np.sort(s.spec_simulate(seq, [(0, n)], rates, 99, 2, j)[0].astype(np.int64))
            want = np.searchsorted(pos, regs[:, 1].astype(np.int64)) - np.searchsorted(pos, regs[:, 0].astype(np.int64))
            assert np.array_equal(whole[:, j], want)
        # seed, contig and scale all enter
        assert not np.array_equal(s.spec_null(seq, regs, rates, 98, 2, 0, 5), whole)
        assert not np.array_equal(s.spec_null(seq, regs, rates, 99, 3, 0, 5), whole)
        assert s.spec_null(seq, regs, rates, 99, 2, 0, 5, scale=0.5).sum() < 0.7 * whole.sum()


@pytest.mark.parametrize("k,fold", [(3, True), (3, False), (5, True)])
def test_closed_forms(k, fold):
    rng = np.random.RandomState(k + fold)
    names, ptype, _ = R.random_model(rng, k, fold, 6, 5, empty=3)
    n = 2000
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.01)
    track = R.track(seq, names, ptype, fold)
    regs = _regions(n, k)
    with _Session(k, names, ptype, fold) as s:
        for t in sorted(set(ptype)):
            rates = np.array([1.0 if x == t else 0.0 for x in ptype])
            ids = track[t % 3]
            own = np.concatenate([[0], np.cumsum((ids >= 0) & (np.asarray(ptype)[np.maximum(ids, 0)] == t))])
            want = (own[regs[:, 1].astype(np.intp)] - own[regs[:, 0].astype(np.intp)]).astype(np.uint32)
            got = s.spec_null(seq, regs, rates, 11, 0, 5, 4, by_type=True)
            assert want.sum() > 50 and np.array_equal(got[:, :, t], np.repeat(want[:, None], 4, axis=1))
            assert np.array_equal(got.sum(axis=2), got[:, :, t])
            assert s.spec_null_stats()["draws"] == 4 * int(want.sum()) == s.spec_null_stats()["hits"]
        for rates, scale in ((np.zeros(len(names)), 1.0), (np.ones(len(names)), 0.0)):
            got = s.spec_null(seq, regs, rates, 11, 0, 0, 3, scale)
            assert got.shape == (len(regs), 3) and not got.any()
            st = s.spec_null_stats()
            assert st["hits"] == 0 and st["draws"] == 0 and st["windows"] > 1000


def test_statistics_of_a_table():
    """One region of 20,000 random bases, 300 replicates, k = 3 with rates in 0.01 .. 0.05: the
    mean over the replicates lies within five standard errors of kp_spec_regions' expectation, the
    standard error from the model's Poisson-binomial variance sum p (1 - p) over the windows, not
    from the sample.  (Seed 20241: the reference draw below, Philox written out on numpy, passes
    the same bound by itself, and the table equals it.)"""
    rng = np.random.RandomState(43)
    names, ptype, _ = R.random_model(rng, 3, True, 6, 5)
    rates = rng.uniform(0.01, 0.05, size=len(names))
    n, reps, seed = 20_000, 300, 20241
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.001)
    with _Session(3, names, ptype, True) as s:
        track = s.spec_track(seq)
        _, _, expected = s.spec_regions(seq, [(0, n)], rates)
        got = s.spec_null(seq, [(0, n)], rates, seed, 1, 0, reps)
    p = np.where(track >= 0, rates[np.maximum(track, 0)], 0.0).sum(axis=0)  # per position: the three slots' rates
    mean, se = float(expected.sum()), math.sqrt(float((p * (1.0 - p)).sum()) / reps)
    assert mean > 1000 and abs(mean - float(p.sum())) < 1e-6 * mean
    # the reference draw: u < c2 at the valid windows
    valid = np.flatnonzero(track[0] != R.INVALID)
    assert N.uniforms(seed, 1, valid[:3], [0, 299]).tolist() == [[S.uniform(seed, 1, int(x), j) for j in (0, 299)]
                                                                  for x in valid[:3]]
    c = np.where(track >= 0, rates[np.maximum(track, 0)], 0.0)
    c2 = (c[0] + c[1]) + c[2]
    ref = (N.uniforms(seed, 1, valid, np.arange(reps)) < c2[valid, None]).sum(axis=0)
    assert abs(float(ref.mean()) - mean) <= 5.0 * se, (float(ref.mean()), mean, se)
    assert np.array_equal(got[0], ref)
    assert abs(float(got.mean()) - mean) <= 5.0 * se


def _raw(s, seq, regions, rates, n_reps, rep_first=0, by_type=0, scale=1.0, counts=True, fill=0x5A5A5A5A):
    """kp_spec_null itself: ``(rc, counts)`` with the output pre-filled."""
    seq = np.ascontiguousarray(seq, np.uint8)
    reg = np.asarray(regions, np.uint64).reshape(-1, 2)
    rb, re = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    rates = np.ascontiguousarray(rates, np.float64)
    out = np.full(min(reg.shape[0] * max(n_reps, 1) * (12 if by_type else 1), 1 << 12) + 1, fill, np.uint32)  # (calls that
    # would need more are the ones refused)
    p = engine._ptr
    rc = engine.load().kp_spec_null(s._h, p(seq), ctypes.c_uint64(seq.shape[0]), ctypes.c_uint32(0), p(rb), p(re),
                                    ctypes.c_uint64(reg.shape[0]), p(rates), ctypes.c_double(scale), ctypes.c_uint64(1),
                                    ctypes.c_uint32(rep_first), ctypes.c_uint32(n_reps), by_type, p(out) if counts else None)
    return rc, out


def _fails(s, text, *args, **kw):
    rc, out = _raw(s, *args, **kw)
    assert rc == ARG and text in engine.load().kp_last_error().decode(), engine.load().kp_last_error()
    assert np.all(out == 0x5A5A5A5A)  # (untouched)


def test_errors():
    seq = R.random_seq(np.random.RandomState(1), 300)
    s = engine.HostSpec()
    _raises(STATE, lambda: s.spec_null(seq, [(0, 300)], [], 1))
    # types A>C (two patterns), A>G, C>T: REF A has the types 0 and 1, REF C the type 5
    names, ptype = ["AAN", "BAN", "NAN", "NCN"], [0, 0, 1, 5]
    with _Session(3, names, ptype, True) as s:
        ok = [0.2, 0.5, 0.5, 1.0]
        reg = [(0, 300), (20, 30)]
        rc, out = _raw(s, seq, reg, ok, 3)
        assert rc == 0 and out[:6].sum() > 100 and out[6] == 0x5A5A5A5A
        for bad in (float("nan"), float("inf"), -1e-9):
            _fails(s, "pattern 1", seq, reg, [0.1, bad, 0.1, 0.1], 3)
        for bad in (float("nan"), float("inf"), -1.0):
            _fails(s, "scale", seq, reg, ok, 3, scale=bad)
        _fails(s, "REF A", seq, reg, [0.2, 0.5 + 2.0 ** -52, 0.5, 1.0], 3)
        _fails(s, "REF C", seq, reg, [0.2, 0.5, 0.5, math.nextafter(1.0, 2.0)], 3)
        _fails(s, "REF", seq, reg, ok, 3, scale=1.0000001)
        _fails(s, "region 1", seq, [(0, 5), (20, 10)], ok, 3)
        _fails(s, "region 0", seq, [(0, 301)], ok, 3)
        _fails(s, "no replicates", seq, reg, ok, 0)
        _fails(s, "2^32", seq, reg, ok, 2, rep_first=2 ** 32 - 1)
        _fails(s, "2^32", seq, reg, ok, 2 ** 32 - 1, rep_first=2, by_type=1)
        rc, out = _raw(s, seq, reg, ok, 1, rep_first=2 ** 32 - 1)  # (the last replicate there is)
        assert rc == 0 and out[2] == 0x5A5A5A5A
        rc, _ = _raw(s, seq, reg, ok, 3, counts=False)
        assert rc == ARG and "null counts" in engine.load().kp_last_error().decode()
        assert engine.load().kp_spec_last_null(None, None) == ARG
        with pytest.raises(ValueError):
            s.spec_null(seq, reg, ok[:3], 1)
        with pytest.raises(ValueError):
            s.spec_null(seq, reg, ok, -1)
        with pytest.raises(ValueError):
            s.spec_null(seq, reg, ok, 1, n_reps=1 << 32)
        _raises(ARG, lambda: s.spec_null(seq, reg, ok, 1, n_reps=0), "no replicates")
        _raises(ARG, lambda: s.spec_null(seq, reg, ok, 1, rep_first=(1 << 32) - 2, n_reps=3), "2^32")
        assert s.spec_null(seq, np.zeros((0, 2)), ok, 1, n_reps=4).shape == (0, 4)
    _raises(STATE, lambda: s.spec_null(seq, [(0, 300)], ok, 1))


def test_null_summary():
    total = np.array([[0, 0, 0, 0], [1, 2, 3, 6], [5, 5, 5, 5], [4000000000, 0, 4000000000, 1]], np.uint32)
    got = spectrum.null_summary(total)
    assert sorted(got) == ["max", "mean", "min", "var"]
    assert got["mean"] == [0.0, 3.0, 5.0, 8000000001 / 4]
    assert got["var"] == [0.0, (4 * 50 - 144) / 12, 0.0, (4 * (2 * 4000000000 ** 2 + 1) - 8000000001 ** 2) / 12]
    assert got["min"] == [0, 1, 5, 0] and got["max"] == [0, 6, 5, 4000000000]
    # obs above, below and equal to every draw; between the draws
    got = spectrum.null_summary(total[:3], [1, 0, 5])
    assert got["p_upper"] == [1 / 5, 5 / 5, 5 / 5] and got["p_lower"] == [5 / 5, 1 / 5, 5 / 5]
    got = spectrum.null_summary(total[1:2], [3])
    assert got["p_upper"] == [3 / 5] and got["p_lower"] == [4 / 5]
    got = spectrum.null_summary(total[1:2], [7])
    assert got["p_upper"] == [1 / 5] and got["p_lower"] == [5 / 5]
    one = spectrum.null_summary(np.array([[3], [0]]), [3, 1])
    assert one["mean"] == [3.0, 0.0] and all(math.isnan(x) for x in one["var"]) and one["min"] == one["max"] == [3, 0]
    assert one["p_upper"] == [1.0, 0.5] and one["p_lower"] == [1.0, 1.0]
    with pytest.raises(ValueError):
        spectrum.null_summary(np.zeros((2, 0)))
    with pytest.raises(ValueError):
        spectrum.null_summary(total, [1, 2])


def test_null_table_batching_and_contig_ids():
    rng = np.random.RandomState(5)
    contigs = [("a", R.random_seq(rng, 900, lower=0.2, invalid=0.01)), ("b", R.random_seq(rng, 4)),
               ("c", R.random_seq(rng, 700))]
    names, ptype, rates = _model(31, 5, True, 6, 7, 4, 0.01, 0.2)
    model = spectrum.Model(names, ptype, rates)
    regions = {"a": [(0, 900), (100, 300), (50, 120)], "c": [(600, 700), (0, 700)], "zz": [(0, 5)]}
    stats = {}
    whole = spectrum.null_table(contigs, model, regions, 8, 7, first=2, by_type=True, host=True, stats=stats)
    assert sorted(whole) == ["a", "c"] and whole["a"].shape == (3, 7, 12) and whole["c"].shape == (2, 7, 12)
    assert stats["hits"] == int(whole["a"].sum()) + int(whole["c"].sum()) > 200
    for budget in (1, 12 * 3, 12 * 7 * 2):
        got = spectrum.null_table(contigs, model, regions, 8, 7, first=2, by_type=True, host=True, budget=budget)
        assert all(np.array_equal(got[x], whole[x]) for x in whole)
    flat = spectrum.null_table(contigs, model, regions, 8, 7, first=2, host=True, budget=5)
    assert all(np.array_equal(flat[x], whole[x].sum(axis=2)) for x in whole)
    # the contig enters by its index in genome order, as in simulate
    sets = {(name, j): pos for j in (2, 8) for name, pos, _, _ in spectrum.simulate(contigs, model, 8, replicate=j, host=True)}
    assert np.array_equal(flat["c"][1, [0, 6]], [len(sets["c", 2]), len(sets["c", 8])])
    assert np.array_equal(flat["a"][0, [0, 6]], [len(sets["a", 2]), len(sets["a", 8])])
    with pytest.raises(ValueError):
        spectrum.null_table(contigs, model, regions, 8, 0, host=True)


def test_command_line(tmp_path, capsys):
    rng = np.random.RandomState(12)
    contigs = [("chr1", R.random_seq(rng, 2500, lower=0.3, invalid=0.004)), ("chr2", R.random_seq(rng, 10)),
               ("chr3", R.random_seq(rng, 1200, lower=0.1))]
    genome = str(tmp_path / "g.fa")
    R.write_fasta(genome, contigs)
    names, ptype, rates = _model(31, 5, True, 6, 7, 4, 0.01, 0.2)
    spectrum.Model(names, ptype, rates).write(str(tmp_path / "model.txt"))
    base = ["--model", str(tmp_path / "model.txt"), "--verbosity", "0"]
    bed = str(tmp_path / "genes.bed")
    regs = [("chr3", 100, 600, "g1"), ("chr1", 1000, 1500, "g2"), ("chr1", 1400, 2000, "g3"), ("chrX", 0, 5, "g4"),
            ("chr3", 600, 601, "g5"), ("chr1", 0, 2500, "g6"), ("chr2", 0, 10, "g7"), ("chr1", 7, 7, "g8")]
    with open(bed, "w") as f:
        f.write("".join(f"{c} {b} {e} {x}\n" for c, b, e, x in regs))
    R_, seed = 6, 77
    sims = []  # per replicate: the simulate subcommand's lines per region
    for j in range(R_ + 2):
        out = str(tmp_path / f"sim{j}.txt")
        assert spectrum.main(["simulate", genome, "--seed", str(seed), "--replicate", str(j), "-o", out] + base, host=True) == 0
        rows = predict._site_lines(out)[0]
        sims.append([sum(1 for c, p, _, _ in rows if c == chrom and b <= p - 1 < e) for chrom, b, e, _ in regs])
    sims = np.array(sims).T  # [region, replicate]
    assert sims[5].min() > 100
    table, draws = str(tmp_path / "null.txt"), str(tmp_path / "draws.txt")
    args = ["null", genome, "--bed", bed, "--replicates", str(R_), "--seed", str(seed), "--draws", draws, "--observed",
            str(tmp_path / "sim1.txt"), "-o", table]
    assert spectrum.main(args + ["--model", str(tmp_path / "model.txt")], host=True) == 0
    err = capsys.readouterr().err
    assert "unknown_contig_regions=1\n" in err and f"hits={int(sims[:, :R_].sum())}\n" in err and "draws=" in err
    got = np.array([[int(x) for x in line.split()] for line in open(draws).read().splitlines()])
    assert np.array_equal(got, sims[:, :R_])
    lines = [x.split() for x in open(table).read().splitlines()]
    head = lines[0]
    assert head == ["#chrom", "start", "end", "name", "valid", "invalid", "exp_total", "sim_mean", "sim_var", "sim_min",
                    "sim_max", "obs_total", "p_upper", "p_lower"]
    assert [x[:4] for x in lines[1:]] == [[c, str(b), str(e), x] for c, b, e, x in regs]
    # the regions subcommand's own columns
    reg_out = str(tmp_path / "regions.txt")
    assert spectrum.main(["regions", genome, "--bed", bed, "--observed", str(tmp_path / "sim1.txt"), "-o", reg_out] + base,
                         host=True) == 0
    want = [x.split() for x in open(reg_out).read().splitlines()]
    for name in ("valid", "invalid", "exp_total", "obs_total"):
        assert [x[head.index(name)] for x in lines[1:]] == [x[want[0].index(name)] for x in want[1:]], name
    summary = spectrum.null_summary(got, sims[:, 1])
    for i, x in enumerate(lines[1:]):
        row = dict(zip(head, x))
        assert int(row["obs_total"]) == sims[i, 1]
        assert row["p_upper"] == repr((1 + int((got[i] >= sims[i, 1]).sum())) / (R_ + 1)) == repr(summary["p_upper"][i])
        assert row["p_lower"] == repr((1 + int((got[i] <= sims[i, 1]).sum())) / (R_ + 1))
        assert row["sim_mean"] == repr(summary["mean"][i]) and row["sim_var"] == repr(summary["var"][i])
        assert (int(row["sim_min"]), int(row["sim_max"])) == (got[i].min(), got[i].max())
    assert lines[4][4:] == ["0", "0", "0.0", "0.0", "0.0", "0", "0", "0", "1.0", "1.0"]  # (chrX)
    # --first-replicate shifts the columns; a file and standard output hold the same text
    assert spectrum.main(["null", genome, "--bed", bed, "--replicates", "3", "--seed", str(seed), "--first-replicate", "5",
                          "--draws", draws] + base, host=True) == 0
    shifted = np.array([[int(x) for x in line.split()] for line in open(draws).read().splitlines()])
    assert np.array_equal(shifted, sims[:, 5:8])
    text = capsys.readouterr().out.splitlines()
    assert text[0].split()[-4:] == ["sim_mean", "sim_var", "sim_min", "sim_max"] and len(text) == len(regs) + 1
    # --by-type: the same columns per type of the model, summing to the totals; --scale scales exp_total
    assert spectrum.main(args + ["--by-type", "--scale", "0.5"] + base, host=True) == 0
    typed = [x.split() for x in open(table).read().splitlines()]
    kinds = [R.ALL_TYPES[t] for t in sorted(set(ptype))]
    assert typed[0][14:21] == [f"sim_mean_{kinds[0]}", f"sim_var_{kinds[0]}", f"sim_min_{kinds[0]}", f"sim_max_{kinds[0]}",
                               f"obs_{kinds[0]}", f"p_upper_{kinds[0]}", f"p_lower_{kinds[0]}"]
    assert len(typed[0]) == 14 + 7 * len(kinds)
    for x, full in zip(typed[1:], lines[1:]):
        row = dict(zip(typed[0], x))
        assert float(row["exp_total"]) == 0.5 * float(full[6]) and row["obs_total"] == full[11]
        assert sum(int(row[f"obs_{t}"]) for t in kinds) == int(row["obs_total"])
        assert abs(sum(float(row[f"sim_mean_{t}"]) for t in kinds) - float(row["sim_mean"])) < 1e-9
    # errors
    for bad in (["--replicates", "0"], ["--replicates", "2", "--first-replicate", str(2 ** 32 - 1)], ["--seed", "-1"]):
        argv = ["null", genome, "--bed", bed, "--replicates", "2", "--seed", "1"] + bad + base
        assert spectrum.main(argv, host=True) == 2
    assert "input error" in capsys.readouterr().err
    assert spectrum.main(["null", genome, "--bed", bed, "--replicates", "2", "--seed", "1", "--scale", "100"] + base,
                         host=True) == 2
    assert "more than 1" in capsys.readouterr().err
