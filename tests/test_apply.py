"""A fitted partition applied to a count table, on the host: ``engine.apply_host``
(kp_apply_host, the kernels' per-row / per-pair / per-term code run serially),
``papa.PatternPartition``, ``apply.read_partition`` and ``apply.main(host=True)``.  Pinned to
the reference's recorded runs (tests/golden/cli5.json, greedy_cli.json: the counts, the
context -> pattern column and the LL line of each) and to brute force by
``Pattern.__contains__``.  Bar: everything equal, ll bit for bit."""
import io

import numpy as np
import pytest

from kmerpapa_amd import apply as A
from kmerpapa_amd import engine
from kmerpapa_amd.io_utils import KmerCounts
from kmerpapa_amd.papa import PatternPartition
from tests import apply_cases as C
from tests.fixtures import write_count_files


def _host(names, super_pat, k, codes, M, U, rates=None):
    return engine.apply_host(k, C.words(names), engine.pattern_word(super_pat), codes, M, U, rates)


@pytest.mark.parametrize("which", C.GOLDEN, ids=[x[1] for x in C.GOLDEN])
def test_recorded_runs(which):
    """The recorded partition applied to the table it was fitted on gives back the recorded
    p_pos / p_neg columns and the recorded LL, with no row unmatched (but the 256 k-mers
    outside NNCNN for ``super``) and no overlap."""
    rec, (names, counts, rates) = C.golden(which)
    table, gp = C.table5()
    pid, pM, pU, ll, st = A.apply_partition(names, table, rates, host=True)
    assert list(zip(pM.tolist(), pU.tolist())) == counts
    assert (st["unmatched"], st["multi"], st["overlap_pairs"], st["outside_super"]) == \
        (256 if which[1] == "super" else 0, 0, 0, 0)
    assert C.bits(ll) == C.bits([C.recorded_ll(rec)])
    # the class, which sorts the patterns: the same counts under the same names
    pp = PatternPartition(list(names), superPattern="NNCNN" if which[1] == "super" else gp)
    by_name = dict(zip(names, counts))
    assert pp.counts(table, host=True) == [by_name[str(p)] for p in pp.patterns]
    assert pp.check(host=True) == {"unmatched": 0, "multi": 0, "overlap_pairs": 0, "outside_super": 0}
    if which[1] == "fit_long":
        want = {x.split()[0]: x.split()[4] for x in rec["output"].splitlines()[1:]}
        assert [names[j] for j in pid.tolist()] == [want[x] for x in table]


def test_read_partition_formats():
    rec, (names, counts, rates) = C.golden(("cli5.json", "fit_long"))
    lines = rec["output"].splitlines()[1:]
    first = {}
    for x in lines:
        first.setdefault(x.split()[4], x.split()[5:])
    assert names == list(first)  # order of first appearance
    assert counts == [(int(v[1]), int(v[0])) for v in first.values()]
    assert [repr(r) for r in rates] == [v[2] for v in first.values()]  # the repr round trip
    short = "pattern p_neg p_pos p_rate\n" + "".join(f"{n} {' '.join(v)}\n" for n, v in first.items())
    assert A.read_partition(io.StringIO(short)) == (names, counts, rates)
    with pytest.raises(ValueError, match="not a kmerpapa output table"):
        A.read_partition(io.StringIO("k alpha P LL_test\n"))


@pytest.mark.parametrize("part", range(4))
def test_random_partitions_equal_brute_force(part):
    for i, (names, gp, k, codes, M, U, rates) in enumerate(C.random_cases()):
        if i % 4 == part:
            assert C.observed(_host(names, gp, k, codes, M, U, rates)) == C.expected(C.random_expected(i)), (i, gp, names)


def test_random_cases_cover_what_they_should():
    cases = C.random_cases()
    assert {7, 8, 9} <= {len(c[0]) for c in cases} and {1, 2, 3} == {np.asarray(c[4]).reshape(len(c[3]), -1).shape[1] for c in cases}
    assert any((c[6] == 0.0).any() and (c[6] == 1.0).any() for c in cases)
    assert any(int(np.max(c[4], initial=0)) >= 1 << 39 for c in cases)
    exp = [C.random_expected(i) for i in range(len(cases))]
    assert any(e[4]["unmatched"] for e in exp) and any(not e[4]["unmatched"] for e in exp)
    assert any(np.isinf(e[3]).any() for e in exp) and any(np.isfinite(e[3]).all() for e in exp)


@pytest.mark.parametrize("kind", C.BROKEN)
def test_broken_partitions(kind):
    names, sup, k, codes, M, U, kmers = C.broken_case(kind)
    exp = C.brute(names, sup, kmers, M, U, None)
    assert C.observed(_host(names, sup, k, codes, M, U)) == C.expected(exp)
    st = exp[4]
    if kind == "removed":
        assert st["unmatched"] > 0 and st["multi"] == 0 == st["overlap_pairs"]
    elif kind in ("duplicated", "widened"):
        assert st["multi"] > 0 and st["overlap_pairs"] > 0 and st["unmatched"] == 0
    else:
        assert st["outside_super"] > 0 and st["unmatched"] == 0 == st["multi"]


def test_edges_n0_n1_p1():
    z = np.zeros(0, np.int64)
    pid, pM, pU, ll, st = _host(["NA", "NC", "NK"], "NN", 2, np.zeros(0, np.uint64), z, z, [0.5, 0.0, 1.0])
    assert pid.shape == (0,) and pM.tolist() == [0, 0, 0] == pU.tolist()
    assert C.bits(ll) == C.bits([0.0])  # +0.0, as get_loss of all-zero counts
    assert (st["unmatched"], st["multi"], st["overlap_pairs"], st["outside_super"]) == (0, 0, 0, 0)
    pid, pM, pU, ll, st = _host(["NA", "NC", "NK"], "NN", 2, [C.codes_of(["GT"])[0]], [3], [5], [0.5, 0.25, 0.125])
    assert (pid.tolist(), pM.tolist(), pU.tolist()) == ([2], [0, 0, 3], [0, 0, 5])
    assert C.observed((pid, pM, pU, ll, st)) == C.expected(C.brute(["NA", "NC", "NK"], "NN", ["GT"], [3], [5], [0.5, 0.25, 0.125]))
    pid, pM, pU, ll, st = _host(["NM"], "NM", 2, C.codes_of(["AA", "CG", "TC"]), [1, 2, 4], [8, 16, 32])
    assert (pid.tolist(), pM.tolist(), pU.tolist(), st["unmatched"]) == ([0, -1, 0], [5], [40], 1)


def test_sparse_16mers():
    names, codes, M, U = C.sparse16()
    assert 4000 < codes.shape[0] <= 5000 and len(names) == 300
    pid, pM, pU, ll, st = _host(names, "N" * 16, 16, codes, M, U)
    epid, eM, eU, un, mu = C.brute_np(names, codes, 16, M, U)
    assert (un, mu) == (0, 0) == (st["unmatched"], st["multi"]) and st["overlap_pairs"] == 0
    assert pid.tolist() == epid.tolist() and pM.tolist() == eM.tolist() and pU.tolist() == eU.tolist()
    assert int(pM.sum()) == int(M.sum()) and int(pU.sum()) == int(U.sum())
    # the class on the same table: a sparse KmerCounts
    pp = PatternPartition(list(names), strandSymmetry=False)
    order = [names.index(str(p)) for p in pp.patterns]
    assert pp.counts(KmerCounts(16, codes, M, U), host=True) == [(int(eM[j]), int(eU[j])) for j in order]


@pytest.mark.parametrize("what", sorted(C.BAD))
def test_bad_arguments_are_kp_e_arg(what):
    with pytest.raises(engine.KPError) as e:
        C.bad_call(engine.apply_host, what)
    assert e.value.code == -1 and "kp_apply_host" in str(e.value)


def test_pattern_partition_interface():
    pats = ["NCN", "NAN"]
    pp = PatternPartition(pats)
    assert pats == ["NAN", "NCN"]  # sorted in place, as the reference does
    assert (len(pp), pp.pattern_length(), str(pp.superPattern)) == (2, 3, "NMN")
    assert str(pp["ACG"]) == "NCN" and str(pp["TAT"]) == "NAN" and pp["AGA"] is None
    assert str(pp) == "[PatternPartition:\n NAN 16\n NCN 16\n ---\n NMN 32]"
    assert str(PatternPartition(["NN"], strandSymmetry=False).superPattern) == "NN"
    with pytest.raises(AssertionError) as e:
        PatternPartition(["NAN", "NGN"])
    assert str(e.value) == "pattern #1 (NGN) is not a subpattern of the superPattern (NMN)"
    with pytest.raises(AssertionError) as e:
        PatternPartition(["NAN"])
    assert str(e.value) == "the patterns does not cover the superPattern (NMN)"
    # an overlap the cardinality check cannot see: NAN twice has NMN's 32 k-mers
    pp = PatternPartition(["NAN", "NAN"])
    assert pp.check(host=True) == {"unmatched": 0, "multi": 0, "overlap_pairs": 1, "outside_super": 0}


def test_pattern_partition_assign_counts_loglik():
    gp, names, kmers, M, U = C.full_case()
    table = KmerCounts(4, C.codes_of(kmers), M, U)  # two count columns
    pp = PatternPartition(list(names), superPattern=gp)
    sorted_names = [str(p) for p in pp.patterns]
    rates = np.linspace(0.01, 0.4, len(names))
    epid, eM, eU, ell, _ = C.brute(sorted_names, gp, kmers, M, U, rates)
    assert pp.assign(table, host=True).tolist() == epid
    assert pp.counts(table, host=True) == [(tuple(m), tuple(u)) for m, u in zip(eM, eU)]
    assert C.bits(pp.loglik(table, rates, host=True)) == C.bits(ell)
    one = KmerCounts(4, table.codes, M[:, 0], U[:, 0])
    assert pp.counts(one, host=True) == one.pattern_counts(sorted_names)
    assert isinstance(pp.loglik(one, rates, host=True), float)
    with pytest.raises(ValueError, match="5-mers"):
        pp.assign(C.table5()[0], host=True)


def _main(tmp_path, capsys, which, extra):
    rec, _ = C.golden(("cli5.json", which))
    pos, bg = write_count_files(5, str(tmp_path))
    part = tmp_path / "partition.txt"
    part.write_text(rec["output"])
    out = tmp_path / "applied.txt"
    capsys.readouterr()
    rc = A.main(["--partition", str(part), "-p", pos, "-b", bg, "-o", str(out)] + extra, host=True)
    return rec, rc, out.read_text(), capsys.readouterr().err


def test_main_short_output(tmp_path, capsys):
    rec, rc, text, err = _main(tmp_path, capsys, "fit", [])
    lines = rec["output"].splitlines()
    want = [lines[0] + " t_neg t_pos"] + [f"{x} {x.split()[1]} {x.split()[2]}" for x in lines[1:]]
    assert rc == 0 and text == "\n".join(want) + "\n"
    assert err == f"LL_test={C.recorded_ll(rec)!r}\n"


def test_main_long_output(tmp_path, capsys):
    rec, rc, text, err = _main(tmp_path, capsys, "fit_long", ["-l"])
    rows = sorted(x.split() for x in rec["output"].splitlines()[1:])
    want = ["context c_neg c_pos pattern p_rate"] + [f"{r[0]} {r[1]} {r[2]} {r[4]} {r[7]}" for r in rows]
    assert rc == 0 and text == "\n".join(want) + "\n"
    assert err == f"LL_test={C.recorded_ll(rec)!r}\n"


def test_main_super_pattern_and_overlap(tmp_path, capsys):
    # a partition of NNCNN over the full table: the other 256 k-mers are reported, not fatal
    rec, rc, text, err = _main(tmp_path, capsys, "super", ["--verbosity", "1"])
    assert rc == 0 and err == f"LL_test={C.recorded_ll(rec)!r}\nunmatched=256\n"
    # ... and none with the main program's -s filter
    rec, rc, text2, err = _main(tmp_path, capsys, "super", ["-s", "NNCNN"])
    assert rc == 0 and err == f"LL_test={C.recorded_ll(rec)!r}\n" and text2 == text
    # overlapping patterns: exit code 1 and a message
    part = tmp_path / "overlap.txt"
    lines = rec["output"].splitlines()
    part.write_text("\n".join(lines + [lines[1]]) + "\n")
    pos, bg = write_count_files(5, str(tmp_path))
    rc = A.main(["--partition", str(part), "-p", pos, "-b", bg, "-o", str(tmp_path / "o.txt")], host=True)
    assert rc == 1 and "not a partition: 1 pairs" in capsys.readouterr().err
