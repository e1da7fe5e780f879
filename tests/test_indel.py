"""Indel breakpoint counts on the host session (kp_indel.h with ctx = NULL, the serial definition
the GPU tests compare the kernels with) against tests/indel_ref.py, an independent restatement of
the header's semantics, and against the brute-force definition of an equivalence class.  No GPU."""
import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, seqio
from tests import indel_ref as R
from tests import seq_ref as S


def _sites(sites):
    """indel_ref sites as the arrays the engine takes."""
    return engine.indel_sites([s[1] for s in sites], [s[2] if s[0] == "del" else 0 for s in sites],
                              [s[2] if s[0] == "ins" else "" for s in sites], [s[3] for s in sites])


def _host(seq, k, sites, both, how="left", seed=0, contig=0, scan=True, regions=None):
    arr = np.frombuffer(seq.encode("latin-1"), np.uint8)
    return engine.seq_indel_host_contig(k, both, arr, contig, None if scan and regions is None else (regions if scan else False),
                                        _sites(sites), how, seed)


def _same_as_ref(seq, k, sites, both, how="left", seed=0, contig=0, regions=None):
    cols, bg, st, res = _host(seq, k, sites, both, how, seed, contig, regions=regions)
    rcols, rbg, rst, rres = R.count(seq, k, sites, both, how, seed, contig, regions=regions)
    for i, name in enumerate(R.COLUMNS):
        assert np.array_equal(cols[i], S.dense(rcols[name], k)), name
    assert np.array_equal(bg, S.dense(rbg, k))
    assert {x: st[x] for x in S.COUNT_STATS} == rst
    assert res.tolist() == [list(r) for r in rres]
    return cols, bg, st, res


def _random_sites(rng, n_contigs=300):
    """Random pure-ACGT contigs of 1..60 bases over a two-letter-heavy alphabet and one insertion
    and one deletion of length 1..8 on each, the indel often copied from the bases next to it."""
    out = []
    for _ in range(n_contigs):
        n = int(rng.randint(1, 61))
        seq = "".join(rng.choice(list("AAAACCCCGT"), size=n))
        b = int(rng.randint(0, n + 1))
        L = int(rng.randint(1, 9))
        ins = seq[b:b + L] if rng.rand() < 0.6 and b + L <= n else "".join(rng.choice(list("AC"), size=L))
        sites = [("ins", b, ins, int(rng.randint(0, 1 << 40)))]
        L = int(rng.randint(1, min(8, n) + 1))
        sites.append(("del", int(rng.randint(0, n - L + 1)), L, int(rng.randint(0, 1 << 40))))
        out.append((seq, sites))
    return out


@pytest.fixture(scope="module")
def random_cases():
    return _random_sites(np.random.RandomState(11))


def test_intervals_equal_the_brute_force_class(random_cases):
    ambiguous = total = 0
    for seq, sites in random_cases:
        res = _host(seq, 2, sites, True, scan=False)[3]
        for site, (lo, hi, p) in zip(sites, res.tolist()):
            assert (lo, hi) == R.brute_interval(seq, site) == R.interval(seq, site), (seq, site)
            assert p == lo
            ambiguous += hi > lo
            total += 1
    assert total >= 600 and 3 * ambiguous >= total, (ambiguous, total)


@pytest.mark.parametrize("how", ["left", "right", "sample"])
def test_every_representative_counts_the_same(random_cases, how):
    for seq, sites in random_cases[:120]:
        for site in sites:
            ref = _host(seq, 4, [site], True, how, seed=77, contig=3)
            lo, hi = R.interval(seq, site)
            for p in range(lo, hi + 1):
                other = R.representative(seq, site, p)
                assert R.mutated(seq, other) == R.mutated(seq, site)
                got = _host(seq, 4, [other], True, how, seed=77, contig=3)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (seq, site, other)
                assert got[3].tolist() == ref[3].tolist() and got[2] == ref[2]


@pytest.mark.parametrize("both", [True, False], ids=["both", "forward"])
@pytest.mark.parametrize("how", ["left", "right", "sample"])
def test_random_contigs_equal_the_reference(random_cases, both, how):
    for i, (seq, sites) in enumerate(random_cases[:150]):
        _same_as_ref(seq, (2, 4, 6)[i % 3], sites, both, how, seed=5 + i, contig=i)


def test_sample_draws_differ_by_key_seed_and_contig():
    seq = "G" + "A" * 50 + "C"
    rows = {}
    for seed, contig, key in ((1, 0, 0), (1, 0, 1), (2, 0, 0), (1, 1, 0), (1 << 40 | 1, 0, 1 << 35)):
        res = _same_as_ref(seq, 2, [("del", 20, 1, key), ("ins", 7, "A", key)], True, "sample", seed, contig)[3]
        assert all(lo == 1 and lo <= p <= hi for lo, hi, p in res.tolist()) and res[0, 1] == 50 and res[1, 1] == 51
        rows[seed, contig, key] = tuple(res[:, 2].tolist())
    assert len(set(rows.values())) >= 4


def test_explicit_runs():
    # a run reaching position 0 and one reaching n; N cuts a run; lower case continues it
    seq = "AAAAGTCNCCCcccTTT"
    n = len(seq)
    sites = [("del", 2, 1, 0), ("ins", 1, "A", 1), ("del", n - 1, 1, 2), ("ins", n, "T", 3), ("del", 9, 1, 4),
             ("ins", 12, "c", 5), ("del", 8, 1, 6), ("ins", 7, "C", 7)]
    res = _same_as_ref(seq, 2, sites, True)[3].tolist()
    assert res[0][:2] == [0, 3] and res[1][:2] == [0, 4]
    assert res[2][:2] == [n - 3, n - 1] and res[3][:2] == [n - 3, n]
    assert res[4][:2] == [8, 13] and res[5][:2] == [8, 14]
    assert res[6][:2] == [8, 13]
    assert res[7][:2] == [6, 7]  # (the N equals nothing: the insertion moves over the C before it only)
    # an insertion longer than the repeat unit, and one of 70 bases
    res = _same_as_ref("GACACACT", 4, [("ins", 2, "CA", 0), ("ins", 1, "ACAC", 1)], True)[3].tolist()
    assert res[0][:2] == [1, 7] and res[1][:2] == [1, 7]
    unit = "ACGGT" * 14
    seq = "CC" + unit * 2 + "ACGA"
    res = _same_as_ref(seq, 6, [("ins", 2 + 70, unit, 0), ("del", 2 + 35, 70, 1)], True, "right")[3].tolist()
    assert res[0][:2] == [2, 2 + 140 + 3] and res[1][:2] == [2, 2 + 70 + 3]


def test_explicit_edges():
    # a deletion of a whole contig; insertions at b = 0 and b = n are skipped (the window runs off)
    cols, bg, st, res = _same_as_ref("ACGT", 2, [("del", 0, 4, 0), ("ins", 0, "G", 1), ("ins", 4, "G", 2)], True)
    assert st["sites"] == 0 and st["sites_skipped"] == 3 and not cols.any()
    assert res.tolist() == [[0, 0, 0], [0, 0, 0], [4, 4, 4]]
    # duplicates count as often as they occur, in both columns
    cols, _, st, _ = _same_as_ref("TTGACGTCAGG", 4, [("del", 4, 2, 0)] * 3 + [("ins", 5, "T", 1)] * 2, False)
    assert st["sites"] == 5 and cols[1].sum() == 3 and cols[2].sum() == 3 and cols[0].sum() == 2
    # n = 0 and n < k
    cols, bg, st, res = _same_as_ref("", 2, [("ins", 0, "A", 0)], True)
    assert st["sites_skipped"] == 1 and st["windows"] == 0 and res.tolist() == [[0, 0, 0]]
    cols, bg, st, _ = _same_as_ref("ACG", 4, [("del", 1, 1, 0), ("ins", 2, "T", 0)], True)
    assert st["sites_skipped"] == 2 and not bg.any()
    # placement first, the validity check after it: the leftmost placement's window holds the N,
    # the passed placement's does not, and the site is skipped, not re-placed
    _, _, st, res = _same_as_ref("GNAAAAAACG", 4, [("del", 6, 1, 0)], True)
    assert res.tolist() == [[2, 7, 2]] and st["sites_skipped"] == 1
    _, _, st, res = _same_as_ref("GNAAAAAACG", 4, [("del", 3, 1, 0)], True, "right")
    assert res.tolist() == [[2, 7, 7]] and st["sites"] == 1


def _rc_index(k):
    return np.array([S.dense({S.revcomp(S.kmer_of(c, k)): 1}, k).argmax() for c in range(4 ** k)])


@pytest.mark.parametrize("k", [2, 4, 6])
def test_table_invariants(k):
    rng = np.random.RandomState(19 + k)
    seq = S.text(S.random_seq(rng, 700, lower=0.2, invalid=0.01, letters="AACCGT")) + "ACGT" * 3 + "GAATTC"
    n = len(seq)
    sites = []
    for i in range(150):
        L = int(rng.randint(1, 6))
        sites.append(("del", int(rng.randint(0, n - L + 1)), L, i))
        sites.append(("ins", int(rng.randint(0, n + 1)), "".join(rng.choice(list("ACGT"), size=L)), i))
    cols, bg, st, _ = _same_as_ref(seq, k, sites, True)
    rc = _rc_index(k)
    assert np.array_equal(cols[0], cols[0][rc]) and np.array_equal(bg, bg[rc])
    assert np.array_equal(cols[2], cols[1][rc])
    assert int(bg.sum()) == 2 * st["windows"] and st["windows"] > 600
    fwd = _same_as_ref(seq, k, sites, False)
    assert int(fwd[1].sum()) == st["windows"] and np.array_equal(fwd[1] + fwd[1][rc], bg)
    assert np.array_equal(fwd[0][1] + fwd[0][2][rc], cols[1])
    regions = np.array([(0, 10), (300, 301), (650, n)])
    _same_as_ref(seq, k, sites[:10], True, regions=regions)


def test_a_palindromic_window_gets_two():
    _, bg, st, _ = _same_as_ref("ACGT", 4, [], True)
    assert st["windows"] == 1 and bg[int(S.dense({"ACGT": 1}, 4).argmax())] == 2 and bg.sum() == 2
    host = engine.HostSeq()
    got, st = host.seq_count_strands(4, True, [(np.frombuffer(b"ACGTT", np.uint8), None)])
    assert got.sum() == 4 and got.max() == 2 and st["windows"] == 2
    got, st = host.seq_count_strands(3, False, [(np.frombuffer(b"ACGTT", np.uint8), None)])  # (any k, forward)
    assert got.sum() == 3 == st["windows"]


def _code(e):
    return e.value.code


def test_error_calls():
    host = engine.HostSeq()
    seq = np.frombuffer(b"ACGTACGTAC", np.uint8)
    for k in (3, 0, 16, 15, -2):
        with pytest.raises(engine.KPError) as e:
            host.seq_begin_indel(k)
        assert _code(e) == -1
    for k in (0, 16):
        with pytest.raises(engine.KPError) as e:
            host.seq_begin_strands(k)
        assert _code(e) == -1
    with pytest.raises(engine.KPError) as e:  # no session
        host.seq_indels(seq, 0, _sites([("ins", 1, "A", 0)]))
    assert _code(e) == -4
    host.seq_begin_indel(14)
    host.seq_end_typed(False, False)
    host.seq_begin_indel(4)
    try:
        for call in (lambda: host.seq_sites(seq, [1]), lambda: host.seq_sites_typed(seq, [1], b"C"),
                     lambda: host.seq_begin_indel(4), lambda: engine._check(engine.load().kp_seq_end(None, None, None))):  # (an indel session ends typed)
            with pytest.raises(engine.KPError) as e:
                call()
            assert _code(e) == -4
        bad = [[("ins", 11, "A", 0)], [("del", 10, 1, 0)], [("del", 8, 3, 0)], [("ins", 3, "", 0)], [("ins", 3, "AN", 0)],
               [("ins", 3, "A", 0), ("del", 11, 1, 0)]]
        for sites in bad:
            with pytest.raises(engine.KPError) as e:
                host.seq_indels(seq, 0, _sites(sites))
            assert _code(e) == -1, sites
        assert "site 1" in str(e.value)
        with pytest.raises(engine.KPError) as e:  # both an insertion and a deletion
            host.seq_indels(seq, 0, engine.indel_sites([3], [2], ["A"]))
        assert _code(e) == -1 and "both" in str(e.value)
        assert host.seq_stats()["sites"] == 0  # (nothing ran)
        host.seq_indels(seq, 0, _sites([("ins", 10, "A", 0), ("del", 9, 1, 0), ("del", 0, 10, 0)]))
    finally:
        cols, bg = host.seq_end_typed()
    assert not cols.any() and not bg.any()
    host.seq_begin_strands(4, True)
    try:
        with pytest.raises(engine.KPError) as e:
            host.seq_sites(seq, [1])
        assert _code(e) == -4
        with pytest.raises(engine.KPError) as e:
            host.seq_indels(seq, 0, _sites([("ins", 1, "A", 0)]))
        assert _code(e) == -4
    finally:
        host.seq_end(False, False)
    for begin in (host.seq_begin, host.seq_begin_typed):  # plain and typed sessions take no indels
        begin(3, True)
        try:
            with pytest.raises(engine.KPError) as e:
                host.seq_indels(seq, 0, _sites([("ins", 1, "A", 0)]))
            assert _code(e) == -4
        finally:
            (host.seq_end if begin == host.seq_begin else host.seq_end_typed)(False, False)


def test_existing_begin_calls_behave_as_before():
    rng = np.random.RandomState(3)
    seq = S.random_seq(rng, 400, lower=0.2, invalid=0.01)
    sites = rng.randint(0, 400, size=50)
    for k, fold in ((3, 1), (5, 0), (4, 0), (7, 1)):
        pos, bg, st = engine.seq_host(k, fold, [(seq, None, sites)])
        rpos, rbg, rst = S.count(k, fold, [(seq, None, sites)])
        assert np.array_equal(pos, S.dense(rpos, k)) and np.array_equal(bg, S.dense(rbg, k))
        assert {x: st[x] for x in S.COUNT_STATS} == rst
        typed = engine.HostSeq().seq_count_typed(k, fold, [(seq, None, None)])
        assert np.array_equal(typed[1], bg) and typed[0].shape == (3, 4 ** k)
    host = engine.HostSeq()
    for begin in (host.seq_begin, host.seq_begin_typed):
        with pytest.raises(engine.KPError) as e:
            begin(4, 1)
        assert _code(e) == -1


SITES_FILE = """# CHROM POS REF ALT
chr1 4 T TGG
chr1 4 TAC T
chr1 5 AC -
chr1 7 - CC
chr1 9 GT CA
chr1 9 GTT CA
chr1 9 G C
chr1 9 G G
chr1 9 G GA,GAA
chr1 9 G <INS>
chr1 9 G GNA
chr1 4 A AGG
chr1 30 C CA
chr1 19 CAC C
chrX 2 A AT
chr2 2 CAAA CA
"""
CHR1 = "ACGTACGGGTAAAAAAACAC"
CHR2 = "GCAAAAAT"


def test_read_indels(tmp_path):
    path = tmp_path / "i.txt"
    path.write_text(SITES_FILE)
    sites, stats = seqio.read_indels(str(path))
    assert stats == {"lines": 16, "not_indel": 5, "complex": 2}
    s = sites["chr1"]
    assert s.pos.tolist() == [4, 4, 4, 6, 4, 30, 19]
    assert s.del_len.tolist() == [0, 2, 2, 0, 0, 0, 2]
    assert s.key.tolist() == [1, 2, 3, 4, 12, 13, 14]  # (0-based line numbers, the comment line counts)
    assert [bytes(s.ins[a:b]).decode() for a, b in zip(s.ins_off[:-1].tolist(), s.ins_off[1:].tolist())] == \
        ["GG", "", "", "CC", "GG", "A", ""]
    expect = [R.classify(*line.split()[2:4]) for line in SITES_FILE.splitlines()[1:]]
    assert sum(x == "not_indel" for x in expect) == 5 and sum(x == "complex" for x in expect) == 2
    kept, off, bad = seqio.match_indel_ref(np.frombuffer(CHR1.lower().encode(), np.uint8), s)
    assert (off, bad) == (2, 1) and kept.key.tolist() == [1, 2, 3, 4]
    assert kept.ins_off.tolist() == [0, 2, 2, 2, 4] and bytes(kept.ins) == b"GGCC"
    kept2, off, bad = seqio.match_indel_ref(np.frombuffer(CHR2.encode(), np.uint8), sites["chr2"])
    assert (off, bad) == (0, 0) and kept2.pos.tolist() == [3] and kept2.del_len.tolist() == [2]
    assert seqio.trim_alleles("CAAA", "CA") == (2, "AA", "") == R.trim("CAAA", "CA")
    with pytest.raises(ValueError):
        seqio.read_indels(__import__("io").StringIO("chr1 0 A AT\n"))


def _kmer_file(path):
    return {a: int(b) for a, b in (line.split() for line in open(path))}


def _counter(c):
    return {kmer: v for kmer, v in c.items() if v}


def test_command_line(tmp_path, capsys):
    fa = str(tmp_path / "g.fa")
    S.write_fasta(fa, [("chr1", CHR1), ("chr2", CHR2)])
    (tmp_path / "i.txt").write_text(SITES_FILE)
    # what the files must hold: the accepted sites by the reference
    chr1 = [("ins", 4, "GG", 1), ("del", 4, 2, 2), ("del", 4, 2, 3), ("ins", 6, "CC", 4)]
    chr2 = [("del", 3, 2, 16)]
    for how, extra in (("left", []), ("right", ["--place", "right"]), ("sample", ["--place", "sample", "--seed", "9"])):
        for strands in ("both", "forward"):
            c1 = R.count(CHR1, 4, chr1, strands == "both", how, 9, 0)
            c2 = R.count(CHR2, 4, chr2, strands == "both", how, 9, 1)
            for col in R.COLUMNS:
                out = str(tmp_path / "o.txt")
                argv = ["indel", fa, str(tmp_path / "i.txt"), col, "-k", "4", "--strands", strands, "-o", out,
                        "--resolved", str(tmp_path / "r.txt")] + extra
                assert C.main(argv, host=True) == 0
                assert _kmer_file(out) == _counter(c1[0][col] + c2[0][col])
                rows = [f"chr1 {lo} {hi} {p} {s[0]} {2}" for s, (lo, hi, p) in zip(chr1, c1[3])]
                rows += [f"chr2 {lo} {hi} {p} del 2" for lo, hi, p in c2[3]]
                assert open(tmp_path / "r.txt").read().splitlines() == rows
            err = capsys.readouterr().err
            for line in ("not_indel=5", "complex=2", "off_contig=2", "ref_mismatch=1", "unknown_contig=1", "ambiguous=2",
                         f"sites={c1[2]['sites'] + c2[2]['sites']}",
                         f"sites_skipped={c1[2]['sites_skipped'] + c2[2]['sites_skipped']}"):
                assert line in err.splitlines(), (line, err)
            bgp = str(tmp_path / "bg.txt")
            assert C.main(["background", fa, "-k", "4", "--strands", strands, "-o", bgp, "--verbosity", "0"], host=True) == 0
            assert _kmer_file(bgp) == _counter(c1[1] + c2[1])
    assert C.main(["indel", fa, str(tmp_path / "i.txt"), "ins", "--radius", "2", "-o", str(tmp_path / "o2.txt"),
                   "--verbosity", "0"], host=True) == 0
    both_left = R.count(CHR1, 4, chr1, True)[0]["ins"] + R.count(CHR2, 4, chr2, True)[0]["ins"]
    assert _kmer_file(str(tmp_path / "o2.txt")) == _counter(both_left)  # (the defaults: both strands, left)
    (tmp_path / "r.bed").write_text("chr1 2 9\nchr2 0 8\n")
    assert C.main(["background", fa, "-k", "3", "--strands", "both", "--bed", str(tmp_path / "r.bed"), "-o", bgp,
                   "--verbosity", "0"], host=True) == 0
    assert sum(_kmer_file(bgp).values()) == 2 * (7 + 6)
    # input errors exit 2
    base = ["indel", fa, str(tmp_path / "i.txt"), "ins", "-o", str(tmp_path / "e.txt")]
    for bad in (base + ["-k", "5"], base + ["-k", "16"], base + ["-k", "4", "--place", "sample"],
                ["indel", fa, str(tmp_path / "missing.txt"), "ins", "-k", "4"],
                ["background", fa, "-k", "16", "--strands", "both"]):
        assert C.main(bad, host=True) == 2
    assert "input error" in capsys.readouterr().err
    # the existing subcommands' defaults are what they were: folding, odd k
    assert C.main(["background", fa, "-k", "4", "-o", bgp], host=True) == 2
    assert C.main(["background", fa, "-k", "3", "-o", bgp, "--verbosity", "0"], host=True) == 0
    ref = S.count(3, True, [(CHR1, None, None), (CHR2, None, None)])[1]
    assert _kmer_file(bgp) == _counter(ref)
