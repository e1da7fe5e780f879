"""kmerpapa_amd.predict on the host session (engine.HostPred: the kernels' per-base and per-code
functions, serially) against the independent oracle of tests/pred_ref.py: per-region pattern
histograms, the expected counts bit for bit, the per-position track and the per-site codes, the
region batching and the command line.  No GPU."""
import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, predict
from kmerpapa_amd.papa import PatternPartition
from tests import pred_ref as R

# k, fold, general pattern, patterns
CASES = [(1, True, "M", 1), (1, True, "M", 2), (3, True, "NMN", 1), (3, True, "NMN", 2), (3, True, "NMN", 32),
         (5, True, "NNMNN", 37), (5, False, "NNCNN", 37), (5, True, "NNCNN", 2), (8, False, "NNNNNNNN", 37),
         (8, False, "NNNNSNNN", 1025), (9, True, "NNNNMNNNN", 1), (9, True, "NNNNMNNNN", 37), (9, True, "NNNNMNNNN", 1025),
         (9, True, "NNNWCGNNN", 37)]


def _contig(rng, n=900):
    seq = R.random_seq(rng, n, lower=0.25, invalid=0.004)
    seq[n // 3] = ord("N")
    seq[n // 3 + 40] = ord("n")
    return seq


def _regions(rng, n, k):
    """Unordered, overlapping, empty, one base long, at both ends, and past where windows fit."""
    fixed = [(0, n), (n - 1, n), (0, 1), (0, 0), (n, n), (n // 2, n // 2), (n - k, n), (0, k), (n // 3 - 2, n // 3 + 3),
             (n // 7, n // 2), (n // 6, n // 6 + 1), (n // 3, n // 3 + 50), (0, n)]
    b = rng.randint(0, n, size=20)
    rand = [(int(x), int(min(n, x + rng.randint(0, 200)))) for x in b]
    reg = np.array(fixed + rand)
    return reg[rng.permutation(reg.shape[0])]


def _words(names, gp):
    return [engine.pattern_word(x) for x in names], engine.pattern_word(gp)


@pytest.mark.parametrize("k,fold,gp,P", CASES, ids=[f"k{c[0]}_{c[2]}_P{c[3]}" for c in CASES])
def test_host_session_equals_the_oracle(k, fold, gp, P):
    rng = np.random.RandomState(7 * k + P)
    names = R.random_partition(rng, gp, P)
    rates = R.wide_rates(rng, P)
    seq = _contig(rng)
    n = seq.shape[0]
    reg = _regions(rng, n, k)
    words, sw = _words(names, gp)
    sites = [0, 1, n - 1, n // 3, n // 3 + k // 2, n // 3 - k // 2 - 1, 5, 5] + rng.randint(0, n, size=50).tolist()
    s = engine.HostPred()
    s.pred_begin(k, words, sw, fold)
    try:
        hist, other, exp = s.pred_regions(seq, reg, rates)
        no_hist = s.pred_regions(seq, reg, rates, want_hist=False)
        whole = s.pred_track(seq)
        part = s.pred_track(seq, 17, n - 5)
        at = s.pred_sites(seq, sites)
        st = s.pred_stats()
    finally:
        s.pred_end()
    ref_track = R.track(seq, names, fold)
    ref_hist, ref_other, ref_exp = R.regions(seq, names, fold, reg, rates)
    assert np.array_equal(hist, ref_hist) and np.array_equal(other, ref_other)
    assert exp.dtype == np.float64 and all(float(a) == float(b) for a, b in zip(exp, ref_exp))  # ==, not allclose
    assert no_hist[0] is None and np.array_equal(no_hist[1], other) and no_hist[2].tobytes() == exp.tobytes()
    assert (hist.sum(axis=1) + other.sum(axis=1)).tolist() == (reg[:, 1] - reg[:, 0]).tolist()
    assert np.array_equal(whole, ref_track) and np.array_equal(part, ref_track[17:n - 5])
    assert np.array_equal(at, ref_track[np.array(sites)])
    # -2 where the window runs off the contig and around the N; -1 only under a narrower super pattern
    assert (whole[:k // 2] == -2).all() and (whole[n - (k - 1 - k // 2):] == -2).all()
    lo, hi = n // 3 - (k - 1 - k // 2), n // 3 + k // 2
    assert (whole[max(lo, 0):hi + 1] == -2).all()
    covers_all = gp in ("M", "NMN", "NNMNN", "NNNNMNNNN", "NNNNNNNN")
    assert ((whole == -1).sum() == 0) == covers_all and (whole >= 0).sum() > 0
    assert int(other[:, 0].sum()) > 0 or covers_all
    assert st["unmatched"] == 2 * int(other[:, 0].sum()) and st["invalid"] == 2 * int(other[:, 1].sum())
    assert st["assigned"] == 2 * int(hist.sum()) and st["path"] == 0 and st["tile"] >= 256
    one = engine.pred_host(k, words, sw, fold, seq, reg, rates, (17, n - 5), sites)
    assert np.array_equal(one[0], hist) and np.array_equal(one[1], other) and one[2].tobytes() == exp.tobytes()
    assert np.array_equal(one[3], part) and np.array_equal(one[4], at) and one[5]["assigned"] == int(hist.sum())


def test_the_order_of_the_adds_matters():
    """The rates span twelve orders of magnitude: summing a row in another order rounds differently,
    so the equality above does pin the order."""
    rng = np.random.RandomState(5)
    names = R.random_partition(rng, "NNNNMNNNN", 1025)
    rates = R.wide_rates(rng, 1025)
    assert rates.max() / rates.min() > 1e10
    seq = R.random_seq(rng, 2_000)
    hist, _, exp = R.regions(seq, names, True, [(0, 2_000), (3, 900)], rates)
    assert any(float(np.sum((hist[r] * rates)[::-1])) != float(exp[r]) for r in range(2))


def test_whole_contig_histogram_equals_the_count_table():
    """One whole-contig region: hist[0] is what counting the contig and summing the table's
    background per pattern gives (count.count_table, PatternPartition.counts, both on the host)."""
    rng = np.random.RandomState(11)
    seq = R.random_seq(rng, 6000, lower=0.2, invalid=0.003)
    gp, k = "NNMNN", 5
    names = sorted(R.random_partition(rng, gp, 37))
    table = C.count_table([("c", seq)], k, sites={"c": rng.randint(0, 6000, size=300)}, host=True)
    counts = PatternPartition(list(names), superPattern=gp).counts(table, host=True)
    got = predict.region_counts([("c", seq)], names, {"c": [(0, 6000)]}, host=True)["c"]
    assert got[0][0].tolist() == [m + u for m, u in counts] and got[2] is None
    assert int(got[1][0, 0]) == 0 and int(got[0][0].sum() + got[1][0, 1]) == 6000


def _raises(code, call):
    with pytest.raises(engine.KPError) as e:
        call()
    assert e.value.code == code, str(e.value)
    return str(e.value)


def test_errors():
    word = engine.pattern_word
    s = engine.HostPred()
    nn = word("NN")
    msg = _raises(-1, lambda: s.pred_begin(3, [word("NCN"), word("ACN"), word("NMA")], word("NNN"), True))
    assert "patterns 0 and 1" in msg
    _raises(-1, lambda: s.pred_begin(0, [0], 0, False))
    _raises(-1, lambda: s.pred_begin(16, [word("N" * 16)], word("N" * 16), False))
    _raises(-1, lambda: s.pred_begin(2, [nn], nn, True))  # folding needs a centre
    _raises(-1, lambda: s.pred_begin(2, [], nn, False))
    _raises(-1, lambda: s.pred_begin(2, [word("N")], nn, False))  # an empty position
    seq = R.random_seq(np.random.RandomState(1), 50)
    for call in (lambda: s.pred_regions(seq, [(0, 5)]), lambda: s.pred_track(seq), lambda: s.pred_sites(seq, [1]),
                 lambda: s.pred_end(), lambda: s.pred_regions(seq, [(0, 5)])):
        _raises(-4, call)
    s.pred_begin(2, [nn], nn, False)
    try:
        _raises(-4, lambda: s.pred_begin(2, [nn], nn, False))
        _raises(-1, lambda: s.pred_sites(seq, [3, 50]))
        _raises(-1, lambda: s.pred_regions(seq, [(0, 51)]))
        _raises(-1, lambda: s.pred_regions(seq, [(7, 6)]))
        _raises(-1, lambda: s.pred_track(seq, 0, 51))
        _raises(-1, lambda: s.pred_track(seq, 9, 8))
        with pytest.raises(ValueError):
            s.pred_regions(seq, [(0, 5)], rates=[0.1, 0.2])
        assert s.pred_track(seq, 4, 4).shape == (0,) and s.pred_sites(seq, []).shape == (0,)
        hist, other, exp = s.pred_regions(seq, np.zeros((0, 2)), [0.5])
        assert hist.shape == (0, 1) and other.shape == (0, 2) and exp.shape == (0,)
    finally:
        s.pred_end()
    _raises(-4, lambda: s.pred_end())
    with pytest.raises(ValueError):
        predict.region_counts([], ["NMN", "NN"], {}, host=True)
    with pytest.raises(ValueError):
        predict.region_counts([("c", seq)], ["NN"], {"c": [(5, 3)]}, fold=False, host=True)


def test_many_patterns_are_checked_through_a_bitmap():
    """From 4,096 patterns on, the disjointness check marks k-mers in a bitmap instead of testing
    every pair; the pair it names is still the first one in (i, j) order."""
    rng = np.random.RandomState(29)
    gp = "NNNNNNN"
    names = R.random_partition(rng, gp, 4200)
    words, sw = _words(names, gp)
    seq = _contig(rng, 400)
    s = engine.HostPred()
    s.pred_begin(7, words, sw, False)
    try:
        assert np.array_equal(s.pred_track(seq), R.track(seq, names, False))
    finally:
        s.pred_end()
    twice = list(words)
    twice[4100] = words[17]  # the same k-mers twice, as many k-mers as before or fewer
    assert "patterns 17 and 4100" in _raises(-1, lambda: s.pred_begin(7, twice, sw, False))
    wide = list(words)
    wide[5], wide[4199] = sw, words[5]  # more k-mers than there are
    msg = _raises(-1, lambda: s.pred_begin(7, wide, sw, False))
    first = min(i for i in range(4200) if i != 5)
    assert f"patterns {min(first, 5)} and {max(first, 5)}" in msg
    gap = words[:2000] + words[2001:]  # a k-mer in no pattern is fine
    s.pred_begin(7, gap, sw, False)
    try:
        assert (s.pred_track(seq) == -1).sum() == (R.track(seq, names, False) == 2000).sum()
    finally:
        s.pred_end()


def test_region_batching_changes_nothing():
    rng = np.random.RandomState(13)
    contigs = [("a", _contig(rng, 700)), ("b", _contig(rng, 300)), ("unused", _contig(rng, 100))]
    names = R.random_partition(rng, "NNMNN", 37)
    rates = R.wide_rates(rng, 37)
    regions = {"a": _regions(rng, 700, 5), "b": _regions(rng, 300, 5), "missing": [(0, 5)]}
    ref = predict.region_counts(contigs, names, regions, rates, host=True)
    assert sorted(ref) == ["a", "b"]
    for budget in (1, 37, 38, 5 * 37 + 1, 10 ** 6):
        got = predict.region_counts(contigs, names, regions, rates, host=True, budget=budget)
        for name in ref:
            assert all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(got[name], ref[name]))
    for name, seq in contigs[:2]:
        h, o, e = R.regions(seq, names, True, regions[name], rates)
        assert np.array_equal(ref[name][0], h) and np.array_equal(ref[name][1], o) and ref[name][2].tobytes() == e.tobytes()
    no = predict.region_counts(contigs, names, regions, host=True, want_hist=False)
    assert no["a"][0] is None and no["a"][2] is None and np.array_equal(no["a"][1], ref["a"][1])


def test_track_rates_and_sites_functions():
    rng = np.random.RandomState(19)
    contigs = [("a", _contig(rng, 500)), ("b", _contig(rng, 200))]
    names = R.random_partition(rng, "NNCNN", 5)
    rates = R.wide_rates(rng, 5)
    one = predict.track(contigs[0][1], names, fold=False, host=True)
    assert np.array_equal(one, R.track(contigs[0][1], names, False))
    assert np.array_equal(predict.track(contigs[0][1], names, fold=False, host=True, begin=20, end=99), one[20:99])
    both = predict.track(contigs, names, fold=False, host=True)
    assert np.array_equal(both["a"], one) and np.array_equal(both["b"], R.track(contigs[1][1], names, False))
    r = predict.rates_of(one, rates)
    assert np.isnan(r[one < 0]).all() and (one < 0).any() and np.array_equal(r[one >= 0], rates[one[one >= 0]])
    sites = {"a": [5, 5, 499, 250], "b": [0], "c": [1]}
    got = predict.site_patterns(contigs, names, sites, fold=False, host=True)
    assert sorted(got) == ["a", "b"] and np.array_equal(got["a"], one[[5, 5, 499, 250]]) and got["b"].tolist() == [-2]


def _write_partition(path, names, rates, long_format=False):
    with open(path, "w") as f:
        if long_format:
            f.write("context c_neg c_pos c_rate pattern p_neg p_pos p_rate\n")
            for x, r in zip(names, rates):  # two k-mer rows per pattern
                f.write(f"{'A' * len(x)} 1 1 0.5 {x} 10 1 {float(r)!r}\n{'C' * len(x)} 1 1 0.5 {x} 10 1 {float(r)!r}\n")
        else:
            f.write("pattern p_neg p_pos p_rate\n" + "".join(f"{x} 10 1 {float(r)!r}\n" for x, r in zip(names, rates)))


@pytest.mark.parametrize("fmt", ["fasta", "2bit"])
def test_command_line(tmp_path, capsys, fmt):
    rng = np.random.RandomState(23)
    contigs = [("chr1", R.random_seq(rng, 1200, invalid=0.004)), ("chr2", R.random_seq(rng, 400))]
    # (both formats spell an invalid byte N and, the .2bit reader dropping the masks, upper case)
    contigs = [(n, np.where(np.isin(s, list(b"ACGT")), s, ord("N")).astype(np.uint8)) for n, s in contigs]
    genome = str(tmp_path / ("g.fa" if fmt == "fasta" else "g.2bit"))
    (R.write_fasta if fmt == "fasta" else R.write_2bit)(genome, contigs)
    seqs = {n: R.text(s) for n, s in contigs}
    names = R.random_partition(rng, "NNCNN", 9)
    rates = [float(x) for x in R.wide_rates(rng, 9)]
    _write_partition(tmp_path / "p.txt", names, rates, long_format=fmt == "2bit")
    base = ["--partition", str(tmp_path / "p.txt"), "--verbosity", "0"]

    bed = [("chr2", 0, 400, "whole"), ("chr1", 100, 900, None), ("chrX", 5, 9, "nowhere"), ("chr1", 0, 1, "edge"),
           ("chr1", 850, 1200, "late"), ("chr2", 7, 7, "empty")]
    with open(tmp_path / "r.bed", "w") as f:
        f.write("# regions\ntrack name=x\n" + "".join(f"{c}\t{b}\t{e}" + (f"\t{x}\t0\t+" if x else "") + "\n" for c, b, e, x in bed))
    want = []
    for c, b, e, x in bed:
        head = f"{c} {b} {e}" + (f" {x}" if x else "")
        if c not in seqs:
            want.append(f"{head} 0 0 0 0.0\n")
            continue
        h, o, ex = R.regions(seqs[c], names, True, [(b, e)], rates)
        want.append(f"{head} {int(h.sum())} {int(o[0, 0])} {int(o[0, 1])} {float(ex[0])!r}\n")
    out = str(tmp_path / "regions.txt")
    assert predict.main(["regions", genome, "--bed", str(tmp_path / "r.bed"), "-o", out] + base, host=True) == 0
    assert open(out).read() == "".join(want)

    def bedgraph(name, b, e, fold):
        pid = R.track(seqs[name], names, fold, b, e).tolist()
        lines, start = [], 0
        for i in range(1, len(pid) + 1):
            if i == len(pid) or pid[i] != pid[start]:
                if pid[start] >= 0:
                    lines.append(f"{name} {b + start} {b + i} {rates[pid[start]]!r}\n")
                start = i
        return "".join(lines)

    assert predict.main(["track", genome, "-o", out, "--no-fold"] + base, host=True) == 0
    assert open(out).read() == bedgraph("chr1", 0, 1200, False) + bedgraph("chr2", 0, 400, False)
    # with regions: merged per contig (seqio.read_bed), in the genome's contig order
    assert predict.main(["track", genome, "--bed", str(tmp_path / "r.bed"), "-o", out] + base, host=True) == 0
    assert open(out).read() == bedgraph("chr1", 0, 1, True) + bedgraph("chr1", 100, 1200, True) + bedgraph("chr2", 0, 400, True)

    sites = []
    for c, p in [("chr2", 5), ("chr1", 700), ("chr1", 700), ("chr1", 1), ("chr1", 1200), ("chr1", 1201), ("chrX", 3), ("chr2", 399)] \
            + [("chr1", int(x)) for x in rng.randint(1, 1201, size=40)]:
        ref = seqs[c][p - 1] if c in seqs and p <= len(seqs[c]) and seqs[c][p - 1] in "ACGT" else "A"
        sites.append((c, p, ref, "ACGT"[("ACGT".index(ref) + 1) % 4]))
    sites.append(("chr2", 11, "ACGT"[("ACGT".index(seqs["chr2"][10]) + 2) % 4], seqs["chr2"][10]))  # a REF mismatch
    with open(tmp_path / "m.txt", "w") as f:
        f.write("#CHROM POS REF ALT\n" + "".join(f"{c}\t{p}\t{r.lower()}\t{a}\n" for c, p, r, a in sites) + "chr1 5 AC A\n")
    want = []
    for c, p, r, a in sites:
        j = -2
        if c in seqs and p <= len(seqs[c]) and seqs[c][p - 1] == r:
            j = R.pid_at(seqs[c], p - 1, names, True)
        want.append(f"{c} {p} {r.lower()} {a} " + (f"{names[j]} {rates[j]!r}\n" if j >= 0 else "NA NA\n"))
    capsys.readouterr()
    assert predict.main(["sites", genome, str(tmp_path / "m.txt"), "-o", out, "--partition", str(tmp_path / "p.txt")], host=True) == 0
    assert open(out).read() == "".join(want)
    err = capsys.readouterr().err
    bad_ref = sum(1 for c, p, r, _ in sites if c in seqs and p <= len(seqs[c]) and seqs[c][p - 1] != r)
    assert bad_ref >= 1
    for line in ("not_snv=1", "off_contig=1", f"ref_mismatch={bad_ref}", "unknown_contig=1"):
        assert line in err.splitlines(), err
    assert any(x.endswith("NA NA\n") for x in want) and any(not x.endswith("NA NA\n") for x in want)


def test_command_line_errors(tmp_path, capsys):
    rng = np.random.RandomState(3)
    R.write_fasta(str(tmp_path / "g.fa"), [("c", R.random_seq(rng, 100))])
    with open(tmp_path / "r.bed", "w") as f:
        f.write("c 0 50\n")
    genome, bed = str(tmp_path / "g.fa"), str(tmp_path / "r.bed")

    def run(names, *extra, bed_file=bed):
        _write_partition(tmp_path / "p.txt", names, [0.1] * len(names))
        rc = predict.main(["regions", genome, "--bed", bed_file, "--partition", str(tmp_path / "p.txt")] + list(extra), host=True)
        return rc, capsys.readouterr()

    rc, io = run(["NCN", "ACN", "NAN", "NAA"])
    assert rc == 1 and io.out == ""
    assert io.err.strip() == "kmerpapa-predict: the patterns are not a partition: 2 pairs of patterns share k-mers"
    rc, io = run(["NN"])
    assert rc == 2 and io.err.startswith("kmerpapa-predict: input error: ") and "--no-fold" in io.err
    assert run(["NN"], "--no-fold")[0] == 0
    assert run(["NCN", "NA"])[0] == 2
    with open(tmp_path / "bad.bed", "w") as f:
        f.write("c 0 101\n")
    rc, io = run(["NMN"], bed_file=str(tmp_path / "bad.bed"))
    assert rc == 2 and io.err.startswith("kmerpapa-predict: input error: ") and io.out == ""
    with open(tmp_path / "bad.bed", "w") as f:
        f.write("c 9 x\n")
    assert run(["NMN"], bed_file=str(tmp_path / "bad.bed"))[0] == 2
    assert run(["NMN"], bed_file=str(tmp_path / "none.bed"))[0] == 2
    with open(tmp_path / "p.txt", "w") as f:
        f.write("not a table\n")
    assert predict.main(["track", genome, "--partition", str(tmp_path / "p.txt")], host=True) == 2
    rc, io = run(["NMN"])
    assert rc == 0 and io.out == "c 0 50 49 0 1 4.9\n" and "assigned=49" in io.err
