"""k-mer context counts of sequences on the host (engine.seq_host / kp_seq_host: the kernels'
per-base code run serially; kmerpapa_amd.count with host=True; the readers of
kmerpapa_amd.seqio) against the independent oracle of tests/seq_ref.py.  Bar: both count
columns and every count stat equal."""
import io
import os
import sys
from argparse import Namespace

import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, seqio
from kmerpapa_amd.io_utils import read_input_table
from tests import seq_ref as R

KS = [(1, False), (2, False), (3, True), (3, False), (5, True), (7, True), (9, True), (11, True), (4, False)]


def _same(got, ref, k):
    pos, bg, st = got
    rpos, rbg, rst = ref
    assert np.array_equal(pos, R.dense(rpos, k)) and np.array_equal(bg, R.dense(rbg, k))
    assert {key: st[key] for key in R.COUNT_STATS} == rst


def _check(k, fold, jobs):
    jobs = list(jobs)
    got = engine.seq_host(k, fold, jobs)
    _same(got, R.count(k, fold, jobs), k)
    return got


def _with_n_runs(rng, n, k):
    """Mixed-case bases with N runs of lengths 1, k - 1, k and longer, well apart."""
    seq = R.random_seq(rng, n, lower=0.3)
    at = 40
    for length in (1, max(k - 1, 1), k, k + 1, 3 * k + 5):
        seq[at:at + length] = ord("N") if length % 2 else ord("n")
        at += length + 2 * k + 7
    return seq


@pytest.mark.parametrize("k,fold", KS)
def test_scan_against_oracle(k, fold):
    rng = np.random.RandomState(100 + k)
    seq = _with_n_runs(rng, 3000, k)
    pos, bg, st = _check(k, fold, [(seq, None, None)])
    assert int(bg.sum()) == st["windows"] > 2000 and st["windows_invalid"] > 0 and not pos.any()
    assert st["path"] == 0 and st["scan_ms"] == 0.0
    # the one-call form of the same session
    one = engine.seq_host_contig(k, fold, seq)
    assert np.array_equal(one[1], bg) and {x: one[2][x] for x in R.COUNT_STATS} == {x: st[x] for x in R.COUNT_STATS}


@pytest.mark.parametrize("k,fold", KS)
def test_invalid_bytes_at_the_ends_and_scattered(k, fold):
    rng = np.random.RandomState(200 + k)
    seq = R.random_seq(rng, 2500, lower=0.5, invalid=0.02)
    seq[0] = ord("N")
    seq[-1] = ord("-")
    _check(k, fold, [(seq, None, None)])
    seq[0] = ord("a")
    seq[-1] = ord("t")
    _check(k, fold, [(seq, None, None)])


@pytest.mark.parametrize("k,fold", KS)
def test_tiny_contigs(k, fold):
    rng = np.random.RandomState(300 + k)
    for n in (0, k - 1, k, k + 1):
        pos, bg, st = _check(k, fold, [(R.random_seq(rng, n), None, None)])
        assert st["windows"] == max(0, n - k + 1) == int(bg.sum())
    # several contigs in one session: no window spans two of them
    parts = [R.random_seq(rng, n) for n in (k, 57, 0, k - 1, 300)]
    pos, bg, st = _check(k, fold, [(p, None, None) for p in parts])
    assert st["windows"] == sum(max(0, p.shape[0] - k + 1) for p in parts)


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_fold_identities(k):
    rng = np.random.RandomState(400 + k)
    seq = _with_n_runs(rng, 4000, k)
    _, raw, st_raw = engine.seq_host(k, False, [(seq, None, None)])
    _, folded, st = engine.seq_host(k, True, [(seq, None, None)])
    codes = np.arange(4 ** k)
    rc = np.zeros_like(codes)
    for i in range(k):  # letter k - 1 - i of the reverse complement = complement of letter i
        rc += (3 - ((codes >> (2 * (k - 1 - i))) & 3)) << (2 * i)
    some = np.random.RandomState(k).randint(0, 4 ** k, size=50)
    assert [R.kmer_of(int(rc[c]), k) for c in some] == [R.revcomp(R.kmer_of(int(c), k)) for c in some]
    centre = (codes >> (2 * (k - 1 - k // 2))) & 3
    assert not folded[centre >= 2].any()
    assert int(folded.sum()) == int(raw.sum()) == st["windows"] == st_raw["windows"]
    keep = centre < 2
    assert np.array_equal(folded[keep], raw[keep] + raw[rc[keep]])


REGION_SETS = {
    "overlapping_and_adjacent": [(100, 200), (150, 260), (260, 300), (900, 950), (1000, 1000)],
    "ends_of_the_contig": [(0, 30), (1970, 2000)],
    "one_base_regions": [(0, 1), (5, 6), (1999, 2000), (700, 701)],
    "empty_only": [(50, 50)],
    "whole": [(0, 2000)],
}


@pytest.mark.parametrize("name", sorted(REGION_SETS))
@pytest.mark.parametrize("k,fold", [(1, False), (4, False), (5, True), (9, True)])
def test_regions(name, k, fold):
    rng = np.random.RandomState(len(name) + k)
    seq = R.random_seq(rng, 2000, lower=0.2, invalid=0.01)
    raw = REGION_SETS[name]
    merged = seqio.merge_regions(raw)
    assert all(merged[i, 1] < merged[i + 1, 0] for i in range(merged.shape[0] - 1))
    got = engine.seq_host(k, fold, [(seq, merged, None)] if merged.shape[0] else [])
    _same(got, R.count(k, fold, [(seq, raw, None)]), k)
    # count_genome merges for itself
    got = C.count_genome([("c", seq)], k, fold, regions={"c": raw, "other": [(0, 5)]}, host=True)
    _same(got, R.count(k, fold, [(seq, raw, None)]), k)
    if name == "whole":
        assert np.array_equal(got[1], engine.seq_host(k, fold, [(seq, None, None)])[1])


def test_merge_regions():
    assert seqio.merge_regions([(5, 9), (1, 3), (3, 4), (8, 12), (20, 20), (30, 31)]).tolist() == [[1, 4], [5, 12], [30, 31]]
    assert seqio.merge_regions([(0, 100), (10, 20), (30, 40), (100, 101)]).tolist() == [[0, 101]]
    assert seqio.merge_regions([]).shape == (0, 2)
    with pytest.raises(ValueError):
        seqio.merge_regions([(5, 4)])


@pytest.mark.parametrize("k,fold", [(1, False), (2, False), (3, True), (5, True), (9, True), (11, False)])
def test_sites(k, fold):
    rng = np.random.RandomState(500 + k)
    n = 1500
    seq = R.random_seq(rng, n, lower=0.3)
    seq[700] = ord("N")
    sites = [0, n - 1, 699, 701, 700, 700 - k // 2 - 1, 700 + k // 2 + 1, k // 2, n - 1 - (k - 1 - k // 2), 33, 33, 33, 900, 33]
    sites += rng.randint(0, n, size=300).tolist()
    pos, bg, st = _check(k, fold, [(seq, False, sites)])
    assert st["sites"] + st["sites_skipped"] == len(sites) and int(pos.sum()) == st["sites"] and not bg.any()
    assert st["sites_skipped"] >= (3 if k > 1 else 1)
    # scan and sites of two contigs in one session
    other = R.random_seq(rng, 400, invalid=0.05)
    _check(k, fold, [(seq, None, sites), (other, [(10, 390)], [5, 5, 399, 200])])
    one = engine.seq_host_contig(k, fold, seq, False, sites)
    assert np.array_equal(one[0], pos) and one[2]["sites_skipped"] == st["sites_skipped"]


def test_errors():
    h = engine.HostSeq()
    seq = R.random_seq(np.random.RandomState(1), 100)
    for k, fold in ((0, False), (16, False), (-1, False), (2, True), (14, True)):
        with pytest.raises(engine.KPError) as e:
            h.seq_begin(k, fold)
        assert e.value.code == -1, (k, fold)
    for call in (lambda: h.seq_scan(seq), lambda: h.seq_sites(seq, [1]), lambda: h.seq_end()):
        with pytest.raises(engine.KPError) as e:
            call()
        assert e.value.code == -4  # KP_E_STATE: nothing is open
    h.seq_begin(3, True)
    with pytest.raises(engine.KPError) as e:
        h.seq_begin(3, True)
    assert e.value.code == -4
    for bad in ([(10, 20), (5, 8)], [(10, 20), (19, 30)], [(90, 101)], [(30, 20)]):
        with pytest.raises(engine.KPError) as e:
            h.seq_scan(seq, np.array(bad))
        assert e.value.code == -1, bad
    with pytest.raises(engine.KPError) as e:
        h.seq_sites(seq, [5, 100])
    assert e.value.code == -1
    h.seq_scan(seq, np.array([(10, 20), (20, 20), (20, 30)]))  # adjacent and empty are fine
    pos, bg = h.seq_end()
    assert int(bg.sum()) == 20 and h.seq_stats()["windows"] == 20
    with pytest.raises(engine.KPError) as e:
        h.seq_end()
    assert e.value.code == -4
    with pytest.raises(engine.KPError) as e:
        engine.seq_host_contig(4, True, seq)
    assert e.value.code == -1
    assert engine.seq_host_contig(4, False, seq)[2]["windows"] == 97  # the failed call left no session open


def _genome(rng):
    a = _with_n_runs(rng, 1203, 5)
    b = R.random_seq(rng, 77, lower=0.5)
    b[:9] = ord("N")
    b[-2:] = ord("n")
    return [("chr1", a), ("chrB", b), ("empty", np.zeros(0, np.uint8)), ("chr3", R.random_seq(rng, 401))]


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_fasta_and_2bit_round_trip(tmp_path, newline):
    contigs = _genome(np.random.RandomState(9))
    fa = str(tmp_path / "g.fa")
    R.write_fasta(fa, contigs, width=61, newline=newline)
    got = list(seqio.read_fasta(fa))
    assert [n for n, _ in got] == [n for n, _ in contigs]
    assert all(np.array_equal(x[1], y[1]) and x[1].dtype == np.uint8 for x, y in zip(got, contigs))  # case kept
    upper = [(n, np.where((s | 0x20) == ord("n"), ord("N"), s & 0xDF).astype(np.uint8)) for n, s in contigs]
    for order in "<>":
        tb = str(tmp_path / f"g{ord(order)}.2bit")
        R.write_2bit(tb, contigs, order)
        assert seqio.is_2bit(tb) and not seqio.is_2bit(fa)
        got = list(seqio.read_genome(tb))
        assert [n for n, _ in got] == [n for n, _ in upper]
        assert all(np.array_equal(x[1], y[1]) for x, y in zip(got, upper))
        # the counts do not depend on the container or on case
        assert np.array_equal(C.count_genome(seqio.read_genome(tb), 5, host=True)[1],
                              C.count_genome(seqio.read_genome(fa), 5, host=True)[1])
    one_line = str(tmp_path / "one.fa")
    R.write_fasta(one_line, contigs[:2], width=10 ** 6)
    assert np.array_equal(list(seqio.read_fasta(one_line))[0][1], contigs[0][1])
    with pytest.raises(ValueError):
        list(seqio.read_fasta(io.BytesIO(b"ACGT\n>x\nAC\n")))


def _sites_text(contigs, rng):
    """(text, expected 0-based kept sites per contig for type None)."""
    a = R.text(contigs[0][1]).upper()
    lines = ["#CHROM POS REF ALT"]
    # (distinct positions: each is also a background window, so no k-mer has positive > background)
    for p in [1, 2, len(a)] + (rng.choice(len(a) - 3, size=200, replace=False) + 3).tolist():
        ref = a[p - 1]
        if ref in "ACGT":
            alt = "ACGT"[("ACGT".index(ref) + 1 + p % 3) % 4]
            lines.append(f"chr1\t{p}\t{ref.lower() if p % 5 == 0 else ref}\t{alt}")
    ok = "C" if a[699] != "C" else "A"
    lines += [f"chr1 700 {ok} T",              # REF mismatch
              "chr1 300 AC A", "chr1 301 A AT", "chr1 302 N A", "chr1 303 A A",  # no SNVs
              f"chr1 {len(a) + 5} A C",        # past the contig
              "chrZ 5 A C",                    # unknown contig
              f"chr3 7 {R.text(contigs[3][1])[6].upper()} {'A' if R.text(contigs[3][1])[6].upper() != 'A' else 'C'} extra columns"]
    return "\n".join(lines) + "\n"


def test_sites_reader(tmp_path):
    rng = np.random.RandomState(4)
    contigs = _genome(rng)
    text = _sites_text(contigs, rng)
    raw, st = seqio.read_sites(io.BytesIO(text.encode()))
    assert st["not_snv"] == 4 and st["other_type"] == 0 and st["lines"] == text.count("\n") - 1
    pos, off, bad = seqio.match_ref(contigs[0][1], *raw["chr1"])
    assert (off, bad) == (1, 1) and pos.shape[0] == raw["chr1"][0].shape[0] - 2
    assert raw["chr3"][0].tolist() == [6] and "chrZ" in raw
    # --type: G>A sites fold to C>T
    a = R.text(contigs[0][1]).upper()
    only, st2 = seqio.read_sites(io.BytesIO(text.encode()), seqio.parse_type("C>T"))
    want = [int(t[1]) - 1 for t in (ln.split() for ln in text.splitlines()[1:])
            if len(t[2]) == 1 and len(t[3]) == 1 and (t[2].upper(), t[3].upper()) in (("C", "T"), ("G", "A"))]
    assert sorted(x for v in only.values() for x in v[0].tolist()) == sorted(want)
    assert any(a[p] == "G" for p in only["chr1"][0].tolist() if p < len(a))  # one matches only after folding
    assert seqio.parse_type("g>a") == "C>T" and seqio.fold_type("T", "C") == "A>G"
    assert st2["other_type"] + sum(len(v[0]) for v in only.values()) + st2["not_snv"] == st2["lines"]
    with pytest.raises(ValueError):
        seqio.parse_type("C>C")
    with pytest.raises(ValueError):
        seqio.read_sites(io.BytesIO(b"chr1 0 A C\n"))
    # extra columns are ignored, never read as REF or ALT: an indel with a fifth column is no site
    extra, st3 = seqio.read_sites(io.BytesIO(b"##x\n#CHROM\tPOS\tREF\tALT\nchr1\t9\tA\tG\t.\t.\nchr1 301 AT A G\nchr1 5 rs1 A G\n"))
    assert extra["chr1"][0].tolist() == [8] and extra["chr1"][1].tolist() == [ord("A")] and st3["not_snv"] == 2


def test_bed_reader():
    bed = b"track name=x\n#c\nchr1\t10\t20\tname\t0\t+\nchr1 15 30\nchr2 0 5\nchr1 30 31\n\nchr2 9 9\n"
    got = seqio.read_bed(io.BytesIO(bed))
    assert got["chr1"].tolist() == [[10, 31]] and got["chr2"].tolist() == [[0, 5]]
    with pytest.raises(ValueError):
        seqio.read_bed(io.BytesIO(b"chr1 10\n"))
    with pytest.raises(ValueError):
        seqio.read_bed(io.BytesIO(b"chr1 a b\n"))


def test_count_table_rules():
    rng = np.random.RandomState(12)
    contigs = _genome(rng)
    sites = {"chr1": rng.randint(0, 1203, size=150), "chr3": [3, 3, 200]}
    pos, bg, st = C.count_genome(contigs, 5, sites=sites, host=True)
    t = C.count_table(contigs, 5, sites=sites, host=True)
    keep = np.flatnonzero(bg)
    assert np.array_equal(t.codes, keep) and np.array_equal(t.M, pos[keep]) and np.array_equal(t.U, bg[keep] - pos[keep])
    assert t.k == 5 and (t.U >= 0).all() and int(t.M.sum()) == st["sites"]
    with pytest.raises(ValueError, match="Problematic k-mer"):  # a site counted five times, background once
        C.count_table(contigs, 5, regions={"chr3": [(200, 201)]}, sites={"chr3": [200] * 5}, host=True)
    # the table goes straight into the host paths of kp_greedy and kp_apply
    from kmerpapa_amd.apply import apply_partition
    full = t.zero_filled("NNMNN")
    pid, pM, pU, _, stq = apply_partition(["NNANN", "NNCNN"], full, host=True)
    assert stq["unmatched"] == 0 and int(pM.sum()) == int(t.M.sum()) and int(pU.sum()) == int(t.U.sum())


def test_command_line_end_to_end(tmp_path, capsys):
    rng = np.random.RandomState(21)
    contigs = _genome(rng)
    tb, fa = str(tmp_path / "g.2bit"), str(tmp_path / "g.fa")
    R.write_2bit(tb, contigs)
    R.write_fasta(fa, contigs)
    sites_file, bed_file = str(tmp_path / "m.txt"), str(tmp_path / "r.bed")
    with open(sites_file, "w") as f:
        f.write(_sites_text(contigs, rng))
    with open(bed_file, "w") as f:
        f.write("chr1 0 500\nchr1 400 1203\nchr3\t0\t401\tx\nchrB 0 77\nchrQ 1 5\nchrQ 9 12\n")
    bg_out, pos_out = str(tmp_path / "bg.txt"), str(tmp_path / "pos.txt")
    assert C.main(["background", tb, "--radius", "2", "--bed", bed_file, "-o", bg_out], host=True) == 0
    assert C.main(["snv", fa, sites_file, "-k", "5", "-o", pos_out, "--verbosity", "1"], host=True) == 0
    err = capsys.readouterr().err
    assert "ref_mismatch=1" in err and "not_snv=4" in err and "unknown_contig=1" in err and "off_contig=1" in err
    assert "unknown_contig_regions=2" in err  # the BED's chrQ is not in the genome
    lines = open(bg_out).read().splitlines()
    assert lines == sorted(lines) and all(len(x.split()[0]) == 5 and x.split()[0][2] in "AC" and int(x.split()[1]) > 0
                                          for x in lines)
    raw, _ = seqio.read_sites(sites_file)
    sites = {name: seqio.match_ref(seq, *raw[name])[0] for name, seq in contigs if name in raw}
    want = C.count_table(contigs, 5, sites=sites, host=True)
    args = Namespace(positive=open(pos_out), background=open(bg_out), negative=None, joint_context_counts=None)
    table, n_neg, n_pos = read_input_table(args, None)
    assert table.k == 5 and np.array_equal(table.codes, want.codes)
    assert np.array_equal(table.M, want.M) and np.array_equal(table.U, want.U)
    assert n_pos == int(want.M.sum()) and n_neg == int(want.U.sum())
    # --type, --no-fold and the whole genome without a BED file
    assert C.main(["snv", tb, sites_file, "--radius", "1", "--type", "G>A", "--verbosity", "0", "-o", pos_out], host=True) == 0
    only, _ = seqio.read_sites(sites_file, "C>T")
    n_ct = sum(seqio.match_ref(seq, *only[name])[0].shape[0] for name, seq in contigs if name in only)
    got = [x.split() for x in open(pos_out).read().splitlines()]
    assert 0 < sum(int(c) for _, c in got) <= n_ct and all(kmer[1] == "C" for kmer, _ in got)
    assert C.main(["background", fa, "-k", "4", "--no-fold", "--verbosity", "0", "-o", bg_out], host=True) == 0
    assert sum(int(x.split()[1]) for x in open(bg_out)) == R.count(4, False, [(s, None, None) for _, s in contigs])[2]["windows"]
    # input errors: exit code 2
    for argv in (["background", fa, "-k", "4"], ["background", fa, "-k", "16", "--no-fold"],
                 ["background", str(tmp_path / "missing.fa"), "-k", "3"], ["snv", fa, sites_file, "-k", "3", "--type", "CT"],
                 ["background", fa, "-k", "3", "--bed", sites_file]):
        assert C.main(argv + ["-o", str(tmp_path / "x")], host=True) == 2, argv
        assert not os.path.exists(tmp_path / "x")  # the output is opened only after the counting succeeded
    assert C.main(["background", fa, "-k", "3", "-o", str(tmp_path / "no_dir" / "x")], host=True) == 2
    assert "input error" in capsys.readouterr().err


def test_module_entry_point(tmp_path):
    """`python -m kmerpapa_amd.count` exists and reports input errors with exit code 2 before
    it touches a GPU."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "kmerpapa_amd.count", "background", str(tmp_path / "none.fa"), "-k", "3"],
                       cwd=root, capture_output=True, text=True)
    assert r.returncode == 2 and "input error" in r.stderr
