"""Coding consequences on the host session (engine.HostSpec: the kernels' per-pair functions run
serially) against the independent oracle of tests/coding_ref.py, the readers of transcripts and both
subcommands.  Every comparison is for equality, integers and float64 bits alike.  No GPU."""
import io

import numpy as np
import pytest

from kmerpapa_amd import engine, seqio, spectrum
from tests import coding_cases as K
from tests import coding_ref as C
from tests import spec_ref as R


def _against_oracle(k, fold, jobs):
    names, words, ptype, rates = K.model(k, fold)
    s = engine.HostSpec()
    s.spec_begin(k, words, ptype, fold)
    try:
        for seq, txs, splice in jobs:
            got = K.run(s, seq, txs, splice, rates)
            K.same(got, K.oracle(seq, names, ptype, fold, txs, splice, rates), counts=False)
            K.check_identities(got, txs, splice)
            positions = sum(e - b for _, segs in txs for b, e in segs) + sum(
                len(C.splice_positions([(int(b), int(e)) for b, e in segs], splice)) for _, segs in txs)
            assert got["counts"][1] == positions
    finally:
        s.spec_end()


def test_class_table_every_codon_position_and_alt_on_both_strands():
    seq, txs = K.table_case()
    _against_oracle(3, True, [(seq, txs, 2)])
    # ... and the classes themselves, once, against a few known ones
    names, words, ptype, rates = K.model(3, True)
    s = engine.HostSpec()
    s.spec_begin(3, words, ptype, True)
    try:
        pos, alts, tx = C.all_pairs(seq, txs, 2)
        assert pos.shape[0] == 2 * 64 * 3 * 3
        cls, _, codons = s.spec_coding_sites(seq, txs, pos, alts, tx, 2)
    finally:
        s.spec_end()
    by = {(int(p), chr(a), int(t)): (int(c), int(x)) for p, a, t, c, x in zip(pos, alts, tx, cls, codons)}
    tgg = 3 * C.codon_index("TGG")  # Trp: TGG > TGA and TAG are stops, TGG > TGT is Cys
    assert by[(tgg + 2, "A", 0)][0] == 2 and by[(tgg + 1, "A", 0)][0] == 2 and by[(tgg + 2, "T", 0)][0] == 1
    taa = 3 * C.codon_index("TAA")  # stop: TAA > TAG stays a stop, TAA > CAA is Gln
    assert by[(taa + 2, "G", 0)][0] == 0 and by[(taa, "C", 0)][0] == 3
    assert by[(taa, "C", 0)][1] == C.codon_index("TAA") | C.codon_index("CAA") << 6
    cca = 3 * C.codon_index("CCA")  # on the - strand CCA reads TGG: C > T at its first base is TGG > TGA
    assert by[(cca, "T", 1)] == (2, C.codon_index("TGG") | C.codon_index("TGA") << 6)
    assert sorted(set(cls.tolist())) == [0, 1, 2, 3]


@pytest.mark.parametrize("k,fold", K.KSETS)
@pytest.mark.parametrize("lengths", K.SPLIT_LENGTHS, ids=lambda x: "".join(map(str, x)))
def test_segment_splits_introns_and_splice_widths(lengths, k, fold):
    """Codons that span two and three segments, introns shorter than twice the splice width and
    abutting segments."""
    jobs = [K.split_case(lengths, intron) + (splice,) for intron in K.INTRONS + [0] for splice in K.SPLICES]
    _against_oracle(k, fold, jobs)


@pytest.mark.parametrize("k,fold", K.KSETS)
@pytest.mark.parametrize("case", ["invalid", "ends", "overlap"])
def test_invalid_bytes_contig_ends_and_overlap(case, k, fold):
    seq, txs = {"invalid": K.invalid_case, "ends": K.ends_case, "overlap": K.overlap_case}[case]()
    _against_oracle(k, fold, [(seq, txs, splice) for splice in K.SPLICES])


def test_invalid_bytes_land_where_the_definitions_say():
    seq, txs = K.invalid_case()
    names, words, ptype, rates = K.model(7, True)
    s = engine.HostSpec()
    s.spec_begin(7, words, ptype, True)
    try:
        _, other, _ = s.spec_coding(seq, txs[:1], 2, rates)
        _, other0, _ = s.spec_coding(seq, txs[:1], 0, rates)
    finally:
        s.spec_end()
    # the codons of 12 and 33 (3 positions each) and the splice positions 17 and 58 have no class
    assert other[0, 7] == 3 + 3 + 2 and other0[0, 7] == 6
    # the N at 8 and 68 only spoils windows: those pairs keep their class
    assert other[0, 5] > 0 and other[0, 4] == 3 * (8 - 2)


def test_random_transcripts():
    seq, txs = K.random_case(1, 3000, 40)
    _against_oracle(5, True, [(seq, txs, 2)])
    _against_oracle(4, False, [(seq, txs, 3)])


def _err(fn, code, text):
    with pytest.raises(engine.KPError) as e:
        fn()
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_argument_and_state_errors():
    s = engine.HostSpec()
    seq = K.table_case()[0]
    ok = [(0, [(0, 6)])]
    _err(lambda: s.spec_coding(seq, ok), -4, "no session")
    _err(lambda: s.spec_coding_sites(seq, ok, [0], b"C", [0]), -4, "no session")
    names, words, ptype, rates = K.model(3, True)
    s.spec_begin(3, words, ptype, True)
    try:
        _err(lambda: s.spec_coding(seq, ok + [(1, [(0, 3), (10, 14)])]), -1, "transcript 1 hold 7 bases")
        _err(lambda: s.spec_coding(seq, [(0, [(0, 4), (3, 5)])]), -1, "transcript 0 are not ascending")
        _err(lambda: s.spec_coding(seq, [(0, [(3, 3), (4, 7)])]), -1, "is empty")
        _err(lambda: s.spec_coding(seq, [(0, [(190, 193)])]), -1, "outside the contig")
        _err(lambda: s.spec_coding(seq, ok, splice=9), -1, "splice must be 0..8")
        _err(lambda: s.spec_coding_sites(seq, ok, [0], b"C", [1]), -1, "names transcript 1 of 1")
        _err(lambda: s.spec_coding_sites(seq, ok, [192], b"C", [0]), -1, "lies past the contig")
        _err(lambda: s.spec_coding_sites(seq, ok, [0], b"N", [0]), -1, "none of ACGTacgt")
        with pytest.raises(ValueError):
            s.spec_coding(seq, ok, rates=rates[:-1])
        with pytest.raises(ValueError):
            s.spec_coding(seq, [(2, [(0, 3)])])
        # nothing to do is fine; a site outside the transcript, ALT = REF
        hist, other, exp = s.spec_coding(seq, [], 2, rates)
        assert hist.shape == (0, 5, len(names)) and other.shape == (0, 8) and exp.shape == (0, 5, 12)
        cls, pid, codons = s.spec_coding_sites(seq, ok, [6, 3, 1], b"CAC", [0, 0, 0])
        assert cls.tolist() == [C.NOT_IN, C.ALT_IS_REF, 1] and pid[1] == R.ALT_IS_REF and codons[:2].tolist() == [0, 0]
    finally:
        s.spec_end()


GTF = """# a comment
chr1\tsrc\texon\t1\t40\t.\t+\t.\tgene_id "G1"; transcript_id "T1"; gene_name "ABC";
chr1\tsrc\tCDS\t31\t36\t.\t+\t0\tgene_id "G1"; transcript_id "T1"; gene_name "ABC";
chr1\tsrc\tCDS\t11\t16\t.\t+\t0\tgene_id "G1"; transcript_id "T1"; gene_name "ABC";
chr2\tsrc\tCDS\t5\t13\t.\t-\t2\ttranscript_id "T2"; gene_id "G2";
chr1\tsrc\tCDS\t61\t66\t.\t+\t0\tgene_id "G1"; transcript_id "T1";
"""


def test_readers():
    txs = seqio.read_gtf_cds(io.BytesIO(GTF.encode()))
    assert [(t.name, t.gene, t.contig, t.strand, t.segments) for t in txs] == [
        ("T1", "ABC", "chr1", 0, [(10, 16), (30, 36), (60, 66)]), ("T2", "G2", "chr2", 1, [(4, 13)])]
    bed = "track name=x\nchr1 10 16 T1 0 +\nchr2 4 13 T2 0 -\nchr1 60 66 T1 0 +\nchr1 30 36 T1 0 +\n"
    got = seqio.read_cds_bed(io.BytesIO(bed.encode()))
    assert [(t.name, t.gene, t.contig, t.strand, t.segments) for t in got] == [
        ("T1", None, "chr1", 0, [(10, 16), (30, 36), (60, 66)]), ("T2", None, "chr2", 1, [(4, 13)])]
    for bad, text in (("chr1 0 3 T 0 +\nchr2 5 8 T 0 +\n", "two contigs"), ("chr1 0 3 T 0 +\nchr1 5 8 T 0 -\n", "both strands"),
                      ("chr1 0 5 T 0 +\nchr1 4 8 T 0 +\n", "overlapping"), ("chr1 0 5 T 0 .\n", "strand"),
                      ("chr1 0 5 T\n", "BED6")):
        with pytest.raises(ValueError, match=text):
            seqio.read_cds_bed(io.BytesIO(bad.encode()))
    with pytest.raises(ValueError, match="transcript_id"):
        seqio.read_gtf_cds(io.BytesIO(b'chr1\ts\tCDS\t1\t3\t.\t+\t0\tgene_id "G";\n'))


def _genome(tmp_path):
    seq1, _ = K.invalid_case()
    seq2 = R.random_seq(np.random.RandomState(2), 50, lower=0.3)
    path = str(tmp_path / "g.fa")
    R.write_fasta(path, [("chr1", seq1), ("chr2", seq2)])
    return path, {"chr1": seq1, "chr2": seq2}


def _expected_lines(seqs, txs, model, fold, splice, scale, observed, by_type):
    """The ``coding`` table formatted from the oracle."""
    names, ptype, rates = model
    tids = sorted(set(ptype))
    head = ["#name", "gene", "contig", "strand", "cds_bases"] + [f"opp_{c}" for c in C.CLASS_NAMES]
    head += [f"exp_{c}" for c in C.CLASS_NAMES] + ["unrated", "no_class"]
    head += [f"obs_{c}" for c in C.CLASS_NAMES] if observed is not None else []
    head += [f"exp_{c}_{R.ALL_TYPES[t]}" for c in C.CLASS_NAMES for t in tids] if by_type else []
    lines = [" ".join(head) + "\n"]
    for t in txs:
        usable = t.length % 3 == 0 and t.contig in seqs
        if usable:
            _, other, exp = C.coding(seqs[t.contig], names, ptype, fold, [(t.strand, t.segments)], splice, rates)
        else:
            other, exp = np.zeros((1, 8), np.uint64), np.zeros((1, 5, 12))
        tok = [t.name, t.gene or ".", t.contig, "+-"[t.strand], str(t.length)] + [str(int(x)) for x in other[0, :5]]
        for c in range(5):
            acc = 0.0
            for ty in range(12):
                acc = acc + float(exp[0, c, ty])
            tok.append(repr(acc * scale))
        tok += [str(int(other[0, 5] + other[0, 6])), str(int(other[0, 7]))]
        if observed is not None:
            obs = [0] * 5
            for chrom, p1, ref, alt in observed:
                if usable and chrom == t.contig and seqs[chrom][p1 - 1] & 0xDF == ord(ref):
                    c = C.pair(seqs[chrom], t.strand, t.segments, splice, p1 - 1, alt)[0]
                    if c >= 0:
                        obs[c] += 1
            tok += [str(x) for x in obs]
        if by_type:
            tok += [repr(float(exp[0, c, ty]) * scale) for c in range(5) for ty in tids]
        lines.append(" ".join(tok) + "\n")
    return lines


def test_command_lines(tmp_path, capsys):
    genome, seqs = _genome(tmp_path)
    k, fold = 5, True
    names, _, ptype, rates = K.model(k, fold)
    spectrum.Model(names, ptype, rates).write(str(tmp_path / "model.txt"))
    gtf = str(tmp_path / "a.gtf")
    with open(gtf, "w") as f:  # T3 is 7 bases long, T4 lies on a contig the genome does not have
        f.write(GTF + 'chr2\ts\tCDS\t20\t26\t.\t+\t0\ttranscript_id "T3";\nchr9\ts\tCDS\t1\t6\t.\t+\t0\ttranscript_id "T4";\n'
                + 'chr1\ts\tCDS\t13\t33\t.\t-\t0\ttranscript_id "T5"; gene_id "G5";\n')
    txs = seqio.read_gtf_cds(gtf)
    s1 = C.text(seqs["chr1"])
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    observed = [("chr1", p, s1[p - 1].upper(), other[s1[p - 1].upper()]) for p in (11, 14, 15, 17, 31, 36, 59, 66, 70, 2)
                if s1[p - 1].upper() in other]
    observed += [("chr1", 32, other[s1[31].upper()], s1[31].upper()), ("chr2", 5, C.text(seqs["chr2"])[4].upper(), "A"),
                 ("chr7", 5, "A", "C")]
    observed = [x for x in observed if x[2] != x[3]]
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        f.write("".join(f"{c} {p} {r} {a}\n" for c, p, r, a in observed) + "chr1 12 AC A\n")
    base = ["--model", str(tmp_path / "model.txt")]
    out = str(tmp_path / "coding.txt")
    argv = ["coding", genome, "--gtf", gtf, "--observed", sites, "--by-type", "--scale", "0.5", "--splice", "3", "-o", out]
    assert spectrum.main(argv + base, host=True) == 0
    err = dict(x.split("=") for x in capsys.readouterr().err.split())
    assert (err["transcripts"], err["skipped_length"], err["unknown_contig_transcripts"]) == ("5", "1", "1")
    assert (err["lines"], err["not_snv"], err["ref_mismatch"], err["unknown_contig"]) == (str(len(observed) + 1), "1", "1", "1")
    want = _expected_lines(seqs, txs, (names, ptype, rates), fold, 3, 0.5, observed, True)
    assert open(out).readlines() == want
    inside = {(c, p) for c, p, r, a in observed if c in seqs and seqs[c][p - 1] & 0xDF == ord(r) and any(
        t.contig == c and t.length % 3 == 0 and C.pair(seqs[c], t.strand, t.segments, 3, p - 1, a)[0] != C.NOT_IN for t in txs)}
    kept = sum(1 for c, p, r, a in observed if c in seqs and seqs[c][p - 1] & 0xDF == ord(r))
    assert int(err["observed_outside"]) == kept - len(inside) > 0
    assert sum(int(x) for line in want[1:] for x in line.split()[17:22]) >= 5
    # the plain table from a BED6 annotation, on standard output
    bed = str(tmp_path / "cds.bed")
    with open(bed, "w") as f:
        f.write("".join(f"{t.contig} {b} {e} {t.name} 0 {'+-'[t.strand]}\n" for t in txs for b, e in t.segments))
    assert spectrum.main(["coding", genome, "--cds-bed", bed, "--verbosity", "0"] + base, host=True) == 0
    for t in txs:
        t.gene = None
    assert capsys.readouterr().out.splitlines(True) == _expected_lines(seqs, txs, (names, ptype, rates), fold, 2, 1.0, None, False)
    # consequences: one line per site and transcript that holds it, sites in file order
    out = str(tmp_path / "cons.txt")
    assert spectrum.main(["consequences", genome, "--cds-bed", bed, sites, "-o", out] + base, host=True) == 0
    err = dict(x.split("=") for x in capsys.readouterr().err.split())
    want = []
    for chrom, p1, ref, alt in observed:
        if chrom not in seqs or seqs[chrom][p1 - 1] & 0xDF != ord(ref):
            continue
        for t in txs:
            if t.contig != chrom or t.length % 3:
                continue
            c, rc, ac = C.pair(seqs[chrom], t.strand, t.segments, 2, p1 - 1, alt)
            if c == C.NOT_IN:
                continue
            pid = int(R.sites(seqs[chrom], names, ptype, fold, [p1 - 1], [alt])[0])
            part = f"{R.ALL_TYPES[ptype[pid]]} {names[pid]} {float(rates[pid])!r}" if pid >= 0 else "NA NA NA"
            if 0 <= c <= 3:
                tail = f"{C.CLASS_NAMES[c]} {rc} {ac} {C.AMINO[rc]} {C.AMINO[ac]}"
            else:
                tail = (C.CLASS_NAMES[4] if c == 4 else "NA") + " NA NA NA NA"
            want.append(f"{chrom} {p1} {ref} {alt} {part} {t.name} {tail}\n")
    got = open(out).readlines()
    assert got == want and len(want) > 8 and any(" splice " in x for x in want) and any(" T5 " in x for x in want)
    assert int(err["sites_outside"]) > 0 and err["skipped_length"] == "1"
    # input errors: exit code 2
    for argv in (["coding", genome, "--cds-bed", bed, "--splice", "9"], ["coding", genome, "--gtf", sites]):
        assert spectrum.main(argv + base, host=True) == 2
        assert "input error" in capsys.readouterr().err
    two = str(tmp_path / "two.bed")
    with open(two, "w") as f:
        f.write("chr1 0 3 T 0 +\nchr2 5 8 T 0 +\n")
    assert spectrum.main(["consequences", genome, "--cds-bed", two, sites] + base, host=True) == 2
    assert "two contigs" in capsys.readouterr().err


def test_batches_change_nothing():
    seq, raw = K.random_case(2, 2000, 25)
    txs = [seqio.Transcript(f"t{i}", None, "c", st, segs) for i, (st, segs) in enumerate(raw)]
    names, _, ptype, rates = K.model(3, True)
    model = spectrum.Model(names, ptype, rates)
    whole = spectrum.coding_rates([("c", seq)], model, txs, by_type=True, host=True)
    small = spectrum.coding_rates([("c", seq)], model, txs, by_type=True, host=True, budget=5 * len(names) * 4)
    for key in ("other", "expected", "expected_by_type", "status"):
        assert whole[key].tobytes() == small[key].tobytes()
    assert whole["other"][:, :5].sum() > 0 and not whole["status"].any()
