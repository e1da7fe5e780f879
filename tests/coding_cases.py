"""Shared inputs and checks of tests/test_coding.py (host session against the oracle) and
tests/test_gpu_coding.py (device against the host session): small contigs with transcripts at the
places where the codon work can go wrong, and the comparison of one session's results with a
reference's, for equality throughout."""
import numpy as np

from kmerpapa_amd import engine
from tests import coding_ref as C
from tests import spec_ref as R

word = engine.pattern_word
KSETS = [(1, True), (3, True), (5, True), (7, True), (4, False)]
SPLIT_LENGTHS = [[1, 1, 1], [2, 4], [4, 2], [1, 5], [3, 3]]
INTRONS = [1, 3, 4, 50]
SPLICES = [0, 2, 8]

_models = {}


def model(k, fold, leaves=6):
    """``(names, words, ptype, rates)`` of a random model of every type but one (so that some pairs
    have no pattern), cached."""
    key = (k, fold, leaves)
    if key not in _models:
        rng = np.random.RandomState(100 * k + fold + leaves)
        names, ptype, rates = R.random_model(rng, k, fold, 6 if fold else 12, leaves, empty=1)
        _models[key] = (names, [word(x) for x in names], ptype, rates)
    return _models[key]


def _seq(seed, n, lower=0.2):
    return R.random_seq(np.random.RandomState(seed), n, lower=lower)


def table_case():
    """The 64 codons in a row, one transcript per strand."""
    seq = np.frombuffer("".join(a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT").encode(), np.uint8).copy()
    return seq, [(0, [(0, 192)]), (1, [(0, 192)])]


def split_case(lengths, intron, lead=9):
    """Segments of ``lengths`` bases with ``intron`` bases between them, on both strands."""
    n = 2 * lead + sum(lengths) + intron * (len(lengths) - 1)
    seq = _seq(7 * sum(lengths) + 31 * intron + len(lengths), n)
    segs, at = [], lead
    for x in lengths:
        segs.append((at, at + x))
        at += x + intron
    return seq, [(0, segs), (1, segs)]


def invalid_case():
    """An N in a codon, in a splice position and in a window only; lower case."""
    seq = _seq(5, 120, lower=0.5)
    segs = [(10, 16), (30, 36), (60, 66)]
    for p in (12, 17, 8, 58, 33, 68):  # codon, splice, window only, splice (far end), codon, window only
        seq[p] = ord("N") if p != 58 else ord("n")
    return seq, [(0, segs), (1, segs)]


def ends_case():
    """Segments that start at base 0 and end at base n."""
    seq = _seq(9, 30)
    segs = [(0, 4), (10, 15), (27, 30)]
    return seq, [(0, segs), (1, segs), (0, [(0, 30)])]


def overlap_case():
    """Two overlapping transcripts on opposite strands (and one without segments)."""
    seq = _seq(11, 70)
    return seq, [(0, [(5, 20), (40, 55)]), (1, [(10, 22), (38, 47)]), (0, [])]


def small_cases():
    """``name: (seq, transcripts)`` of every small case."""
    out = {"table": table_case(), "invalid": invalid_case(), "ends": ends_case(), "overlap": overlap_case()}
    for lengths in SPLIT_LENGTHS:
        for intron in INTRONS + [0]:
            out["split_" + "".join(map(str, lengths)) + f"_{intron}"] = split_case(lengths, intron)
    return out


def random_case(seed, n, n_tx, max_segs=6):
    """``n_tx`` random transcripts on a contig of ``n`` bases with a few invalid bytes: both
    strands, overlapping each other, segments of 1..60 bases and introns of 0..40."""
    rng = np.random.RandomState(seed)
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.002)
    txs = []
    while len(txs) < n_tx:
        lens = rng.randint(1, 61, size=rng.randint(1, max_segs + 1)).tolist()
        lens[-1] += (-sum(lens)) % 3
        gaps = rng.randint(0, 41, size=len(lens) - 1).tolist()
        span = sum(lens) + sum(gaps)
        at = int(rng.randint(0, n - span + 1))
        if len(txs) == 0:
            at = 0  # one transcript at each end of the contig
        if len(txs) == 1:
            at = n - span
        segs = []
        for x, g in zip(lens, gaps + [0]):
            segs.append((at, at + x))
            at += x + g
        txs.append((int(rng.randint(0, 2)), segs))
    return seq, txs


def bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint64)


def run(s, seq, transcripts, splice, rates):
    """Every result of one session ``s`` for a case: kp_spec_coding's arrays and counts, and
    kp_spec_coding_sites' over every possible pair."""
    hist, other, exp = s.spec_coding(seq, transcripts, splice, rates)
    st = s.spec_coding_stats()
    pos, alts, tx = C.all_pairs(seq, transcripts, splice)
    cls, pid, codons = s.spec_coding_sites(seq, transcripts, pos, alts, tx, splice)
    return {"hist": hist, "other": other, "exp": exp, "cls": cls, "pid": pid, "codons": codons,
            "counts": (st["items"], st["positions"], st["pairs"]), "sites": (pos, alts, tx)}


def check_identities(got, transcripts, splice):
    """The two identities of other[8], and kp_spec_coding_sites agreeing with kp_spec_coding: the
    classes of all possible pairs, counted per transcript, are other[0..4]."""
    other, hist = got["other"].astype(np.int64), got["hist"].astype(np.int64)
    pos, alts, tx = got["sites"]
    for t, (_, segs) in enumerate(transcripts):
        positions = sum(e - b for b, e in segs) + len(C.splice_positions([(int(b), int(e)) for b, e in segs], splice))
        assert other[t, :5].sum() == hist[t].sum() + other[t, 5] + other[t, 6]
        assert 3 * positions == other[t, :5].sum() + 3 * other[t, 7]
        mine = got["cls"][tx == t]
        assert (mine >= 0).sum() + (mine == C.NO_CLASS).sum() == mine.shape[0]
        assert np.array_equal(np.bincount(mine[mine >= 0], minlength=5), other[t, :5])
    assert got["counts"][2] == other[:, :5].sum()


def same(got, want, counts=True):
    for key in ("hist", "other", "cls", "pid", "codons"):
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert np.array_equal(bits(got["exp"]), bits(want["exp"]))
    if counts:
        assert got["counts"] == want["counts"]


def oracle(seq, names, ptype, fold, transcripts, splice, rates):
    hist, other, exp = C.coding(seq, names, ptype, fold, transcripts, splice, rates)
    pos, alts, tx = C.all_pairs(seq, transcripts, splice)
    cls, pid, codons = C.coding_sites(seq, names, ptype, fold, transcripts, splice, pos, alts, tx)
    return {"hist": hist, "other": other, "exp": exp, "cls": cls, "pid": pid, "codons": codons}
