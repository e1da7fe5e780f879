"""An independent oracle for the coding-consequence calls (kp_coding.h), written from the
definitions in include/kmerpapa_hip.h: plain Python over strings.  A transcript's CDS is spliced by
string slicing and, on the - strand, reverse-complemented as a whole; a codon is a slice of that
string; the genetic code is a dict from amino acid to its codons; windows, folding and slots are
tests.spec_ref's; the expected sums are Python floats added in the stated order.  It shares no code
with the library."""
import numpy as np

from tests import spec_ref as R
from tests.seq_ref import COMPLEMENT, revcomp, text

CLASS_NAMES = ["synonymous", "missense", "nonsense", "stop_lost", "splice"]
NOT_IN, NO_CLASS, ALT_IS_REF = -1, -2, -3

CODE = {
    "A": "GCT GCC GCA GCG", "R": "CGT CGC CGA CGG AGA AGG", "N": "AAT AAC", "D": "GAT GAC", "C": "TGT TGC",
    "Q": "CAA CAG", "E": "GAA GAG", "G": "GGT GGC GGA GGG", "H": "CAT CAC", "I": "ATT ATC ATA",
    "L": "TTA TTG CTT CTC CTA CTG", "K": "AAA AAG", "M": "ATG", "F": "TTT TTC", "P": "CCT CCC CCA CCG",
    "S": "TCT TCC TCA TCG AGT AGC", "T": "ACT ACC ACA ACG", "W": "TGG", "Y": "TAT TAC", "V": "GTT GTC GTA GTG",
    "*": "TAA TAG TGA",
}
AMINO = {codon: aa for aa, codons in CODE.items() for codon in codons.split()}
assert len(AMINO) == 64


def class_of(ref_codon, alt_codon):
    a, b = AMINO[ref_codon], AMINO[alt_codon]
    if a == b:
        return 0
    if b == "*":
        return 2
    if a == "*":
        return 3
    return 1


def codon_index(codon):
    return 16 * "ACGT".index(codon[0]) + 4 * "ACGT".index(codon[1]) + "ACGT".index(codon[2])


def _cds(seq, strand, segs):
    """The transcript-strand CDS string and, per genomic coding position, its index in it."""
    spliced = "".join(seq[b:e] for b, e in segs).upper()
    where = [g for b, e in segs for g in range(b, e)]
    assert len(spliced) % 3 == 0
    if strand:
        cds = "".join(COMPLEMENT.get(c, "N") for c in reversed(spliced))
        index = {g: len(where) - 1 - j for j, g in enumerate(where)}
    else:
        cds, index = spliced, {g: j for j, g in enumerate(where)}
    return cds, index


def splice_positions(segs, splice):
    out = []
    for (_, a), (b, _) in zip(segs[:-1], segs[1:]):
        pos = set(range(a, min(a + splice, b))) | set(range(max(b - splice, a), b))
        out += sorted(pos)
    return out


def pair(seq, strand, segs, splice, g, alt):
    """``(class, ref codon, alt codon)`` of one (position, forward ALT) pair of a transcript: the
    class 0..4 or NOT_IN / NO_CLASS / ALT_IS_REF, the codons as transcript-strand strings or None."""
    seq = text(seq)
    cds, index = _cds(seq, strand, segs)
    own, alt = seq[g].upper(), alt.upper()
    if g in index:
        t = index[g]
        codon = cds[t - t % 3:t - t % 3 + 3]
        if any(c not in COMPLEMENT for c in codon):
            return NO_CLASS, None, None
        if alt == own:
            return ALT_IS_REF, None, None
        new = COMPLEMENT[alt] if strand else alt
        changed = codon[:t % 3] + new + codon[t % 3 + 1:]
        return class_of(codon, changed), codon, changed
    if g in splice_positions(segs, splice):
        if own not in COMPLEMENT:
            return NO_CLASS, None, None
        return (ALT_IS_REF if alt == own else 4), None, None
    return NOT_IN, None, None


def _pattern_of(seq, patterns, ptype, fold, g, alt, cache):
    """The pattern of a pair: an index, R.NONE, or R.INVALID without a valid window."""
    w, ref, a = R.site_of(seq, g, alt, len(patterns[0]), fold)
    if w is None or w == "off":
        return R.INVALID
    return R.slots_of(w, patterns, ptype, cache)[R.slot(ref, a)]


def coding(seq, patterns, ptype, fold, transcripts, splice, rates=None):
    """``(hist [m, 5, P], other [m, 8], expected [m, 5, 12] or None)`` of kp_spec_coding;
    ``transcripts``: ``(strand, segments)`` each."""
    seq = text(seq)
    m, P = len(transcripts), len(patterns)
    hist = np.zeros((m, 5, P), np.uint64)
    other = np.zeros((m, 8), np.uint64)
    cache = {}
    for t, (strand, segs) in enumerate(transcripts):
        segs = [(int(b), int(e)) for b, e in segs]
        cds, index = _cds(seq, strand, segs)
        for g in sorted(index) + splice_positions(segs, splice):
            own = seq[g].upper()
            if g in index:
                at = index[g]
                codon = cds[at - at % 3:at - at % 3 + 3]
                bad = any(c not in COMPLEMENT for c in codon)
            else:
                bad = own not in COMPLEMENT
            if bad:
                other[t, 7] += 1
                continue
            for alt in "ACGT":
                if alt == own:
                    continue
                if g in index:
                    new = COMPLEMENT[alt] if strand else alt
                    cls = class_of(codon, codon[:at % 3] + new + codon[at % 3 + 1:])
                else:
                    cls = 4
                other[t, cls] += 1
                pid = _pattern_of(seq, patterns, ptype, fold, g, alt, cache)
                if pid == R.INVALID:
                    other[t, 5] += 1
                elif pid == R.NONE:
                    other[t, 6] += 1
                else:
                    hist[t, cls, pid] += 1
    exp = None
    if rates is not None:
        exp = np.array([[R.expected_of(hist[t, c], ptype, rates) for c in range(5)] for t in range(m)],
                       np.float64).reshape(m, 5, 12)
    return hist, other, exp


def coding_sites(seq, patterns, ptype, fold, transcripts, splice, pos, alts, tx):
    """``(cls, pid, codons)`` of kp_spec_coding_sites."""
    seq = text(seq)
    cls, codons = [], []
    for g, a, t in zip(pos, alts, tx):
        a = chr(a) if not isinstance(a, str) else a
        strand, segs = transcripts[int(t)]
        c, ref, alt = pair(seq, strand, [(int(b), int(e)) for b, e in segs], splice, int(g), a)
        cls.append(c)
        codons.append(codon_index(ref) | codon_index(alt) << 6 if ref is not None else 0)
    pid = R.sites(seq, patterns, ptype, fold, pos, alts)
    return np.array(cls, np.int32).reshape(-1), pid, np.array(codons, np.uint32).reshape(-1)


def all_pairs(seq, transcripts, splice):
    """Every (position, ALT != own base, transcript) of the transcripts' coding and splice
    positions whose own byte is a base: ``(pos, alts, tx)``."""
    seq = text(seq)
    pos, alts, tx = [], [], []
    for t, (strand, segs) in enumerate(transcripts):
        segs = [(int(b), int(e)) for b, e in segs]
        for g in [g for b, e in segs for g in range(b, e)] + splice_positions(segs, splice):
            for alt in "ACGT":
                if seq[g].upper() in COMPLEMENT and alt != seq[g].upper():
                    pos.append(g)
                    alts.append(ord(alt))
                    tx.append(t)
    return np.array(pos, np.uint64), np.array(alts, np.uint8), np.array(tx, np.uint32)


__all__ = ["AMINO", "CLASS_NAMES", "class_of", "coding", "coding_sites", "all_pairs", "pair", "revcomp"]
