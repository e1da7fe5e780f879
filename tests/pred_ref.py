"""An independent oracle for kmerpapa_amd.predict (kp_pred.h): plain Python over strings -- a
window per centre from tests.seq_ref, IUPAC letters as sets of bases, and the literal loop that
defines ``expected``.  It shares no code with the library."""
import numpy as np

from tests.seq_ref import random_seq, revcomp, text, window, write_2bit, write_fasta  # noqa: F401 (re-exported)

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "M": "AC", "R": "AG", "W": "AT", "S": "CG", "Y": "CT", "K": "GT",
         "V": "ACG", "H": "ACT", "D": "AGT", "B": "CGT", "N": "ACGT"}
LETTER = {frozenset(v): key for key, v in IUPAC.items()}
NONE, INVALID = -1, -2


def matches(kmer, pattern):
    return all(c in IUPAC[p] for c, p in zip(kmer, pattern))


def pattern_of(kmer, patterns):
    """Index of the pattern ``kmer`` belongs to, or -1; the patterns must be disjoint."""
    hit = [i for i, p in enumerate(patterns) if matches(kmer, p)]
    assert len(hit) <= 1
    return hit[0] if hit else NONE


def pid_at(seq, centre, patterns, fold, cache=None):
    """The code of kp_pred_track at one position of the contig ``seq`` (a str)."""
    k = len(patterns[0])
    w = window(seq, centre, k, fold)
    if w is None or w == "off":
        return INVALID
    if cache is None:
        return pattern_of(w, patterns)
    if w not in cache:
        cache[w] = pattern_of(w, patterns)
    return cache[w]


def track(seq, patterns, fold, begin=0, end=None, cache=None):
    seq = text(seq)
    cache = {} if cache is None else cache
    end = len(seq) if end is None else end
    return np.array([pid_at(seq, c, patterns, fold, cache) for c in range(begin, end)], np.int32).reshape(-1)


def expected_of(hist_row, rates):
    acc = 0.0
    for p in range(len(rates)):
        acc = acc + float(int(hist_row[p])) * float(rates[p])
    return acc


def regions(seq, patterns, fold, regs, rates=None):
    """``(hist [m, P], other [m, 2], expected [m] or None)`` of kp_pred_regions."""
    pid = track(seq, patterns, fold)
    P = len(patterns)
    hist = np.zeros((len(regs), P), np.uint64)
    other = np.zeros((len(regs), 2), np.uint64)
    for r, (b, e) in enumerate(regs):
        for j in pid[int(b):int(e)].tolist():
            if j >= 0:
                hist[r, j] += 1
            else:
                other[r, 0 if j == NONE else 1] += 1
    exp = None if rates is None else np.array([expected_of(hist[r], rates) for r in range(len(regs))], np.float64)
    return hist, other, exp


def random_partition(rng, gen_pat, n_leaves):
    """A partition of ``gen_pat`` into ``n_leaves`` patterns: starting from the general pattern, a
    random leaf is split at a random ambiguous position into two non-empty complementary IUPAC
    subsets, until there are enough.  Disjoint by construction, and covers ``gen_pat`` exactly."""
    def ambiguous(p):
        return any(len(IUPAC[c]) > 1 for c in p)

    leaves = [gen_pat]
    cand = [0] if ambiguous(gen_pat) else []  # leaves that can still be split
    while len(leaves) < n_leaves:
        assert cand, "the general pattern has fewer k-mers than leaves asked for"
        at = rng.randint(len(cand))
        i = cand[at]
        cand[at] = cand[-1]
        cand.pop()
        p = leaves[i]
        amb = [j for j, c in enumerate(p) if len(IUPAC[c]) > 1]
        j = amb[rng.randint(len(amb))]
        bases = list(IUPAC[p[j]])
        while True:
            pick = [b for b in bases if rng.randint(2)]
            if 0 < len(pick) < len(bases):
                break
        rest = [b for b in bases if b not in pick]
        leaves[i] = p[:j] + LETTER[frozenset(pick)] + p[j + 1:]
        leaves.append(p[:j] + LETTER[frozenset(rest)] + p[j + 1:])
        cand += [x for x in (i, len(leaves) - 1) if ambiguous(leaves[x])]
    order = rng.permutation(len(leaves))
    return [leaves[i] for i in order]


def wide_rates(rng, n):
    """Rates over twelve orders of magnitude: the order of the adds of ``expected`` matters."""
    return (10.0 ** rng.uniform(-12, 0, size=n)) * rng.uniform(0.1, 1.0, size=n)
