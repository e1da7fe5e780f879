"""An independent oracle for the indel breakpoint counts (kmerpapa_amd.count.count_indels,
kp_indel.h), written from the semantics of include/kmerpapa_hip.h with Python strings and
collections.Counter.  It shares no code with the library.  A site is ``("ins", b, string, key)`` or
``("del", s, length, key)``; tables are Counters of k-mers."""
from collections import Counter

from tests import sim_ref
from tests.seq_ref import COMPLEMENT, revcomp

TAG = 0x494E444C
COLUMNS = ("ins", "del_start", "del_end")
MIRROR = {"ins": "ins", "del_start": "del_end", "del_end": "del_start"}


def same(x, y):
    """Two bytes are the same base: case is ignored, an invalid byte equals nothing."""
    return x.upper() in COMPLEMENT and x.upper() == y.upper()


def trim(ref, alt):
    """``(prefix length, ref, alt)`` after the longest common prefix, then the longest common
    suffix of the rest, are gone."""
    q = 0
    while ref[q:] and alt[q:] and ref[q] == alt[q]:
        q += 1
    ref, alt = ref[q:], alt[q:]
    while ref and alt and ref[-1] == alt[-1]:
        ref, alt = ref[:-1], alt[:-1]
    return q, ref, alt


def classify(ref, alt):
    """A ``CHROM POS REF ALT`` line's kind: ``("ins", offset, string)``, ``("del", offset, length)``
    (offset from POS - 1), ``"complex"`` or ``"not_indel"``.  ``-`` and ``.`` are empty alleles."""
    ref, alt = ("" if x in "-." else x.upper() for x in (ref, alt))
    if set(ref + alt) - set("ACGT"):
        return "not_indel"
    q, r, a = trim(ref, alt)
    if r and a:
        return "not_indel" if len(r) == len(a) == 1 else "complex"
    if not r and not a:
        return "not_indel"
    return ("ins", q, a) if a else ("del", q, len(r))


def interval(seq, site):
    """``(lo, hi)`` by the two formulas of the header."""
    n = len(seq)
    if site[0] == "ins":
        _, b, ins, _ = site
        L = len(ins)
        a = 0
        while b - 1 - a >= 0 and same(seq[b - 1 - a], ins[(L - 1 - a) % L]):
            a += 1
        c = 0
        while b + c < n and same(seq[b + c], ins[c % L]):
            c += 1
        return b - a, b + c
    _, s, L, _ = site
    e = s + L
    a = 0
    while s - 1 - a >= 0 and same(seq[s - 1 - a], seq[e - 1 - a]):
        a += 1
    c = 0
    while e + c < n and same(seq[s + c], seq[e + c]):
        c += 1
    return s - a, s + c


def mutated(seq, site):
    if site[0] == "ins":
        return seq[:site[1]] + site[2] + seq[site[1]:]
    return seq[:site[1]] + seq[site[1] + site[2]:]


def brute_interval(seq, site):
    """The definition: every placement of an indel of the same kind and length whose mutated
    sequence equals the site's (pure upper-case ACGT contigs only)."""
    want = mutated(seq, site)
    if site[0] == "ins":
        L = len(site[2])
        hits = [b for b in range(len(seq) + 1) if seq[:b] + want[b:b + L] + seq[b:] == want]
    else:
        L = site[2]
        hits = [s for s in range(len(seq) - L + 1) if seq[:s] + seq[s + L:] == want]
    assert hits == list(range(hits[0], hits[-1] + 1)), "the class is not contiguous"
    return hits[0], hits[-1]


def representative(seq, site, p):
    """The same mutation written at breakpoint ``p`` of its interval: an inserted string rotates."""
    if site[0] == "del":
        return ("del", p, site[2], site[3])
    _, b, ins, key = site
    L = len(ins)
    want = mutated(seq, site)
    return ("ins", p, want[p:p + L], key)


def place(lo, hi, how, seed=0, contig=0, key=0):
    if how == "left":
        return lo
    if how == "right":
        return hi
    x0 = sim_ref.philox((key & sim_ref.M32, key >> 32, contig, TAG), (seed & sim_ref.M32, seed >> 32))[0]
    return lo + ((x0 * (hi - lo + 1)) >> 32)


def window(seq, b, k):
    """The window of breakpoint ``b``: None if it runs off the contig or holds an invalid byte."""
    r = k // 2
    if b - r < 0 or b + r > len(seq):
        return None
    w = seq[b - r:b + r].upper()
    return w if all(c in COMPLEMENT for c in w) else None


def count(seq, k, sites, both, how="left", seed=0, contig=0, scan=True, regions=None):
    """``({column: Counter}, bg Counter, stats, resolved rows)`` of one contig."""
    cols = {c: Counter() for c in COLUMNS}
    bg = Counter()
    st = {"windows": 0, "windows_invalid": 0, "sites": 0, "sites_skipped": 0}

    def add(col, w):
        cols[col][w] += 1
        if both:
            cols[MIRROR[col]][revcomp(w)] += 1

    resolved = []
    for site in sites:
        lo, hi = interval(seq, site)
        p = place(lo, hi, how, seed, contig, site[3])
        resolved.append((lo, hi, p))
        w = window(seq, p, k)
        if site[0] == "ins":
            if w is None:
                st["sites_skipped"] += 1
                continue
            add("ins", w)
        else:
            e = window(seq, p + site[2], k)
            if w is None or e is None:
                st["sites_skipped"] += 1
                continue
            add("del_start", w)
            add("del_end", e)
        st["sites"] += 1
    if scan:
        centres = set(range(len(seq) + 1))
        if regions is not None:
            centres = set()
            for b, e in regions:
                centres.update(range(int(b), int(e)))
        r = k // 2
        for b in sorted(centres):
            if b - r < 0 or b - r + k > len(seq):
                continue
            w = window(seq, b, k)
            if w is None:
                st["windows_invalid"] += 1
                continue
            st["windows"] += 1
            bg[w] += 1
            if both:
                bg[revcomp(w)] += 1
    return cols, bg, st, resolved
