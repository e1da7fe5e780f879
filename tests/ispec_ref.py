"""An independent oracle for the indel-model session (kp_ispec.h), written from the semantics of
include/kmerpapa_hip.h: a loop over breakpoints with string windows, ``pattern_utils.matches`` for
the k-mers of a pattern and a reverse complement by string reversal.  It shares no code with the
library; a site's interval and placement are tests/indel_ref.py's.  Patterns are IUPAC strings,
kinds 0 (ins) and 1 (del)."""
from kmerpapa_amd.pattern_utils import matches
from tests import indel_ref as R
from tests.seq_ref import revcomp

NONE, INVALID = -1, -2


def lookup(patterns, kinds):
    """``[{k-mer: first pattern of kind 0}, {k-mer: first pattern of kind 1}]``."""
    out = [{}, {}]
    for p, (pat, kind) in enumerate(zip(patterns, kinds)):
        for kmer in matches(pat):
            out[kind].setdefault(kmer, p)
    return out


def entry(tabs, w):
    """The four ids of a valid window: ins of w, ins of rc(w), del of w, del of rc(w)."""
    rc = revcomp(w)
    return [tabs[0].get(w, NONE), tabs[0].get(rc, NONE), tabs[1].get(w, NONE), tabs[1].get(rc, NONE)]


def regions(seq, k, patterns, kinds, regs, rates=None):
    """``(hist [m][2][P], other [m][5], expected [m][4] or None)`` as Python lists."""
    tabs = lookup(patterns, kinds)
    P = len(patterns)
    hist, other, exp = [], [], []
    for begin, end in regs:
        h = [[0] * P, [0] * P]
        o = [0] * 5
        for b in range(int(begin), int(end)):
            w = R.window(seq, b, k)
            if w is None:
                o[4] += 1
                continue
            for e, p in enumerate(entry(tabs, w)):
                if p == NONE:
                    o[e] += 1
                else:
                    h[e & 1][p] += 1
        hist.append(h)
        other.append(o)
        if rates is not None:
            row = []
            for kind in (0, 1):
                for strand in (0, 1):
                    acc = 0.0
                    for p in range(P):
                        if kinds[p] == kind:
                            acc = acc + float(h[strand][p]) * float(rates[p])
                    row.append(acc)
            exp.append(row)
    return hist, other, (exp if rates is not None else None)


def track(seq, k, patterns, kinds, begin, end):
    """Four planes over the breakpoints ``[begin, end)``."""
    tabs = lookup(patterns, kinds)
    planes = [[], [], [], []]
    for b in range(begin, end):
        w = R.window(seq, b, k)
        ids = [INVALID] * 4 if w is None else entry(tabs, w)
        for e in range(4):
            planes[e].append(ids[e])
    return planes


def sites(seq, k, patterns, kinds, site_list, how="left", seed=0, contig=0):
    """``(pid rows, resolved rows)`` of indel_ref sites."""
    tabs = lookup(patterns, kinds)
    pid, resolved = [], []
    for site in site_list:
        lo, hi = R.interval(seq, site)
        p = R.place(lo, hi, how, seed, contig, site[3])
        resolved.append([lo, hi, p])
        w = R.window(seq, p, k)
        if site[0] == "ins":
            pid.append([INVALID, INVALID] if w is None else [tabs[0].get(w, NONE), tabs[0].get(revcomp(w), NONE)])
            continue
        e = R.window(seq, p + site[2], k)
        if w is None or e is None:
            pid.append([INVALID, INVALID])
        else:
            pid.append([tabs[1].get(w, NONE), tabs[1].get(revcomp(e), NONE)])
    return pid, resolved
