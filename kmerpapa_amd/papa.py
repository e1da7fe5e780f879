"""Patterns and pattern partitions (the reference's ``kmerpapa.papa``, src/kmerpapa/papa.py).

``Pattern`` (:3-50) is the containment helper the CLI's --super_pattern filter uses.
``PatternPartition`` (:53-107) keeps the reference's interface -- the constructor with its two
assertions, ``__len__``, ``pattern_length``, ``__getitem__``, ``__str__``, all plain host
code -- and adds what the reference stops short of: the full validity check (with the pairwise
check the reference leaves commented out as slow) and the partition applied to a count
table, both on the GPU through ``engine.Device.apply`` (kp_apply).
"""
import numpy as np

from .pattern_utils import code, matches, set_code, set_perm_code, inv_code


class Pattern:
    """An IUPAC pattern that answers ``kmer in pattern``."""

    def __init__(self, pattern_string):
        self.pattern = pattern_string

    def __contains__(self, context):
        return all(c in set_code[p] for p, c in zip(self.pattern, context))

    def __str__(self):
        return self.pattern

    __repr__ = __str__

    def __len__(self):
        return len(self.pattern)

    def __iter__(self):
        return matches(self.pattern)

    def __and__(self, other):
        out = []
        for a, b in zip(self.pattern, other.pattern):
            both = set_code[a] & set_code[b]
            if not both:
                return None
            out.append(inv_code[both])
        return Pattern("".join(out))

    def __le__(self, other):
        return all(x in set_perm_code[y] for x, y in zip(self.pattern, other.pattern))

    def cardinality(self):
        n = 1
        for x in self.pattern:
            n *= len(code[x])
        return n


class PatternPartition:
    """A k-mer pattern partition (papa.py:53-107).

    The constructor sorts ``patterns`` in place and asserts, as the reference does, that
    every pattern is a sub-pattern of the super pattern and that the cardinalities add up to
    the super pattern's.  :meth:`check`, :meth:`assign`, :meth:`counts` and :meth:`loglik`
    run on the first visible GPU (``host=True``: the same code serially on the host,
    ``engine.apply_host``); pattern indices everywhere refer to the sorted ``patterns``."""

    def __init__(self, patterns, superPattern=None, strandSymmetry=True):
        patterns.sort()
        self.patterns = [Pattern(p) for p in patterns]
        if superPattern is None:
            sp = "N" * len(patterns[0])
            if strandSymmetry:
                radius = len(patterns[0]) // 2
                sp = "N" * radius + "M" + "N" * radius
            self.superPattern = Pattern(sp)
        else:
            self.superPattern = Pattern(superPattern)
        n_matches = 0
        for i in range(len(self.patterns)):
            n_matches += self.patterns[i].cardinality()
            assert self.patterns[i] <= self.superPattern, \
                "pattern #%r (%r) is not a subpattern of the superPattern (%r)" \
                % (i, self.patterns[i], self.superPattern)
        assert n_matches == self.superPattern.cardinality(), \
            "the patterns does not cover the superPattern (%r)" % (self.superPattern)

    def __len__(self):
        return len(self.patterns)

    def pattern_length(self):
        return len(self.patterns[0])

    def __getitem__(self, context):
        for p in self.patterns:
            if context in p:
                return p
        return None

    def __str__(self):
        res = ["[PatternPartition:"]
        for pattern in self.patterns:
            res.append(str(pattern) + " " + str(pattern.cardinality()))
        res.append("-" * len(self.patterns[0]))
        res.append(str(self.superPattern) + " " + str(self.superPattern.cardinality()) + "]")
        return "\n ".join(res)

    # ---- backed by kp_apply ----

    def _apply(self, codes, M, U, rates, want_pid, host):
        from . import engine
        k = self.pattern_length()
        words = [engine.pattern_word(str(p)) for p in self.patterns]
        sw = engine.pattern_word(str(self.superPattern))
        if host:
            return engine.apply_host(k, words, sw, codes, M, U, rates, want_pid)
        return engine.get_device(engine.visible_devices()[0]).apply(k, words, sw, codes, M, U, rates, want_pid)

    def _table(self, table):
        if table.k != self.pattern_length():
            raise ValueError(f"the table holds {table.k}-mers, the partition {self.pattern_length()}-mers")
        return table.codes, table.M, table.U

    def check(self, host=False):
        """The validity of the patterns alone: a dict of ``overlap_pairs`` (pattern pairs that
        share a k-mer: the reference's commented-out check) and ``outside_super`` (patterns
        that are not sub-patterns of the super pattern), with ``unmatched`` and ``multi`` = 0
        (those count table rows; see :meth:`apply`)."""
        z = np.zeros(0, np.int64)
        st = self._apply(np.zeros(0, np.uint64), z, z, None, False, host)[4]
        return {key: st[key] for key in ("unmatched", "multi", "overlap_pairs", "outside_super")}

    def apply(self, table, rates=None, want_pid=True, host=False):
        """Everything at once for a :class:`~kmerpapa_amd.io_utils.KmerCounts` table (sparse
        or full; ``M``/``U`` ``[n]`` or ``[n, ncol]``): ``(pid, pat_M, pat_U, ll, stats)`` as
        ``engine.Device.apply`` returns them."""
        return self._apply(*self._table(table), rates, want_pid, host)

    def assign(self, table, host=False):
        """Index of the pattern of every row of ``table`` (int32; -1 = no pattern matches the
        row, -2 = several do)."""
        return self.apply(table, host=host)[0]

    def counts(self, table, host=False):
        """Per-pattern ``(M, U)`` of ``table`` as ``KmerCounts.pattern_counts`` lists them (a
        list of int pairs; with several count columns, pairs of int tuples).  The table may be
        sparse; rows that match no pattern, or several, are counted nowhere."""
        _, pM, pU, _, _ = self.apply(table, want_pid=False, host=host)
        if pM.ndim == 1:
            return list(zip(pM.tolist(), pU.tolist()))
        return [(tuple(m), tuple(u)) for m, u in zip(pM.tolist(), pU.tolist())]

    def loglik(self, table, rates, host=False):
        """-2 log-likelihood of ``table`` under one rate per pattern
        (``score_utils.get_loss`` with penalty 0 of the table's per-pattern counts, with the
        given rates): a float, or a float64 array for several count columns."""
        ll = self.apply(table, rates=rates, want_pid=False, host=host)[3]
        return float(ll[0]) if np.asarray(table.M).ndim == 1 else ll
