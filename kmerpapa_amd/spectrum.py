"""The whole mutation spectrum in one genome pass: ``python -m kmerpapa_amd.spectrum`` (the
``kmerpapa-spectrum`` command).

A mutation-rate model is one partition per mutation type -- after strand folding ``A>C A>G A>T C>A
C>G C>T``, each fitted under its own super pattern (``NNANN``, ``NNCNN``).  ``kmerpapa-count``,
``kmerpapa`` and ``kmerpapa-predict`` handle one type per run; this module counts every type's
sites in one session (``engine.Device.seq_*_typed``), joins the per-type partitions into one model
file and takes the whole model back to the genome in one scan (``engine.Device.spec_*``,
kp_spec.h): a window's centre base is the (folded) REF, an ALT is one of the three other bases, and
its rank among them in ``ACGT`` order is its *slot*, so three slots per k-mer cover every type and
the type id is ``3 * code(REF) + slot``.  Semantics: include/kmerpapa_hip.h.  The reference has no
such step.

The model file is this project's own format: a header ``type pattern p_neg p_pos p_rate`` and one
row per pattern, grouped by type in id order, the patterns of a type in the order of its partition
file, rates as Python float reprs.

``track`` without ``--type`` writes, per position, the sum of the rates of the model's types with
the position's (folded) REF base, added in slot order from 0.0 -- the probability that the position
mutates at all.  A position gets a value only if every one of those types has a pattern for its
window (and the model has at least one such type): a partly covered position has no value.

``simulate`` draws a random mutation set from the model (``engine.Device.spec_simulate``,
kp_sim.h) and writes it as ``CHROM POS REF ALT`` lines that ``count``, ``fit`` and ``regions
--observed`` read: every position mutates into each of its types with the rate of the type's
pattern, at most once, by a counter-based random number of (seed, contig index, position,
replicate), so a run is repeatable and a ``--bed`` subset changes no draw.

``null`` builds the null distribution such draws imply for the mutation count of every region
(``engine.Device.spec_null``, kp_null.h): ``--replicates`` sets are drawn and counted per region in
one pass per contig, column ``j`` being exactly ``simulate --replicate F+j``, and each region gets
the mean, variance and range of its simulated counts and, with ``--observed``, empirical p-values.

``coding`` gives the table a burden or constraint test reads: per transcript the expected number of
synonymous, missense, nonsense, stop-lost and essential-splice mutations beside the mutational
opportunity and, with ``--observed``, the observed ones (``engine.Device.spec_coding``,
kp_coding.h).  The class of a (position, ALT) pair comes from the standard genetic code and the
transcript's CDS (``--gtf`` or ``--cds-bed``); its rate is the model's, as ``sites`` reports it.
``consequences`` writes the class, codons and amino acids of given mutations, one line per site
and transcript.

``coding-null`` joins the two: the null distribution of the mutation count per transcript and
class (``engine.Device.spec_coding_null``, kp_cnull.h).  Column ``j`` is exactly ``simulate
--replicate F+j`` classified as ``coding --observed`` classifies it; each transcript gets, per class
and for all classes and the loss-of-function ones together, the mean, variance and range of its
simulated counts and, with ``--observed``, the observed count and empirical p-values.
"""
import argparse
import contextlib
import gc
import os
import sys
import tempfile

import numpy as np

from . import seqio
from .apply import read_partition
from .predict import DEFAULT_BUDGET, _bed_lines, _by_contig, _region_array, _site_lines

BASES = "ACGT"
HEADER = ["type", "pattern", "p_neg", "p_pos", "p_rate"]
ALT_IS_REF = -3


def TYPES(fold=True):
    """The canonical type strings in id order: 6 with strand folding, 12 without."""
    return [f"{r}>{a}" for r in (BASES[:2] if fold else BASES) for a in BASES if a != r]


def type_id(text, fold=True):
    """The id of ``X>Y``: ``3 * code(REF) + slot``.  With ``fold`` the type is folded first as
    ``seqio.fold_type`` does (``G>A`` is ``C>T``)."""
    kind = seqio.parse_type(text)  # (validates; folded)
    if not fold:
        kind = text.upper()
    return TYPES(False).index(kind)


def slot_of(ref, alt):
    """The rank of ``alt`` among the bases other than ``ref`` in ``ACGT`` order."""
    return [b for b in BASES if b != ref.upper()].index(alt.upper())


def super_pattern(kind, k):
    """The super pattern a type is fitted under: N everywhere, REF in the centre."""
    return "N" * (k // 2) + kind[0] + "N" * (k - 1 - k // 2)


class Model:
    """One partition per mutation type.  ``types``: the type strings present, in id order;
    ``names``, ``ptype`` (type ids, uint32), ``rates`` (float64) and ``counts`` (``(M, U)``): one
    entry per pattern, grouped by type; ``k`` the pattern length."""

    def __init__(self, names, ptype, rates, counts=None):
        self.names = list(names)
        self.ptype = np.asarray(ptype, np.uint32).reshape(-1)
        self.rates = np.asarray(rates, np.float64).reshape(-1)
        self.counts = [tuple(c) for c in counts] if counts is not None else [(0, 0)] * len(self.names)
        if not self.names:
            raise ValueError("a model without patterns")
        if not len(self.names) == self.ptype.shape[0] == self.rates.shape[0] == len(self.counts):
            raise ValueError("one type, rate and pair of counts per pattern")
        self.k = len(self.names[0])
        if any(len(x) != self.k for x in self.names):
            raise ValueError("patterns of different lengths")
        if np.any(self.ptype >= 12) or np.any(np.diff(self.ptype.astype(np.int64)) < 0):
            raise ValueError("the patterns must be grouped by type in id order")
        all_types = TYPES(False)
        self.types = [all_types[t] for t in sorted(set(self.ptype.tolist()))]

    @property
    def folded(self):
        """Every type has A or C as REF: the model can be used with strand folding."""
        return bool(np.all(self.ptype < 6))

    @classmethod
    def from_partitions(cls, parts):
        """``parts``: ``{type string: (names, counts, rates)}`` as ``apply.read_partition``
        returns them.  Types as written (not folded); a type may be given once."""
        names, ptype, rates, counts = [], [], [], []
        ids = {}
        for kind, part in parts.items():
            t = type_id(kind, fold=False)
            if t in ids:
                raise ValueError(f"type {kind} given twice")
            ids[t] = part
        for t in sorted(ids):
            pn, pc, pr = ids[t]
            names += list(pn)
            counts += list(pc)
            rates += list(pr)
            ptype += [t] * len(pn)
        return cls(names, ptype, rates, counts)

    @classmethod
    def read(cls, file):
        if isinstance(file, (str, os.PathLike)):
            with open(file) as f:
                return cls.read(f)
        if file.readline().split() != HEADER:
            raise ValueError(f"not a spectrum model: the first line must be '{' '.join(HEADER)}'")
        names, ptype, rates, counts = [], [], [], []
        for line in file:
            tok = line.split()
            if not tok:
                continue
            if len(tok) != 5:
                raise ValueError(f"bad line in the model file:\n{line.strip()}")
            ptype.append(type_id(tok[0], fold=False))
            names.append(tok[1])
            counts.append((int(tok[3]), int(tok[2])))
            rates.append(float(tok[4]))
        return cls(names, ptype, rates, counts)

    def write(self, file):
        if isinstance(file, (str, os.PathLike)):
            with open(file, "w") as f:
                return self.write(f)
        all_types = TYPES(False)
        file.write(" ".join(HEADER) + "\n")
        file.write("".join(f"{all_types[t]} {x} {u} {m} {float(r)!r}\n"
                           for t, x, (m, u), r in zip(self.ptype.tolist(), self.names, self.counts, self.rates.tolist())))

    def words(self):
        from .engine import pattern_word
        return [pattern_word(x) for x in self.names]


def _check_fold(model, fold):
    if not 1 <= model.k <= 15:
        raise ValueError("the patterns must be 1..15 positions long")
    if fold and model.k % 2 == 0:
        raise ValueError("strand folding needs an odd k (use --no-fold)")
    if fold and not model.folded:
        raise ValueError("the model has types with REF G or T: it was not fitted with strand folding (use --no-fold)")


@contextlib.contextmanager
def session(model, fold=True, host=False):
    """A kp_spec session of ``model``: yields the object whose ``spec_regions`` / ``spec_track`` /
    ``spec_sites`` / ``spec_stats`` run in it -- the first visible GPU's ``engine.Device``, or
    with ``host=True`` the host session."""
    from . import engine
    _check_fold(model, fold)
    s = engine.HostSpec() if host else engine.get_device(engine.visible_devices()[0])
    s.spec_begin(model.k, model.words(), model.ptype, fold)
    try:
        yield s
    finally:
        s.spec_end()


def count_genome(contigs, k, fold=True, regions=None, sites=None, host=False):
    """``count.count_genome`` for every mutation type at once.  ``sites``: ``{name: (pos0, alt)}``,
    ``alt`` the ALT bases as bytes.  Returns ``(pos_counts [3, 4^k], bg_counts [4^k], stats)``:
    column = slot of the (folded) ALT."""
    from . import engine

    def jobs():
        for name, seq in contigs:
            if regions is None:
                reg = None
            elif regions is False or name not in regions:
                reg = False
            else:
                reg = seqio.merge_regions(regions[name])
                reg = reg if reg.shape[0] else False
            st = sites.get(name) if sites is not None else None
            if reg is not False or (st is not None and len(st[0])):
                yield seq, reg, st

    s = engine.HostSpec() if host else engine.get_device(engine.visible_devices()[0])
    return s.seq_count_typed(k, fold, jobs())


def type_column(k, pos_counts, kind):
    """The dense positive column of one type: its slot's column at the k-mers with its REF in
    the centre, zero elsewhere."""
    ref, slot = BASES.index(kind[0]), slot_of(kind[0], kind[2])
    centre = (np.arange(4 ** k, dtype=np.uint64) >> np.uint64(2 * (k - 1 - k // 2))) & np.uint64(3)
    return np.where(centre == ref, pos_counts[slot], 0).astype(np.uint64)


def tables_of(k, fold, pos_counts, bg_counts):
    """``{type: KmerCounts}`` of typed counts: rows = the k-mers with the type's REF in the centre
    and a non-zero background, M the type's column, U = background - M (``count.table_of``'s
    ``ValueError`` where M > background)."""
    from .count import table_of
    out = {}
    for kind in TYPES(fold):
        col = type_column(k, pos_counts, kind)
        bg = type_column(k, np.stack([bg_counts] * 3), kind)
        out[kind] = table_of(k, col, bg)
    return out


def count_tables(contigs, k, fold=True, regions=None, sites=None, host=False):
    """:func:`count_genome` as one ``io_utils.KmerCounts`` per type (:func:`tables_of`)."""
    pos, bg, _ = count_genome(contigs, k, fold, regions, sites, host)
    return tables_of(k, fold, pos, bg)


def _contig_regions(s, seq, reg, P, rates, want_hist, budget):
    """One contig's regions in batches of at most ``budget`` counters a call."""
    m = reg.shape[0]
    step = max(1, int(budget) // max(P, 1))
    hist = np.zeros((m, P), np.uint64) if want_hist else None
    other = np.zeros((m, 4), np.uint64)
    exp = np.zeros((m, 12), np.float64)
    for b in range(0, m, step):
        h, o, e = s.spec_regions(seq, reg[b:b + step], rates, want_hist)
        other[b:b + step], exp[b:b + step] = o, e
        if want_hist:
            hist[b:b + step] = h
    return hist, other, exp


def region_rates(contigs, model, regions, fold=True, want_hist=False, host=False, budget=DEFAULT_BUDGET):
    """The model over regions of ``contigs`` (``predict.region_counts`` for every type at once).
    Returns ``{contig: (hist, other, expected)}``: ``hist`` uint64 ``[m, P]`` (None without
    ``want_hist``), ``other`` uint64 ``[m, 4]`` = positions without a pattern in slot 0, 1, 2 and
    positions without a valid window, ``expected`` float64 ``[m, 12]`` by type id.  Batching by
    ``budget`` counters a call changes no result."""
    out = {}
    with session(model, fold, host) as s:
        for name, seq in contigs:
            if name in regions:
                out[name] = _contig_regions(s, seq, _region_array(regions[name]), len(model.names), model.rates,
                                            want_hist, budget)
    return out


def track(seq_or_contigs, model, fold=True, host=False, begin=0, end=None):
    """The pattern index per ALT slot at every position: int32 ``[3, len]`` (``predict.track``'s
    codes per slot).  One contig (with ``begin`` / ``end`` a range of it) or an iterable of
    ``(name, array)`` giving a dict."""
    with session(model, fold, host) as s:
        if isinstance(seq_or_contigs, (np.ndarray, bytes, bytearray)):
            seq = np.frombuffer(seq_or_contigs, np.uint8) if not isinstance(seq_or_contigs, np.ndarray) else seq_or_contigs
            return s.spec_track(seq, begin, end)
        return {name: s.spec_track(seq) for name, seq in seq_or_contigs}


def site_rates(contigs, model, sites, fold=True, host=False):
    """The pattern of each site's own mutation type: ``sites`` is ``{contig: (pos0, alt)}``, the
    result ``{contig: int32 array}`` (-1 none, -2 no valid window, -3 ALT equals the centre base);
    ``predict.rates_of(pid, model.rates)`` gives the rates."""
    out = {}
    with session(model, fold, host) as s:
        for name, seq in contigs:
            if name in sites:
                out[name] = s.spec_sites(seq, *sites[name])
    return out


def simulate(contigs, model, seed, regions=None, scale=1.0, replicate=0, fold=True, host=False, stats=None):
    """A random mutation set drawn from ``model`` (``engine.Device.spec_simulate``): yields
    ``(name, pos, alt, pid)`` per contig in genome order -- 0-based positions ascending, the
    forward-strand ALT bases as upper-case ASCII and the pattern whose rate (times ``scale``)
    produced each hit.  A position mutates at most once, into each of its types with the
    probability of the type's pattern.  ``regions``: ``{name: [(begin, end), ...]}``; a contig's
    regions are merged into their union, a contig without regions draws nothing, None = every
    whole contig.  The draw depends on ``(seed, contig, position, replicate)`` and the model only,
    the contig by its 0-based index in genome order: a subset of regions or contigs changes no
    draw elsewhere, and another ``replicate`` gives an independent set.  A dict ``stats`` gets
    ``windows`` (valid windows inside the regions), ``hits`` and ``items`` added up."""
    with session(model, fold, host) as s:
        for contig_id, (name, seq) in enumerate(contigs):
            if regions is None:
                reg = np.array([(0, seq.shape[0])], np.uint64)
            else:
                reg = seqio.merge_regions(regions.get(name, np.zeros((0, 2), np.uint64)))
                if reg.shape[0] and int(reg[-1, 1]) > seq.shape[0]:
                    raise ValueError(f"a region of {name} ends past the contig's {seq.shape[0]} bases")
            pos, alt, pid = s.spec_simulate(seq, reg, model.rates, seed, contig_id, replicate, scale)
            if stats is not None:
                st = s.spec_sim_stats()
                for key in ("windows", "hits", "items"):
                    stats[key] = stats.get(key, 0) + st[key]
            yield name, pos, alt, pid


def _contig_null(s, seq, reg, rates, seed, contig_id, first, replicates, scale, by_type, budget, stats=None):
    """One contig's null table in batches of regions, and of replicates if need be, of at most
    ``budget`` counters a call."""
    m, nt = reg.shape[0], 12 if by_type else 1
    rep_step = max(1, min(int(replicates), int(budget) // nt))
    reg_step = max(1, int(budget) // (rep_step * nt))
    out = np.zeros((m, replicates, 12) if by_type else (m, replicates), np.uint32)
    for b in range(0, m, reg_step):
        for j in range(0, replicates, rep_step):
            n = min(rep_step, replicates - j)
            out[b:b + reg_step, j:j + n] = s.spec_null(seq, reg[b:b + reg_step], rates, seed, contig_id, first + j, n,
                                                       scale, by_type)
            if stats is not None:
                st = s.spec_null_stats()
                for key in ("windows", "draws", "hits", "items"):
                    stats[key] = stats.get(key, 0) + st[key]
    return out


def null_table(contigs, model, regions, seed, replicates, first=0, scale=1.0, by_type=False, fold=True, host=False,
               budget=DEFAULT_BUDGET, stats=None):
    """The null distribution of the mutation count per region (``engine.Device.spec_null``):
    ``{contig: table}``, ``table`` uint32 ``[m, replicates]`` (``[m, replicates, 12]`` by type id
    with ``by_type``).  Column ``j`` holds, per region of ``regions[contig]`` (``(begin, end)``
    pairs in any order, overlapping or not, nothing merged), the hits :func:`simulate` draws
    inside it with ``replicate = first + j`` and the same seed, scale and genome: the contig
    enters the draw by its 0-based index in genome order, exactly as there.  Batching by
    ``budget`` counters a call changes no result.  A dict ``stats`` gets ``windows``, ``draws``,
    ``hits`` and ``items`` added up over the calls."""
    replicates, first = int(replicates), int(first)
    if replicates < 1 or first < 0 or first + replicates > 1 << 32:
        raise ValueError("the replicates must be at least one and number below 2^32")
    out = {}
    with session(model, fold, host) as s:
        for contig_id, (name, seq) in enumerate(contigs):
            if name in regions:
                out[name] = _contig_null(s, seq, _region_array(regions[name]), model.rates, seed, contig_id, first,
                                         replicates, scale, by_type, budget, stats)
    return out


def null_summary(total, observed=None):
    """Per region of a null table ``total [m, R]``: a dict of lists ``mean`` (``S1 / R``), ``var``
    (the unbiased ``(R * S2 - S1 * S1) / (R * (R - 1))`` from integer sums, one division; nan for
    ``R == 1``), ``min`` and ``max``; with ``observed [m]`` also the empirical p-values that are
    never 0 (Phipson & Smyth): ``p_upper = (1 + #{j: sim_j >= obs}) / (R + 1)`` and ``p_lower``
    with ``<=``."""
    total = np.asarray(total)
    if total.ndim != 2 or total.shape[1] < 1:
        raise ValueError("a null table is [regions, replicates] with at least one replicate")
    m, R = total.shape
    out = {"mean": [], "var": [], "min": [], "max": []}
    if observed is not None:
        observed = np.asarray(observed).reshape(-1)
        if observed.shape[0] != m:
            raise ValueError("one observed count per region")
        out.update(p_upper=[], p_lower=[])
    for i in range(m):
        row = total[i].astype(np.uint64)
        top = int(row.max())
        S1 = int(row.sum()) if top * R < 1 << 64 else sum(row.tolist())
        S2 = int((row * row).sum()) if top * top * R < 1 << 64 else sum(x * x for x in row.tolist())
        out["mean"].append(S1 / R)
        out["var"].append((R * S2 - S1 * S1) / (R * (R - 1)) if R > 1 else float("nan"))
        out["min"].append(int(row.min()))
        out["max"].append(top)
        if observed is not None:
            obs = int(observed[i])
            out["p_upper"].append((1 + int((total[i] >= obs).sum())) / (R + 1))
            out["p_lower"].append((1 + int((total[i] <= obs).sum())) / (R + 1))
    return out


CLASSES = ["synonymous", "missense", "nonsense", "stop_lost", "splice"]
# the amino acid of codon 16 b0 + 4 b1 + b2 (ACGT digits), the standard genetic code
AMINO = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"


def codon_text(index):
    return BASES[index >> 4 & 3] + BASES[index >> 2 & 3] + BASES[index & 3]


def _usable(transcripts, lengths):
    """Per transcript: 0 usable, 1 its CDS length is no multiple of 3, 2 its contig is unknown."""
    return np.array([1 if t.length % 3 else (0 if t.contig in lengths else 2) for t in transcripts], np.int64)


def _contig_coding(s, seq, txs, splice, P, rates, budget):
    """One contig's transcripts in batches of at most ``budget`` counters a call."""
    m = len(txs)
    step = max(1, int(budget) // max(5 * P, 1))
    other = np.zeros((m, 8), np.uint64)
    exp = np.zeros((m, 5, 12), np.float64)
    for b in range(0, m, step):
        _, o, e = s.spec_coding(seq, [(t.strand, t.segments) for t in txs[b:b + step]], splice, rates, want_hist=False)
        other[b:b + step], exp[b:b + step] = o, e
    return other, exp


def coding_rates(contigs, model, transcripts, splice=2, scale=1.0, by_type=False, fold=True, host=False,
                 budget=DEFAULT_BUDGET):
    """Expected mutations per transcript by coding consequence (``engine.Device.spec_coding``).
    ``transcripts``: ``seqio.Transcript`` objects (``seqio.read_gtf_cds`` / ``read_cds_bed``).
    Returns a dict of arrays with one row per transcript, in their order: ``other`` uint64 ``[T,
    8]`` (the pairs of class synonymous, missense, nonsense, stop-lost and essential splice --
    the mutational opportunity --, the pairs with an invalid window, those without a pattern, the
    positions without a class), ``expected`` float64 ``[T, 5]`` = per class the sum of its twelve
    type sums in ascending type order, times ``scale``; with ``by_type`` also ``expected_by_type``
    ``[T, 5, 12]``, each type sum times ``scale``; ``status`` int64 ``[T]``: 0 computed, 1 skipped
    because the CDS length is no multiple of 3, 2 on a contig the genome does not have (their rows
    are zero).  Batching by ``budget`` counters a call changes no result."""
    transcripts = list(transcripts)
    T = len(transcripts)
    other = np.zeros((T, 8), np.uint64)
    exp = np.zeros((T, 5, 12), np.float64)
    per = {}
    for i, t in enumerate(transcripts):
        if t.length % 3 == 0:
            per.setdefault(t.contig, []).append(i)
    seen = set()
    with session(model, fold, host) as s:
        for name, seq in contigs:
            seen.add(name)
            if name in per:
                idx = np.array(per[name])
                o, e = _contig_coding(s, seq, [transcripts[i] for i in per[name]], splice, len(model.names), model.rates,
                                      budget)
                other[idx], exp[idx] = o, e
    total = np.zeros((T, 5), np.float64)
    for t in range(12):
        total = total + exp[:, :, t]
    out = {"other": other, "expected": total * float(scale), "status": _usable(transcripts, seen)}
    if by_type:
        out["expected_by_type"] = exp * float(scale)
    return out


def _contig_coding_null(s, seq, txs, rates, seed, contig_id, first, replicates, scale, splice, budget, stats=None):
    """One contig's table in batches of transcripts, and of replicates if need be, of at most
    ``budget`` counters a call."""
    m = len(txs)
    rep_step = max(1, min(int(replicates), int(budget) // 5))
    tx_step = max(1, int(budget) // (rep_step * 5))
    out = np.zeros((m, replicates, 5), np.uint32)
    for b in range(0, m, tx_step):
        table = [(t.strand, t.segments) for t in txs[b:b + tx_step]]
        for j in range(0, replicates, rep_step):
            n = min(rep_step, replicates - j)
            out[b:b + tx_step, j:j + n] = s.spec_coding_null(seq, table, rates, seed, contig_id, first + j, n, scale, splice)
            if stats is not None:
                st = s.spec_coding_null_stats()
                for key in ("hits", "unclassed") + (("positions", "drawing") if j == 0 else ()):
                    stats[key] = stats.get(key, 0) + st[key]
    return out


def coding_null_table(contigs, model, transcripts, seed, replicates, first=0, scale=1.0, splice=2, fold=True, host=False,
                      budget=DEFAULT_BUDGET, stats=None):
    """The null distribution of the mutation count per transcript and coding consequence
    (``engine.Device.spec_coding_null``): ``{"counts": uint32 [T, replicates, 5], "status": int64
    [T]}``, rows in the order of ``transcripts`` (``seqio.Transcript`` objects).  Column ``j``
    holds, per transcript and class (:data:`CLASSES`), the hits :func:`simulate` draws with
    ``replicate = first + j`` and the same seed, scale and genome, classed as
    :func:`coding_sites` classes them: the contig enters the draw by its 0-based index in genome
    order, exactly as there.  ``status`` as :func:`coding_rates`'; a skipped transcript's rows are
    zero.  Batching by ``budget`` counters a call changes no result.  A dict ``stats`` gets
    ``positions``, ``drawing``, ``hits`` and ``unclassed`` added up over the calls.  A contig whose
    sequence is None must hold no usable transcript."""
    replicates, first = int(replicates), int(first)
    if replicates < 1 or first < 0 or first + replicates > 1 << 32:
        raise ValueError("the replicates must be at least one and number below 2^32")
    transcripts = list(transcripts)
    counts = np.zeros((len(transcripts), replicates, 5), np.uint32)
    per = {}
    for i, t in enumerate(transcripts):
        if t.length % 3 == 0:
            per.setdefault(t.contig, []).append(i)
    seen = set()
    with session(model, fold, host) as s:
        for contig_id, (name, seq) in enumerate(contigs):
            seen.add(name)
            if name in per:
                counts[np.array(per[name])] = _contig_coding_null(s, seq, [transcripts[i] for i in per[name]], model.rates,
                                                                  seed, contig_id, first, replicates, scale, splice, budget,
                                                                  stats)
    return {"counts": counts, "status": _usable(transcripts, seen)}


def site_pairs(txs, pos):
    """The (site, transcript) pairs of one contig whose site lies inside the transcript's span
    (first CDS base to last), by interval search over the sorted positions: ``(site index,
    transcript index)`` arrays ordered by site, then transcript."""
    pos = np.asarray(pos, np.uint64)
    order = np.argsort(pos, kind="stable")
    ranked = pos[order]
    si, ti = [], []
    for j, t in enumerate(txs):
        if not t.segments:
            continue
        lo = np.searchsorted(ranked, np.uint64(t.segments[0][0]), "left")
        hi = np.searchsorted(ranked, np.uint64(t.segments[-1][1]), "left")
        si.append(order[lo:hi])
        ti.append(np.full(hi - lo, j, np.int64))
    si = np.concatenate(si) if si else np.zeros(0, np.int64)
    ti = np.concatenate(ti) if ti else np.zeros(0, np.int64)
    keep = np.lexsort((ti, si))
    return si[keep].astype(np.int64), ti[keep]


def coding_sites(s, seq, txs, pos, alt, splice=2):
    """The consequences of one contig's sites in its transcripts ``txs``, in the open session
    ``s``: ``(site index, transcript index, cls, pid, codons)`` of every pair whose site is a
    coding or essential splice position of the transcript (``engine.Device.spec_coding_sites``)."""
    si, ti = site_pairs(txs, pos)
    if not si.shape[0]:
        return si, ti, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint32)
    cls, pid, codons = s.spec_coding_sites(seq, [(t.strand, t.segments) for t in txs], np.asarray(pos, np.uint64)[si],
                                           np.asarray(alt, np.uint8)[si], ti, splice)
    keep = cls != -1
    return si[keep], ti[keep], cls[keep], pid[keep], codons[keep]


_CLASS = np.full(256, 4, np.uint8)
for _i, _b in enumerate(BASES):
    _CLASS[ord(_b)] = _CLASS[ord(_b.lower())] = _i


def folded_ref(seq, fold):
    """The REF code (0..3; 4 = no base) of every position on the counted strand."""
    ref = _CLASS[seq]
    return np.where(fold & (ref >= 2) & (ref < 4), 3 - ref, ref).astype(np.uint8)


def track_values(model, pid, ref, kind=None):
    """``(has, value)`` per position of a track ``pid [3, len]`` with ``ref`` =
    :func:`folded_ref` of the same positions: one type's rate, or by default the sum over the
    model's types with that REF in slot order (the module docstring's rule)."""
    rates = np.concatenate([model.rates, [0.0]])
    present = np.zeros((5, 3), bool)
    for t in set(model.ptype.tolist()):
        if kind is None or t == type_id(kind, fold=False):
            present[t // 3, t % 3] = True
    pres = present[ref].T  # [3, len]
    has = pres.any(axis=0) & np.all(~pres | (pid >= 0), axis=0)
    value = np.zeros(pid.shape[1], np.float64)
    for s in range(3):
        value = value + np.where(pres[s] & has, rates[np.where(pid[s] >= 0, pid[s], -1)], 0.0)
    return has, value


# ---------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------

def _type_file(prefix, kind):
    return f"{prefix}.{kind[0]}_{kind[2]}.txt"


def _matched_sites(path, report):
    """The sites file per contig (``seqio.read_sites_alt``), its line counts added to ``report``."""
    raw, st = seqio.read_sites_alt(path)
    report.update(st)
    report.update(off_contig=0, ref_mismatch=0)
    return raw


def _keep_matching(seq, pos, ref, alt, report):
    on = pos < np.uint64(seq.shape[0])
    same = np.zeros(pos.shape[0], bool)
    same[on] = (seq[pos[on].astype(np.intp)] & 0xDF) == ref[on]
    report["off_contig"] += int((~on).sum())
    report["ref_mismatch"] += int((on & ~same).sum())
    return pos[same], ref[same], alt[same]


def _run_count(args, k, fold, host, report):
    from .count import write_counts
    raw = _matched_sites(args.sites, report)
    regions = seqio.read_bed(args.bed) if args.bed else None
    seen, kept = set(), {}

    def contigs():
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            if name in raw:
                pos, ref, alt = _keep_matching(seq, *raw[name], report)
                kept[name] = (pos, alt)
            yield name, seq

    pos, bg, st = count_genome(contigs(), k, fold, regions=regions, sites=kept, host=host)
    report["unknown_contig"] = sum(len(v[0]) for name, v in raw.items() if name not in seen)
    if regions is not None:
        report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in seen)
    report.update(windows=st["windows"], windows_invalid=st["windows_invalid"], sites=st["sites"],
                  sites_skipped=st["sites_skipped"])
    with open(f"{args.output}.background.txt", "w") as out:
        write_counts(out, k, bg)
    written = {}  # type: (sites counted, background windows with its REF in the centre)
    for kind in TYPES(fold):
        col = type_column(k, pos, kind)
        if col.any():
            with open(_type_file(args.output, kind), "w") as out:
                write_counts(out, k, col)
            written[kind] = (int(col.sum()), int(type_column(k, np.stack([bg] * 3), kind).sum()))
    return written


def _run_join(pairs, output):
    parts = {}
    for item in pairs:
        kind, _, path = item.partition("=")
        if not path:
            raise ValueError(f"--type takes X>Y=PARTITION_FILE, not {item!r}")
        with open(path) as f:
            parts[kind.upper()] = read_partition(f)
        if not parts[kind.upper()][0]:
            raise ValueError(f"the partition file {path} holds no pattern")
    model = Model.from_partitions(parts)
    for t, x in zip(model.ptype.tolist(), model.names):
        if x[model.k // 2] != BASES[t // 3]:
            raise ValueError(f"pattern {x} of type {TYPES(False)[t]} does not have its REF base in the centre")
    model.write(output)
    return model


def _run_fit(args, k, fold, host, report):
    from . import cli
    tmp = None
    prefix = args.prefix
    if prefix is None:
        tmp = tempfile.TemporaryDirectory()
        prefix = os.path.join(tmp.name, "counts")
    try:
        args.output, model_path = prefix, args.output
        kinds = _run_count(args, k, fold, host, report)
        if not kinds:
            raise ValueError("no site was counted")
        pairs = []
        for kind in kinds:
            part = f"{prefix}.{kind[0]}_{kind[2]}.partition.txt"
            argv = ["-p", _type_file(prefix, kind), "-b", f"{prefix}.background.txt", "-s", super_pattern(kind, k),
                    "-o", part, "--verbosity", str(args.verbosity)]
            if args.penalty_values:
                argv += ["-c"] + [repr(x) for x in args.penalty_values]
            if args.pseudo_counts:
                argv += ["-a"] + [repr(x) for x in args.pseudo_counts]
            if args.nfolds is not None:
                argv += ["-N", str(args.nfolds)]
            if args.seed is not None:
                argv += ["--seed", str(args.seed)]
            argv += ["--greedy"] * args.greedy + ["--greedyCV"] * args.greedyCV
            rc = cli.main(argv)
            gc.collect()  # (cli.main leaves its output file to be closed with its argparse namespace)
            if rc:
                raise ValueError(f"the fit of {kind} failed with exit code {rc}")
            pairs.append(f"{kind}={part}")
        model = _run_join(pairs, model_path)
        # a partition file read before it was written out in full would be short: every type's
        # pattern counts must add up to the count files the fit read
        for kind, (n_pos, n_bg) in kinds.items():
            own = [c for c, t in zip(model.counts, model.ptype.tolist()) if t == type_id(kind, fold=False)]
            got = (sum(m for m, _ in own), sum(m + u for m, u in own))
            if got != (n_pos, n_bg):
                raise RuntimeError(f"the partition of {kind} holds {got[0]} sites in {got[1]} windows, its count files "
                                   f"{n_pos} in {n_bg}: the partition file is incomplete")
        report["types"] = len(model.types)
        report["patterns"] = len(model.names)
    finally:
        if tmp is not None:
            tmp.cleanup()


def _observed(path, genome_contigs, model, fold, report):
    """Per contig ``{type id: sorted positions}`` of the sites whose REF matches the genome, for
    the model's types; the sites of other types are counted in ``report["observed_other_type"]``."""
    raw = _matched_sites(path, report)
    out = {}
    ids = np.array([[3 * r + (a if a < r else a - 1) if a != r else 0 for a in range(4)] for r in range(4)])
    for name, seq in genome_contigs.items():
        if name not in raw:
            continue
        pos, ref, alt = _keep_matching(seq, *raw[name], report)
        r, a = _CLASS[ref].astype(np.int64), _CLASS[alt].astype(np.int64)
        if fold:
            flip = r >= 2
            r, a = np.where(flip, 3 - r, r), np.where(flip, 3 - a, a)
        t = ids[r, a]
        out[name] = {int(x): np.sort(pos[t == x]) for x in set(model.ptype.tolist())}
        report["observed_other_type"] = report.get("observed_other_type", 0) + int((~np.isin(t, model.ptype)).sum())
    report["unknown_contig"] = sum(len(v[0]) for name, v in raw.items() if name not in genome_contigs)
    return out


def _run_regions(args, model, fold, host, report, out):
    rows = _bed_lines(args.bed)
    per = _by_contig(rows)
    n = len(rows)
    tids = sorted(set(model.ptype.tolist()))
    other = np.zeros((n, 4), np.uint64)
    exp = np.zeros((n, 12), np.float64)
    obs = np.zeros((n, 12), np.int64)
    seen = {}
    with session(model, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            if name in per:
                seen[name] = seq
                idx = np.array(per[name])
                reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
                _, o, e = _contig_regions(s, seq, reg, len(model.names), model.rates, False, DEFAULT_BUDGET)
                other[idx], exp[idx] = o, e
        st = s.spec_stats()
    report.update(assigned=st["assigned"], unmatched=st["unmatched"], invalid=st["invalid"],
                  unknown_contig_regions=sum(len(v) for name, v in per.items() if name not in seen))
    if args.observed:
        sites = _observed(args.observed, seen, model, fold, report)
        for name, by_type in sites.items():
            idx = np.array(per[name])
            reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
            for t, pos in by_type.items():
                obs[idx, t] = np.searchsorted(pos, reg[:, 1], "left") - np.searchsorted(pos, reg[:, 0], "left")
    labelled = any(row[3] is not None for row in rows)
    kinds = [TYPES(False)[t] for t in tids]
    head = ["#chrom", "start", "end"] + ["name"] * labelled + ["valid", "invalid", "exp_total"] + [f"exp_{x}" for x in kinds]
    if args.observed:
        head += ["obs_total"] + [f"obs_{x}" for x in kinds]
    lines = [" ".join(head) + "\n"]
    for i, (chrom, b, e, label) in enumerate(rows):
        known = chrom in seen
        inv = int(other[i, 3])
        tok = [chrom, str(b), str(e)] + [label if label is not None else "."] * labelled
        tok += [str(e - b - inv if known else 0), str(inv)]
        total = 0.0
        for t in tids:
            total = total + float(exp[i, t])
        tok += [repr(total)] + [repr(float(exp[i, t])) for t in tids]
        if args.observed:
            tok += [str(int(obs[i, tids].sum()))] + [str(int(obs[i, t])) for t in tids]
        lines.append(" ".join(tok) + "\n")
    out.write("".join(lines))


def _run_track(args, model, fold, host, report, out):
    regions = seqio.read_bed(args.bed) if args.bed else None
    kind = None
    if args.type:
        kind = TYPES(False)[type_id(args.type, fold)]
        if kind not in model.types:
            raise ValueError(f"the model has no type {kind}")
    seen = set()
    positions = 0
    with session(model, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            if regions is None:
                ranges = [(0, seq.shape[0])]
            else:
                ranges = regions.get(name, np.zeros((0, 2), np.uint64)).tolist()
            for b, e in ranges:
                if e > seq.shape[0]:
                    raise ValueError(f"region {name} {b} {e} ends past the contig's {seq.shape[0]} bases")
                pid = s.spec_track(seq, b, e)
                if not pid.shape[1]:
                    continue
                has, value = track_values(model, pid, folded_ref(seq[b:e], fold), kind)
                key = np.where(has, value.view(np.int64), -1)
                first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))  # where a run starts
                last = np.concatenate([first[1:], [key.shape[0]]])
                keep = has[first]
                positions += int((last - first)[keep].sum())
                out.write("".join(f"{name} {b + x} {b + y} {v!r}\n" for x, y, v in
                                  zip(first[keep].tolist(), last[keep].tolist(), value[first][keep].tolist())))
    report["positions_with_a_rate"] = positions
    if regions is not None:
        report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in seen)


def _run_sites(args, model, fold, host, report, out):
    rows, skipped = _site_lines(args.sites)
    per = _by_contig(rows)
    pid = np.full(len(rows), -4, np.int32)  # -4: not looked up
    report.update(lines=len(rows) + skipped, not_snv=skipped, off_contig=0, ref_mismatch=0)
    seen = set()
    with session(model, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            if name in per:
                seen.add(name)
                idx = np.array(per[name])
                pos = np.array([rows[i][1] - 1 for i in per[name]], np.uint64)
                ref = np.array([ord(rows[i][2].upper()) for i in per[name]], np.uint8)
                alt = np.array([ord(rows[i][3].upper()) for i in per[name]], np.uint8)
                on = pos < np.uint64(seq.shape[0])
                same = np.zeros(pos.shape[0], bool)
                same[on] = (seq[pos[on].astype(np.intp)] & 0xDF) == ref[on]
                report["off_contig"] += int((~on).sum())
                report["ref_mismatch"] += int((on & ~same).sum())
                pid[idx[same]] = s.spec_sites(seq, pos[same], alt[same])
    report["unknown_contig"] = sum(len(v) for name, v in per.items() if name not in seen)
    report["without_pattern"] = int(((pid == -1) | (pid == -2)).sum())
    kinds = TYPES(False)
    rates = model.rates.tolist()
    out.write("".join(f"{c} {p} {r} {a} " + (f"{kinds[int(model.ptype[j])]} {model.names[j]} {rates[j]!r}\n" if j >= 0
                                             else "NA NA NA\n")
                      for (c, p, r, a), j in zip(rows, pid.tolist())))


def _run_simulate(args, model, fold, host, report, out):
    regions = seqio.read_bed(args.bed) if args.bed else None
    if not 0 <= args.seed < 1 << 64 or not 0 <= args.replicate < 1 << 32:
        raise ValueError("--seed must be an unsigned 64-bit and --replicate an unsigned 32-bit integer")
    seen, seqs = set(), {}

    def contigs():
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            seqs[name] = seq
            yield name, seq

    stats = {"windows": 0, "hits": 0}
    per_type = np.zeros(12, np.int64)
    for name, pos, alt, pid in simulate(contigs(), model, args.seed, regions, args.scale, args.replicate, fold, host, stats):
        ref = seqs.pop(name)[pos.astype(np.intp)] & 0xDF
        per_type += np.bincount(model.ptype[pid], minlength=12)
        out.write("".join(f"{name} {p + 1} {chr(r)} {chr(a)}\n" for p, r, a in zip(pos.tolist(), ref.tolist(), alt.tolist())))
    report.update(windows=stats["windows"], hits=stats["hits"])
    kinds = TYPES(False)
    for t in sorted(set(model.ptype.tolist())):
        report[f"hits_{kinds[t]}"] = int(per_type[t])
    if regions is not None:
        report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in seen)


def _run_null(args, model, fold, host, report, out):
    rows = _bed_lines(args.bed)
    per = _by_contig(rows)
    n, R, first = len(rows), args.replicates, args.first_replicate
    if not 0 <= args.seed < 1 << 64:
        raise ValueError("--seed must be an unsigned 64-bit integer")
    if R < 1 or first < 0 or first + R > 1 << 32:
        raise ValueError("--replicates must be at least 1, and --first-replicate + --replicates at most 2^32")
    tids = sorted(set(model.ptype.tolist()))
    kinds = [TYPES(False)[t] for t in tids]
    cols = ["total"] + (kinds if args.by_type else [])  # a summary per column and BED line
    other = np.zeros((n, 4), np.uint64)
    exp = np.zeros((n, 12), np.float64)
    obs = np.zeros((n, 12), np.int64)
    tables, seen = {}, {}
    stats = {"windows": 0, "draws": 0, "hits": 0}
    with session(model, fold, host) as s:
        for contig_id, (name, seq) in enumerate(seqio.read_genome(args.genome)):
            if name in per:
                seen[name] = seq
                idx = np.array(per[name])
                reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
                _, o, e = _contig_regions(s, seq, reg, len(model.names), model.rates, False, DEFAULT_BUDGET)
                other[idx], exp[idx] = o, e
                tables[name] = _contig_null(s, seq, reg, model.rates, args.seed, contig_id, first, R, args.scale,
                                            args.by_type, DEFAULT_BUDGET, stats)
        st = s.spec_stats()
    report.update(assigned=st["assigned"], unmatched=st["unmatched"], invalid=st["invalid"], windows=stats["windows"],
                  draws=stats["draws"], hits=stats["hits"],
                  unknown_contig_regions=sum(len(v) for name, v in per.items() if name not in seen))
    if args.observed:
        sites = _observed(args.observed, seen, model, fold, report)
        for name, by_type in sites.items():
            idx = np.array(per[name])
            reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
            for t, pos in by_type.items():
                obs[idx, t] = np.searchsorted(pos, reg[:, 1], "left") - np.searchsorted(pos, reg[:, 0], "left")
    obs_total = obs[:, tids].sum(axis=1)
    summary = [[None] * len(cols) for _ in range(n)]  # per BED line and column: (mean, var, min, max[, p_upper, p_lower])
    draws = ["0" + " 0" * (R - 1) + "\n"] * n
    for name, idx in per.items():
        if name not in tables:
            tab = np.zeros((len(idx), R, 12) if args.by_type else (len(idx), R), np.uint32)
        else:
            tab = tables.pop(name)
        total = tab.sum(axis=2, dtype=np.uint32) if args.by_type else tab  # (a region's count is below 2^32)
        for c, col in enumerate(cols):
            t = None if c == 0 else tids[c - 1]
            one = total if t is None else tab[:, :, t]
            ob = None if not args.observed else (obs_total[idx] if t is None else obs[idx, t])
            sm = null_summary(one, ob)
            keys = ["mean", "var", "min", "max"] + (["p_upper", "p_lower"] if args.observed else [])
            for x, i in enumerate(idx):
                summary[i][c] = [sm[key][x] for key in keys]
        if args.draws and name in seen:
            for x, i in enumerate(idx):
                draws[i] = " ".join(map(str, total[x].tolist())) + "\n"
    labelled = any(row[3] is not None for row in rows)
    head = ["#chrom", "start", "end"] + ["name"] * labelled + ["valid", "invalid", "exp_total"]
    for c, col in enumerate(cols):
        tail = "" if c == 0 else "_" + col
        head += [f"sim_mean{tail}", f"sim_var{tail}", f"sim_min{tail}", f"sim_max{tail}"]
        if args.observed:
            head += [f"obs_{col}", f"p_upper{tail}", f"p_lower{tail}"]
    lines = [" ".join(head) + "\n"]
    for i, (chrom, b, e, label) in enumerate(rows):
        inv = int(other[i, 3])
        tok = [chrom, str(b), str(e)] + [label if label is not None else "."] * labelled
        tok += [str(e - b - inv if chrom in seen else 0), str(inv)]
        total = 0.0
        for t in tids:
            total = total + float(exp[i, t])
        tok += [repr(total * float(args.scale))]
        for c in range(len(cols)):
            v = summary[i][c]
            tok += [repr(float(v[0])), repr(float(v[1])), str(v[2]), str(v[3])]
            if args.observed:
                tok += [str(int(obs_total[i] if c == 0 else obs[i, tids[c - 1]])), repr(float(v[4])), repr(float(v[5]))]
        lines.append(" ".join(tok) + "\n")
    out.write("".join(lines))
    if args.draws:
        with open(args.draws, "w") as f:
            f.write("".join(draws))


def _read_transcripts(args):
    return seqio.read_gtf_cds(args.gtf) if args.gtf else seqio.read_cds_bed(args.cds_bed)


def _check_splice(splice):
    if not 0 <= splice <= 8:
        raise ValueError("--splice must be 0..8")


def _coding_observed(args, model, fold, host, report, txs, status, seqs):
    """int64 ``[T, 5]``: the sites of ``args.observed`` per usable transcript and class (``cls >=
    0``); ``seqs``: every contig of the genome by name."""
    obs = np.zeros((len(txs), 5), np.int64)
    raw = _matched_sites(args.observed, report)
    per = {}
    for i, t in enumerate(txs):
        if status[i] == 0:
            per.setdefault(t.contig, []).append(i)
    outside = 0
    with session(model, fold, host) as s:
        for name, seq in seqs.items():
            if name not in raw:
                continue
            pos, ref, alt = _keep_matching(seq, *raw[name], report)
            own = [txs[i] for i in per.get(name, [])]
            si, ti, cls, _, _ = coding_sites(s, seq, own, pos, alt, args.splice)
            hit = cls >= 0
            np.add.at(obs, (np.array(per.get(name, []), np.int64)[ti[hit]], cls[hit]), 1)
            outside += pos.shape[0] - np.unique(si).shape[0]
    report["unknown_contig"] = sum(len(v[0]) for name, v in raw.items() if name not in seqs)
    report["observed_outside"] = outside
    return obs


def _run_coding(args, model, fold, host, report, out):
    _check_splice(args.splice)
    txs = _read_transcripts(args)
    T = len(txs)
    seqs = {}

    def contigs():
        for name, seq in seqio.read_genome(args.genome):
            if args.observed:
                seqs[name] = seq
            yield name, seq

    res = coding_rates(contigs(), model, txs, args.splice, args.scale, args.by_type, fold, host)
    status, other, exp = res["status"], res["other"], res["expected"]
    report.update(transcripts=T, skipped_length=int((status == 1).sum()), unknown_contig_transcripts=int((status == 2).sum()))
    obs = _coding_observed(args, model, fold, host, report, txs, status, seqs) if args.observed else np.zeros((T, 5), np.int64)
    tids = sorted(set(model.ptype.tolist()))
    kinds = [TYPES(False)[t] for t in tids]
    head = ["#name", "gene", "contig", "strand", "cds_bases"] + [f"opp_{c}" for c in CLASSES] + [f"exp_{c}" for c in CLASSES]
    head += ["unrated", "no_class"]
    if args.observed:
        head += [f"obs_{c}" for c in CLASSES]
    if args.by_type:
        head += [f"exp_{c}_{x}" for c in CLASSES for x in kinds]
    lines = [" ".join(head) + "\n"]
    for i, t in enumerate(txs):
        tok = [t.name, t.gene if t.gene is not None else ".", t.contig, "+-"[t.strand], str(t.length)]
        tok += [str(int(x)) for x in other[i, :5]] + [repr(float(x)) for x in exp[i]]
        tok += [str(int(other[i, 5] + other[i, 6])), str(int(other[i, 7]))]
        if args.observed:
            tok += [str(int(x)) for x in obs[i]]
        if args.by_type:
            tok += [repr(float(res["expected_by_type"][i, c, ty])) for c in range(5) for ty in tids]
        lines.append(" ".join(tok) + "\n")
    out.write("".join(lines))


def _run_coding_null(args, model, fold, host, report, out):
    _check_splice(args.splice)
    R, first = args.replicates, args.first_replicate
    if not 0 <= args.seed < 1 << 64:
        raise ValueError("--seed must be an unsigned 64-bit integer")
    if R < 1 or first < 0 or first + R > 1 << 32:
        raise ValueError("--replicates must be at least 1, and --first-replicate + --replicates at most 2^32")
    txs = _read_transcripts(args)
    T = len(txs)
    wanted = {t.contig for t in txs if t.length % 3 == 0}
    seqs = {}  # every contig in genome order; the sequence of those a later step reads

    def contigs():
        for name, seq in seqio.read_genome(args.genome):
            seqs[name] = seq if args.observed or name in wanted else None
            yield name, seq

    res = coding_rates(contigs(), model, txs, args.splice, args.scale, False, fold, host)
    status, other, exp = res["status"], res["other"], res["expected"]
    stats = {"positions": 0, "drawing": 0, "hits": 0, "unclassed": 0}
    tab = coding_null_table(seqs.items(), model, txs, args.seed, R, first, args.scale, args.splice, fold, host,
                            stats=stats)["counts"]
    report.update(transcripts=T, skipped_length=int((status == 1).sum()), unknown_contig_transcripts=int((status == 2).sum()),
                  **stats)
    obs = _coding_observed(args, model, fold, host, report, txs, status, seqs) if args.observed else None
    # a summary per column: the five classes, then all of them and nonsense + essential splice, summed per replicate
    cols = CLASSES + ["total", "lof"]
    sims = [tab[:, :, c] for c in range(5)] + [tab.sum(axis=2, dtype=np.uint32), tab[:, :, 2] + tab[:, :, 4]]
    keys = ["mean", "var", "min", "max"] + (["p_upper", "p_lower"] if args.observed else [])
    obs_cols, summary = [], []
    for c, one in enumerate(sims):
        ob = None
        if args.observed:
            ob = obs[:, c] if c < 5 else (obs.sum(axis=1) if c == 5 else obs[:, 2] + obs[:, 4])
        obs_cols.append(ob)
        summary.append(null_summary(one, ob) if T else {key: [] for key in keys})
    head = ["#name", "gene", "contig", "strand", "cds_bases"] + [f"opp_{c}" for c in CLASSES] + [f"exp_{c}" for c in CLASSES]
    for col in cols:
        head += [f"sim_mean_{col}", f"sim_var_{col}", f"sim_min_{col}", f"sim_max_{col}"]
        if args.observed:
            head += [f"obs_{col}", f"p_upper_{col}", f"p_lower_{col}"]
    lines = [" ".join(head) + "\n"]
    for i, t in enumerate(txs):
        tok = [t.name, t.gene if t.gene is not None else ".", t.contig, "+-"[t.strand], str(t.length)]
        tok += [str(int(x)) for x in other[i, :5]] + [repr(float(x)) for x in exp[i]]
        for c in range(len(cols)):
            sm = summary[c]
            tok += [repr(float(sm["mean"][i])), repr(float(sm["var"][i])), str(sm["min"][i]), str(sm["max"][i])]
            if args.observed:
                tok += [str(int(obs_cols[c][i])), repr(float(sm["p_upper"][i])), repr(float(sm["p_lower"][i]))]
        lines.append(" ".join(tok) + "\n")
    out.write("".join(lines))
    if args.draws:
        with open(args.draws, "w") as f:
            f.write("".join(f"{t.name} {CLASSES[c]} " + " ".join(map(str, tab[i, :, c].tolist())) + "\n"
                            for i, t in enumerate(txs) for c in range(5)))


def _run_consequences(args, model, fold, host, report, out):
    _check_splice(args.splice)
    txs = _read_transcripts(args)
    rows, skipped = _site_lines(args.sites)
    per_rows = _by_contig(rows)
    report.update(transcripts=len(txs), skipped_length=sum(1 for t in txs if t.length % 3), lines=len(rows) + skipped,
                  not_snv=skipped, off_contig=0, ref_mismatch=0)
    per = {}
    for t in txs:
        if t.length % 3 == 0:
            per.setdefault(t.contig, []).append(t)
    seen = set()
    kinds = TYPES(False)
    rates = model.rates.tolist()
    found = [[] for _ in rows]  # per site: its lines, transcripts in input order
    with session(model, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            if name not in per_rows:
                continue
            idx = np.array(per_rows[name])
            pos = np.array([rows[i][1] - 1 for i in per_rows[name]], np.uint64)
            ref = np.array([ord(rows[i][2].upper()) for i in per_rows[name]], np.uint8)
            alt = np.array([ord(rows[i][3].upper()) for i in per_rows[name]], np.uint8)
            on = pos < np.uint64(seq.shape[0])
            same = np.zeros(pos.shape[0], bool)
            same[on] = (seq[pos[on].astype(np.intp)] & 0xDF) == ref[on]
            report["off_contig"] += int((~on).sum())
            report["ref_mismatch"] += int((on & ~same).sum())
            idx, pos, alt = idx[same], pos[same], alt[same]
            own = per.get(name, [])
            for i, j, c, p, cod in zip(*[x.tolist() for x in coding_sites(s, seq, own, pos, alt, args.splice)]):
                model_part = f"{kinds[int(model.ptype[p])]} {model.names[p]} {rates[p]!r}" if p >= 0 else "NA NA NA"
                if 0 <= c <= 3:
                    rc, ac = cod & 63, cod >> 6 & 63
                    tail = f"{CLASSES[c]} {codon_text(rc)} {codon_text(ac)} {AMINO[rc]} {AMINO[ac]}"
                else:
                    tail = (CLASSES[4] if c == 4 else "NA") + " NA NA NA NA"
                chrom, p1, r, a = rows[int(idx[i])]
                found[int(idx[i])].append(f"{chrom} {p1} {r} {a} {model_part} {own[j].name} {tail}\n")
    report["unknown_contig"] = sum(len(v) for name, v in per_rows.items() if name not in seen)
    report["unknown_contig_transcripts"] = sum(1 for t in txs if t.contig not in seen)
    report["sites_outside"] = sum(1 for x in found if not x)
    out.write("".join(line for lines in found for line in lines))


def get_parser():
    p = argparse.ArgumentParser(prog="kmerpapa-spectrum",
                                description="Counts, fits and applies one k-mer pattern partition per mutation type "
                                            "in one pass over the genome")
    sub = p.add_subparsers(dest="command", required=True)

    def common(q, output_help, default=None):
        q.add_argument("--no-fold", action="store_true",
                       help="Take every window as read (12 types); default: a window with G or T in the centre is "
                            "taken as its reverse complement and ALT is complemented with it (6 types)")
        q.add_argument("-o", "--output", metavar="PATH", help=output_help, default=default, required=default is None)
        q.add_argument("--verbosity", type=int, default=1,
                       help="Amount of info printed to stderr during execution. 0:silent, 1:default")

    def counting(q):
        q.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
        q.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
        size = q.add_mutually_exclusive_group(required=True)
        size.add_argument("-k", type=int, help="Length of the k-mers (1..15; odd unless --no-fold)")
        size.add_argument("--radius", type=int, help="Bases on each side of the centre: k = 2 * radius + 1")
        q.add_argument("--bed", metavar="FILE", help="Count the background only where the centre lies in these regions")

    cnt = sub.add_parser("count", help="background counts and the counts of every mutation type's sites, in one session")
    counting(cnt)
    common(cnt, "Prefix of PREFIX.background.txt and one PREFIX.X_Y.txt per type that has sites")
    joi = sub.add_parser("join", help="per-type partition files into one model file")
    joi.add_argument("--type", action="append", required=True, metavar="X>Y=FILE",
                     help="A type and the output table of kmerpapa (short or -l format) fitted for it; repeat per type")
    joi.add_argument("-o", "--output", required=True, metavar="MODEL", help="The model file")
    joi.add_argument("--verbosity", type=int, default=1)
    fit = sub.add_parser("fit", help="count, fit every type that has sites with kmerpapa's options, and join")
    counting(fit)
    common(fit, "The model file")
    fit.add_argument("--prefix", metavar="PREFIX", help="Keep the count and partition files under this prefix")
    fit.add_argument("-c", "--penalty_values", type=float, nargs="+", metavar="c")
    fit.add_argument("-a", "--pseudo_counts", type=float, nargs="+", metavar="a")
    fit.add_argument("-N", "--nfolds", type=int, metavar="N")
    fit.add_argument("--seed", type=int)
    fit.add_argument("--greedy", action="store_true")
    fit.add_argument("--greedyCV", action="store_true")

    def applying(q):
        q.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
        q.add_argument("--model", required=True, metavar="FILE", help="Model file of `join` or `fit`")
        common(q, "Output file (default: standard output)", "-")

    reg = sub.add_parser("regions", help="per region: expected mutations by type and in total, and the observed ones")
    applying(reg)
    reg.add_argument("--bed", metavar="FILE", required=True, help="The regions; a 4th column is carried through as a name")
    reg.add_argument("--observed", metavar="SITES", help="CHROM POS REF ALT lines to count per region and type.  Only sites of the model's types are "
                          "counted (obs_total is their sum); the number of the others is reported on stderr as "
                          "observed_other_type")
    trk = sub.add_parser("track", help="the rate at every position, as bedGraph")
    applying(trk)
    trk.add_argument("--bed", metavar="FILE", help="Only the positions of these regions")
    trk.add_argument("--type", metavar="X>Y",
                     help="This type's rate.  Default: the sum of the rates of the model's types with the position's "
                          "REF base, in slot order; a position where one of them has no pattern gets no value")
    sit = sub.add_parser("sites", help="the type, pattern and rate of given mutations")
    applying(sit)
    sit.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    sim = sub.add_parser("simulate", help="a random mutation set drawn from the model, as CHROM POS REF ALT lines")
    applying(sim)
    sim.add_argument("--seed", type=int, required=True,
                     help="Seed of the draw (0 .. 2^64 - 1): the same seed, replicate, genome and model give the same set")
    sim.add_argument("--replicate", type=int, default=0, metavar="R",
                     help="Number of the set (default 0): every replicate of a seed is an independent draw")
    sim.add_argument("--scale", type=float, default=1.0, metavar="X", help="Multiply every rate by X (default 1)")
    sim.add_argument("--bed", metavar="FILE", help="Only the positions of these regions (their union); the draws "
                                                   "inside them are those of a whole-genome run")
    nul = sub.add_parser("null", help="per region: the null distribution of the mutation count over many simulated "
                                      "sets, and the empirical p-values of the observed count")
    applying(nul)
    nul.add_argument("--bed", metavar="FILE", required=True, help="The regions; a 4th column is carried through as a name")
    nul.add_argument("--replicates", type=int, required=True, metavar="R", help="Number of simulated sets")
    nul.add_argument("--seed", type=int, required=True,
                     help="Seed of the draws (0 .. 2^64 - 1): set j is `simulate --seed SEED --replicate F+j`")
    nul.add_argument("--first-replicate", type=int, default=0, metavar="F", help="Number of the first set (default 0)")
    nul.add_argument("--scale", type=float, default=1.0, metavar="X", help="Multiply every rate by X (default 1)")
    nul.add_argument("--observed", metavar="SITES",
                     help="CHROM POS REF ALT lines to count per region as `regions --observed` does; adds obs_total "
                          "and the empirical p_upper = (1 + #{sim >= obs}) / (R + 1) and p_lower (with <=)")
    nul.add_argument("--by-type", action="store_true", help="The same columns per mutation type of the model as well")
    nul.add_argument("--draws", metavar="FILE", help="Write the raw totals: one line per region, R integers")

    def annotated(q):
        src = q.add_mutually_exclusive_group(required=True)
        src.add_argument("--gtf", metavar="FILE", help="The transcripts: the CDS lines of a GTF file, grouped by transcript_id")
        src.add_argument("--cds-bed", metavar="FILE",
                         help="The transcripts: BED6 lines, one per CDS segment, column 4 the transcript, column 6 the strand")
        q.add_argument("--splice", type=int, default=2, metavar="N",
                       help="Intronic bases at each end of an intron that are essential splice positions (0..8, default 2)")

    cod = sub.add_parser("coding", help="per transcript: expected, possible and observed mutations by coding consequence")
    applying(cod)
    annotated(cod)
    cod.add_argument("--scale", type=float, default=1.0, metavar="X", help="Multiply every expected count by X (default 1)")
    cod.add_argument("--observed", metavar="SITES", help="CHROM POS REF ALT lines to count per transcript and class")
    cod.add_argument("--by-type", action="store_true", help="The expected counts per class and mutation type of the model as well")
    cnu = sub.add_parser("coding-null", help="per transcript and coding consequence: the null distribution of the "
                                             "mutation count over many simulated sets, and empirical p-values")
    applying(cnu)
    annotated(cnu)
    cnu.add_argument("--replicates", type=int, required=True, metavar="R", help="Number of simulated sets")
    cnu.add_argument("--seed", type=int, required=True,
                     help="Seed of the draws (0 .. 2^64 - 1): set j is `simulate --seed SEED --replicate F+j`")
    cnu.add_argument("--first-replicate", type=int, default=0, metavar="F", help="Number of the first set (default 0)")
    cnu.add_argument("--scale", type=float, default=1.0, metavar="X", help="Multiply every rate by X (default 1)")
    cnu.add_argument("--observed", metavar="SITES",
                     help="CHROM POS REF ALT lines to count per transcript and class as `coding --observed` does; adds "
                          "obs_* and the empirical p_upper = (1 + #{sim >= obs}) / (R + 1) and p_lower (with <=)")
    cnu.add_argument("--draws", metavar="FILE", help="Write the raw counts: one line per transcript and class, R integers")
    con = sub.add_parser("consequences", help="the class, codons and amino acids of given mutations, per transcript")
    applying(con)
    annotated(con)
    con.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    return p


def _overlap_report(model):
    """Pairs of patterns of one type that share k-mers."""
    from .apply import lca_pattern
    from .engine import apply_host, pattern_word
    pairs = 0
    for t in sorted(set(model.ptype.tolist())):
        names = [x for x, y in zip(model.names, model.ptype.tolist()) if y == t]
        pairs += apply_host(model.k, [pattern_word(x) for x in names], pattern_word(lca_pattern(names)), [], [], [])[4][
            "overlap_pairs"]
    return pairs


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 1 with a message if a type's patterns overlap; 2 on input
    errors."""
    import io

    from .engine import KPError
    args = get_parser().parse_args(args=argv)
    report = {}
    buf = io.StringIO()
    try:
        if args.command == "join":
            _run_join(args.type, args.output)
            return 0
        fold = not args.no_fold
        seqio.is_2bit(args.genome)  # (a genome that cannot be opened is reported before a GPU is touched)
        if args.command in ("count", "fit"):
            k = args.k if args.k is not None else 2 * args.radius + 1
            if not 1 <= k <= 15:
                raise ValueError("k must be 1..15")
            if fold and k % 2 == 0:
                raise ValueError("strand folding needs an odd k (use --no-fold)")
            (_run_count if args.command == "count" else _run_fit)(args, k, fold, host, report)
        else:
            model = Model.read(args.model)
            _check_fold(model, fold)
            run = {"regions": _run_regions, "track": _run_track, "sites": _run_sites, "simulate": _run_simulate,
                   "null": _run_null, "coding": _run_coding, "coding-null": _run_coding_null,
                   "consequences": _run_consequences}[args.command]
            streamed = args.command in ("track", "simulate")  # (written contig by contig)
            try:
                if streamed and args.output != "-":
                    with open(args.output, "w") as out:
                        run(args, model, fold, host, report, out)
                else:
                    run(args, model, fold, host, report, sys.stdout if streamed else buf)
            except KPError as e:
                if e.code == -1 and "not a partition" in str(e):
                    print(f"kmerpapa-spectrum: a type's patterns are not a partition: {_overlap_report(model)} pairs of "
                          "patterns share k-mers", file=sys.stderr)
                    return 1
                raise
    except (ValueError, OSError, KeyError, KPError) as e:
        if isinstance(e, KPError) and e.code != -1:  # only KP_E_ARG is the input's fault
            raise
        print(f"kmerpapa-spectrum: input error: {e}", file=sys.stderr)
        return 2
    if args.verbosity > 0:
        for key, v in report.items():
            print(f"{key}={v}", file=sys.stderr)
    if args.command in ("count", "fit"):
        return 0
    try:
        if args.command in ("track", "simulate"):
            sys.stdout.flush()
        elif args.output == "-":
            sys.stdout.write(buf.getvalue())
            sys.stdout.flush()
        else:
            with open(args.output, "w") as out:
                out.write(buf.getvalue())
    except OSError as e:
        print(f"kmerpapa-spectrum: cannot write the output: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
