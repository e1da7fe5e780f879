"""An indel model -- one k-mer pattern partition for insertions and one for deletions -- fitted on
and applied to the breakpoints of a genome on both strands: ``python -m kmerpapa_amd.indel`` (the
``kmerpapa-indel`` command).

``kmerpapa-count indel`` counts breakpoint contexts at even ``k`` and the main program partitions
them; this module is what uses such a fit.  The semantics are stated in include/kmerpapa_hip.h
(the kp_ispec block): the window of breakpoint ``b`` is ``seq[b - k/2, b + k/2)``.  The partitions
are fitted on the ``ins`` and ``del_start`` columns of a both-strand counting session, so ``del``
rates mean "a deletion begins here, read 5' to 3'": on the forward strand ``r(W(b))`` is the rate of
a deletion starting at ``b`` and ``r(rc(W(b)))`` that of one ending at ``b``; a fitted partition is
not rc-symmetric even where its table is, so an insertion's rate is the mean of both look-ups.  The
work runs on the GPU (``engine.Device.ispec_*``, kp_ispec.h) or, with ``--host``, in the host session.

  join     per-kind partition files into one model file (``type pattern p_neg p_pos p_rate`` with
           the type tokens ``ins`` and ``del``, in that order; one k for both)
  fit      one both-strand counting session, the main program once per kind, and join
  regions  per BED line: breakpoints with a valid window, expected insertions and deletions by
           strand, and with ``--observed`` the observed ones, resolved as the counting resolves them
  track    the rate per breakpoint as bedGraph
  sites    per indel: its equivalence interval, the chosen breakpoint, its two patterns and rates
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
from .predict import DEFAULT_BUDGET, _bed_lines, _by_contig

HEADER = ["type", "pattern", "p_neg", "p_pos", "p_rate"]
KINDS = ("ins", "del")  # the type tokens, in kind id order (engine.ISPEC_INS, engine.ISPEC_DEL)
TRACK_KINDS = ("ins", "del_start", "del_end")


def _overlapping_pair(words, k):
    """The first two of the pattern ``words`` that share a k-mer, or None."""
    w = np.asarray(words, np.uint64)
    low = np.uint64(int("1" * k, 16))
    for i in range(w.shape[0] - 1):
        x = w[i + 1:] & w[i]
        full = ((x | (x >> np.uint64(1)) | (x >> np.uint64(2)) | (x >> np.uint64(3))) & low) == low
        if full.any():
            return i, i + 1 + int(np.flatnonzero(full)[0])
    return None


class Model:
    """An insertion and a deletion partition.  ``names``, ``pkind`` (0 ins, 1 del; uint32), ``rates``
    (float64) and ``counts`` (``(M, U)``): one entry per pattern, the insertion patterns first;
    ``k`` the pattern length, even.  Either kind may be missing."""

    def __init__(self, names, pkind, rates, counts=None):
        from .engine import pattern_word
        self.names = list(names)
        self.pkind = np.asarray(pkind, np.uint32).reshape(-1)
        self.rates = np.asarray(rates, np.float64).reshape(-1)
        self.counts = [tuple(c) for c in counts] if counts is not None else [(0, 0)] * len(self.names)
        if not self.names:
            raise ValueError("a model without patterns")
        if not len(self.names) == self.pkind.shape[0] == self.rates.shape[0] == len(self.counts):
            raise ValueError("one kind, rate and pair of counts per pattern")
        self.k = len(self.names[0])
        for kind in (0, 1):
            lens = sorted({len(x) for x, t in zip(self.names, self.pkind.tolist()) if t == kind})
            if len(lens) > 1:
                raise ValueError(f"the {KINDS[kind]} patterns have different lengths: {lens}")
        if any(len(x) != self.k for x in self.names):
            ks = [len([x for x, t in zip(self.names, self.pkind.tolist()) if t == kind][0]) for kind in (0, 1)]
            raise ValueError(f"the ins patterns are {ks[0]}-mers and the del patterns {ks[1]}-mers: one k for both kinds")
        if self.k % 2 or not 2 <= self.k <= 14:
            raise ValueError(f"the patterns are {self.k}-mers: k must be even and 2..14 (the window of a breakpoint has "
                             "k/2 bases on each side)")
        if np.any(self.pkind > 1) or np.any(np.diff(self.pkind.astype(np.int64)) < 0):
            raise ValueError("the patterns must be grouped by kind, ins before del")
        self.kinds = [KINDS[t] for t in sorted(set(self.pkind.tolist()))]
        for kind in (0, 1):
            idx = np.flatnonzero(self.pkind == kind)
            pair = _overlapping_pair([pattern_word(self.names[i]) for i in idx], self.k)
            if pair is not None:
                raise ValueError(f"the {KINDS[kind]} patterns are not a partition: {self.names[idx[pair[0]]]} and "
                                 f"{self.names[idx[pair[1]]]} share k-mers")

    @classmethod
    def from_partitions(cls, parts):
        """``parts``: ``{"ins" or "del": (names, counts, rates)}`` as ``apply.read_partition`` returns them."""
        names, pkind, rates, counts = [], [], [], []
        for kind, token in enumerate(KINDS):
            if token in parts:
                pn, pc, pr = parts[token]
                names += list(pn)
                counts += list(pc)
                rates += list(pr)
                pkind += [kind] * len(pn)
        return cls(names, pkind, rates, counts)

    @classmethod
    def read(cls, file):
        if isinstance(file, (str, os.PathLike)):
            with open(file) as f:
                return cls.read(f)
        if file.readline().split() != HEADER:
            raise ValueError(f"not an indel model: the first line must be '{' '.join(HEADER)}'")
        names, pkind, rates, counts = [], [], [], []
        for line in file:
            tok = line.split()
            if not tok:
                continue
            if len(tok) != 5:
                raise ValueError(f"bad line in the model file:\n{line.strip()}")
            if tok[0] not in KINDS:
                raise ValueError(f"not an indel model: type {tok[0]!r} is neither 'ins' nor 'del'")
            pkind.append(KINDS.index(tok[0]))
            names.append(tok[1])
            counts.append((int(tok[3]), int(tok[2])))
            rates.append(float(tok[4]))
        return cls(names, pkind, rates, counts)

    def write(self, file):
        if isinstance(file, (str, os.PathLike)):
            with open(file, "w") as f:
                return self.write(f)
        file.write(" ".join(HEADER) + "\n")
        file.write("".join(f"{KINDS[t]} {x} {u} {m} {float(r)!r}\n"
                           for t, x, (m, u), r in zip(self.pkind.tolist(), self.names, self.counts, self.rates.tolist())))

    def words(self):
        from .engine import pattern_word
        return [pattern_word(x) for x in self.names]


@contextlib.contextmanager
def session(model, host=False):
    """A kp_ispec session of ``model``: yields the object whose ``ispec_regions`` / ``ispec_track`` /
    ``ispec_sites`` / ``ispec_stats`` run in it -- the first visible GPU's ``engine.Device``, or with
    ``host=True`` the host session."""
    from . import engine
    s = engine.HostISpec() if host else engine.get_device(engine.visible_devices()[0])
    s.ispec_begin(model.k, model.words(), model.pkind)
    try:
        yield s
    finally:
        s.ispec_end()


def region_rates(contigs, model, regions, want_hist=False, host=False, budget=DEFAULT_BUDGET):
    """The model over regions of ``contigs`` (an iterable of ``(name, uint8 array)``): ``{contig:
    (hist, other, expected)}`` as ``engine.Device.ispec_regions`` returns them for ``regions[contig]``
    (``[m, 2]`` breakpoints ``begin <= b < end``).  Batching by ``budget`` counters a call changes no
    result."""
    out = {}
    with session(model, host) as s:
        for name, seq in contigs:
            if name in regions:
                out[name] = s.ispec_regions(seq, regions[name], model.rates, want_hist, budget)
    return out


def track_values(model, pid, kind):
    """``(has, value)`` per breakpoint of ``pid`` (``engine.Device.ispec_track``) for ``kind``: ``ins``
    is the mean of the two strands' insertion rates, ``del_start`` the deletion rate of the window,
    ``del_end`` that of its reverse complement.  ``has`` is False where a needed pattern is missing."""
    if kind == "ins":
        has = (pid[0] >= 0) & (pid[1] >= 0)
        value = (model.rates[np.where(has, pid[0], 0)] + model.rates[np.where(has, pid[1], 0)]) * 0.5
    else:
        plane = pid[2 if kind == "del_start" else 3]
        has = plane >= 0
        value = model.rates[np.where(has, plane, 0)]
    return has, np.where(has, value, 0.0)


def _read_observed(path, report):
    raw, st = seqio.read_indels(path)
    report.update(st)
    report.update(off_contig=0, ref_mismatch=0)
    return raw


def _place_args(args):
    if args.place == "sample" and args.seed is None:
        raise ValueError("--place sample needs --seed")
    if args.seed is not None and not 0 <= args.seed < 1 << 64:
        raise ValueError("--seed must be 0..2^64 - 1")
    return args.place, args.seed or 0


def _run_join(pairs, output):
    parts = {}
    for item in pairs:
        kind, _, path = item.partition("=")
        if not path or kind not in KINDS:
            raise ValueError(f"--type takes ins=PARTITION_FILE or del=PARTITION_FILE, not {item!r}")
        if kind in parts:
            raise ValueError(f"type {kind} given twice")
        with open(path) as f:
            parts[kind] = read_partition(f)
        if not parts[kind][0]:
            raise ValueError(f"the partition file {path} holds no pattern")
    model = Model.from_partitions(parts)
    model.write(output)
    return model


def _run_fit(args, k, host, report):
    from . import cli
    from .count import count_indels, write_counts
    place, seed = _place_args(args)
    raw = _read_observed(args.sites, report)
    seen = []

    def contigs():  # (every contig, so that a contig's index is its place in the genome)
        for name, seq in seqio.read_genome(args.genome):
            if name in raw:
                seen.append(name)
                raw[name], off, bad = seqio.match_indel_ref(seq, raw[name])
                report["off_contig"] += off
                report["ref_mismatch"] += bad
            yield name, seq

    ins, del_start, _, bg, st, _ = count_indels(contigs(), k, raw, "both", place, seed if place == "sample" else None,
                                                regions=None, host=host)
    report["unknown_contig"] = sum(len(v) for name, v in raw.items() if name not in seen)
    report.update(windows=st["windows"], windows_invalid=st["windows_invalid"], sites=st["sites"],
                  sites_skipped=st["sites_skipped"], ambiguous=st["ambiguous"])
    tables = {kind: col for kind, col in (("ins", ins), ("del", del_start)) if col.any()}
    if not tables:
        raise ValueError("no site was counted")
    tmp = None
    prefix = args.prefix
    if prefix is None:
        tmp = tempfile.TemporaryDirectory()
        prefix = os.path.join(tmp.name, "counts")
    try:
        with open(f"{prefix}.background.txt", "w") as out:
            write_counts(out, k, bg)
        pairs = []
        for kind, col in tables.items():
            with open(f"{prefix}.{kind}.txt", "w") as out:
                write_counts(out, k, col)
            part = f"{prefix}.{kind}.partition.txt"
            argv = ["-p", f"{prefix}.{kind}.txt", "-b", f"{prefix}.background.txt", "-o", part, "--verbosity",
                    str(args.verbosity)]
            if args.penalty_values:
                argv += ["-c"] + [repr(x) for x in args.penalty_values]
            if args.pseudo_counts:
                argv += ["-a"] + [repr(x) for x in args.pseudo_counts]
            if args.nfolds is not None:
                argv += ["-N", str(args.nfolds)]
            if args.fit_seed is not None:
                argv += ["--seed", str(args.fit_seed)]
            argv += ["--greedy"] * args.greedy + ["--greedyCV"] * args.greedyCV
            rc = cli.main(argv)
            gc.collect()  # (cli.main leaves its output file to be closed with its argparse namespace)
            if rc:
                raise ValueError(f"the fit of {kind} failed with exit code {rc}")
            pairs.append(f"{kind}={part}")
        model = _run_join(pairs, args.output)
        # a partition file read before it was written out in full would be short: every kind's
        # pattern counts must add up to the count tables the fit read
        for kind, col in tables.items():
            own = [c for c, t in zip(model.counts, model.pkind.tolist()) if KINDS[t] == kind]
            got = (sum(m for m, _ in own), sum(m + u for m, u in own))
            if got != (int(col.sum()), int(bg.sum())):
                raise RuntimeError(f"the partition of {kind} holds {got[0]} sites in {got[1]} windows, its count tables "
                                   f"{int(col.sum())} in {int(bg.sum())}: the partition file is incomplete")
        report["kinds"] = len(model.kinds)
        report["patterns"] = len(model.names)
    finally:
        if tmp is not None:
            tmp.cleanup()


def _resolve(s, args, raw, index, name, seq, report):
    """The indels of one contig that match its sequence, through the session's sites call:
    ``(sites, pid, resolved)``."""
    place, seed = _place_args(args)
    sites, off, bad = seqio.match_indel_ref(seq, raw[name])
    report["off_contig"] += off
    report["ref_mismatch"] += bad
    if not len(sites):
        return sites, np.zeros((0, 2), np.int32), np.zeros((0, 3), np.uint64)
    pid, res = s.ispec_sites(seq, index, sites.arrays(), place, seed)
    return sites, pid, res


def _run_regions(args, model, host, report, out):
    rows = _bed_lines(args.bed)
    per = _by_contig(rows)
    n = len(rows)
    other = np.zeros((n, 5), np.uint64)
    exp = np.zeros((n, 4), np.float64)
    obs = np.zeros((n, 3), np.int64)
    raw = _read_observed(args.observed, report) if args.observed else {}
    seen = set()
    kept = skipped = 0
    with session(model, host) as s:
        for index, (name, seq) in enumerate(seqio.read_genome(args.genome)):
            seen.add(name)
            if name in per:
                idx = np.array(per[name])
                reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
                if np.any(reg[:, 1] > seq.shape[0]):
                    b, e = reg[reg[:, 1] > seq.shape[0]][0].tolist()
                    raise ValueError(f"region {name} {b} {e} ends past the contig's {seq.shape[0]} bases")
                _, o, e = s.ispec_regions(seq, reg, model.rates, False, DEFAULT_BUDGET)
                other[idx], exp[idx] = o, e
            if name in raw:
                sites, pid, res = _resolve(s, args, raw, index, name, seq, report)
                ok = pid[:, 0] != -2
                kept += int(ok.sum())
                skipped += int((~ok).sum())
                if name in per:
                    dele = sites.del_len != 0
                    p = res[:, 2]
                    for col, pos in enumerate((p[ok & ~dele], p[ok & dele], (p + sites.del_len)[ok & dele])):
                        pos = np.sort(pos)
                        obs[idx, col] = np.searchsorted(pos, reg[:, 1], "left") - np.searchsorted(pos, reg[:, 0], "left")
        st = s.ispec_stats()
    report.update(assigned=st["assigned"], unmatched=st["unmatched"], invalid=st["invalid"],
                  unknown_contig_regions=sum(len(v) for name, v in per.items() if name not in seen))
    if args.observed:
        report["unknown_contig"] = sum(len(v) for name, v in raw.items() if name not in seen)
        report.update(kept=kept, skipped=skipped)
    labelled = any(row[3] is not None for row in rows)
    head = ["#chrom", "start", "end"] + ["name"] * labelled + ["valid", "invalid", "exp_ins_fwd", "exp_ins_rc", "exp_ins",
                                                              "exp_del_start", "exp_del_end"]
    if args.observed:
        head += ["obs_ins", "obs_del_start", "obs_del_end"]
    lines = [" ".join(head) + "\n"]
    for i, (chrom, b, e, label) in enumerate(rows):
        known = chrom in seen
        inv = int(other[i, 4])
        tok = [chrom, str(b), str(e)] + [label if label is not None else "."] * labelled
        tok += [str(e - b - inv if known else 0), str(inv)]
        fwd, rc = float(exp[i, 0]), float(exp[i, 1])
        tok += [repr(fwd), repr(rc), repr((fwd + rc) * 0.5), repr(float(exp[i, 2])), repr(float(exp[i, 3]))]
        if args.observed:
            tok += [str(int(x)) for x in obs[i]]
        lines.append(" ".join(tok) + "\n")
    out.write("".join(lines))


def _run_track(args, model, host, report, out):
    regions = seqio.read_bed(args.bed) if args.bed else None
    need = "ins" if args.kind == "ins" else "del"
    if need not in model.kinds:
        raise ValueError(f"the model has no {need} patterns")
    seen = set()
    breakpoints = 0
    with session(model, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            if regions is None:
                ranges = [(0, seq.shape[0])]
            else:
                ranges = regions.get(name, np.zeros((0, 2), np.uint64)).tolist()
            for b, e in ranges:
                if e > seq.shape[0]:
                    raise ValueError(f"region {name} {b} {e} ends past the contig's {seq.shape[0]} bases")
                pid = s.ispec_track(seq, b, e)
                if not pid.shape[1]:
                    continue
                has, value = track_values(model, pid, args.kind)
                key = np.where(has, value.view(np.int64), -1)
                first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))  # where a run starts
                last = np.concatenate([first[1:], [key.shape[0]]])
                keep = has[first]
                breakpoints += int((last - first)[keep].sum())
                out.write("".join(f"{name} {b + x} {b + y} {v!r}\n" for x, y, v in
                                  zip(first[keep].tolist(), last[keep].tolist(), value[first][keep].tolist())))
    report["breakpoints_with_a_rate"] = breakpoints
    if regions is not None:
        report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in seen)


def _run_sites(args, model, host, report, out):
    raw = _read_observed(args.sites, report)
    seen = set()
    lines = []  # (key, text)
    kept = skipped = 0
    rates = model.rates.tolist()
    with session(model, host) as s:
        for index, (name, seq) in enumerate(seqio.read_genome(args.genome)):
            if name not in raw:
                continue
            seen.add(name)
            sites, pid, res = _resolve(s, args, raw, index, name, seq, report)
            ok = pid[:, 0] != -2
            kept += int(ok.sum())
            skipped += int((~ok).sum())
            il = (sites.ins_off[1:] - sites.ins_off[:-1]).tolist()
            for key, (lo, hi, p), dl, n_ins, (a, b) in zip(sites.key.tolist(), res.tolist(), sites.del_len.tolist(), il,
                                                           pid.tolist()):
                tail = " ".join(f"{model.names[j]} {rates[j]!r}" if j >= 0 else "NA NA" for j in (a, b))
                lines.append((key, f"{name} {lo} {hi} {p} {'del' if dl else 'ins'} {dl or n_ins} {tail}\n"))
    report["unknown_contig"] = sum(len(v) for name, v in raw.items() if name not in seen)
    report.update(kept=kept, skipped=skipped)
    out.write("".join(text for _, text in sorted(lines)))


def get_parser():
    p = argparse.ArgumentParser(prog="kmerpapa-indel",
                                description="Fits and applies one k-mer pattern partition for insertions and one for "
                                            "deletions at the breakpoints of a genome, on both strands")
    sub = p.add_subparsers(dest="command", required=True)

    def common(q, output_help, default=None):
        q.add_argument("-o", "--output", metavar="PATH", help=output_help, default=default, required=default is None)
        q.add_argument("--host", action="store_true", help="Run on the host session instead of the GPU")
        q.add_argument("--verbosity", type=int, default=1,
                       help="Amount of info printed to stderr during execution. 0:silent, 1:default")

    def placing(q):
        q.add_argument("--place", choices=("left", "right", "sample"), default="left",
                       help="Where an indel inside a repeat is placed: the leftmost (default) or rightmost equivalent "
                            "placement, or one drawn per site (needs --seed); as kmerpapa-count indel")
        q.add_argument("--seed", type=int, help="Seed of --place sample")

    joi = sub.add_parser("join", help="an insertion and a deletion partition file into one model file")
    joi.add_argument("--type", action="append", required=True, metavar="KIND=FILE",
                     help="ins=FILE or del=FILE: the output table of kmerpapa (short or -l format) fitted for the kind; "
                          "either kind alone is fine")
    joi.add_argument("-o", "--output", required=True, metavar="MODEL", help="The model file")
    joi.add_argument("--verbosity", type=int, default=1)
    fit = sub.add_parser("fit", help="count on both strands, fit each kind that has sites with kmerpapa's options, and join")
    fit.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
    fit.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    size = fit.add_mutually_exclusive_group(required=True)
    size.add_argument("-k", type=int, help="Length of the k-mers (even, 2..14)")
    size.add_argument("--radius", type=int, help="Bases on each side of the breakpoint: k = 2 * radius")
    placing(fit)
    common(fit, "The model file")
    fit.add_argument("--prefix", metavar="PREFIX", help="Keep the count and partition files under this prefix")
    fit.add_argument("-c", "--penalty_values", type=float, nargs="+", metavar="c")
    fit.add_argument("-a", "--pseudo_counts", type=float, nargs="+", metavar="a")
    fit.add_argument("-N", "--nfolds", type=int, metavar="N")
    fit.add_argument("--fit-seed", type=int, dest="fit_seed", metavar="S", help="kmerpapa's --seed (of its fold split)")
    fit.add_argument("--greedy", action="store_true")
    fit.add_argument("--greedyCV", action="store_true")

    def applying(q):
        q.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
        q.add_argument("--model", required=True, metavar="FILE", help="Model file of `join` or `fit`")
        common(q, "Output file (default: standard output)", "-")

    reg = sub.add_parser("regions", help="per region: expected insertions and deletions by strand, and the observed ones")
    applying(reg)
    reg.add_argument("--bed", metavar="FILE", required=True,
                     help="The regions (breakpoints start <= b < end); a 4th column is carried through as a name")
    reg.add_argument("--observed", metavar="SITES",
                     help="CHROM POS REF ALT lines: counts per region the kept insertions and deletion starts whose chosen "
                          "breakpoint p, and the deletion ends whose p + L, lies in it")
    placing(reg)
    trk = sub.add_parser("track", help="the rate at every breakpoint, as bedGraph")
    applying(trk)
    trk.add_argument("--kind", choices=TRACK_KINDS, required=True,
                     help="ins: the mean of the two strands' insertion rates; del_start / del_end: the rate of a deletion "
                          "starting / ending at the breakpoint.  A breakpoint lacking a needed pattern is left out")
    trk.add_argument("--bed", metavar="FILE", help="Only the breakpoints of these regions")
    sit = sub.add_parser("sites", help="the interval, chosen breakpoint, patterns and rates of given indels")
    applying(sit)
    sit.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    placing(sit)
    return p


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 2 on input errors."""
    import io

    from .engine import KPError
    args = get_parser().parse_args(args=argv)
    host = host or getattr(args, "host", False)
    report = {}
    buf = io.StringIO()
    try:
        if args.command == "join":
            _run_join(args.type, args.output)
            return 0
        seqio.is_2bit(args.genome)  # (a genome that cannot be opened is reported before a GPU is touched)
        if args.command == "fit":
            k = args.k if args.k is not None else 2 * args.radius
            if not 2 <= k <= 14 or k % 2:
                raise ValueError("k must be even and 2..14 (the window of a breakpoint has k/2 bases on each side)")
            _run_fit(args, k, host, report)
        else:
            model = Model.read(args.model)
            run = {"regions": _run_regions, "track": _run_track, "sites": _run_sites}[args.command]
            if args.command == "track" and args.output != "-":  # (written contig by contig)
                with open(args.output, "w") as out:
                    run(args, model, host, report, out)
            else:
                run(args, model, host, report, sys.stdout if args.command == "track" else buf)
    except (ValueError, OSError, KeyError, KPError) as e:
        if isinstance(e, KPError) and e.code != -1:  # only KP_E_ARG is the input's fault
            raise
        print(f"kmerpapa-indel: input error: {e}", file=sys.stderr)
        return 2
    if args.verbosity > 0:
        for key, v in report.items():
            print(f"{key}={v}", file=sys.stderr)
    if args.command == "fit":
        return 0
    try:
        if args.command == "track":
            sys.stdout.flush()
        elif args.output == "-":
            sys.stdout.write(buf.getvalue())
            sys.stdout.flush()
        else:
            with open(args.output, "w") as out:
                out.write(buf.getvalue())
    except OSError as e:
        print(f"kmerpapa-indel: cannot write the output: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
