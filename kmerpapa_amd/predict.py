"""Take a fitted partition back to the genome: ``python -m kmerpapa_amd.predict`` (the
``kmerpapa-predict`` command).

The partition is the table the main program printed (either format, ``apply.read_partition``);
the genome is FASTA or ``.2bit``.  Three questions are answered on the GPU
(``engine.Device.pred_*``, kp_pred.h): how many positions of a region fall into each pattern and
how many mutations the rates expect there (``regions``), the rate at every position (``track``),
and the pattern and rate at given sites (``sites``).  Windows, the centre and strand folding are
``kmerpapa-count``'s (include/kmerpapa_hip.h); a position whose window matches no pattern -- the
normal case under a super pattern such as ``NNCNN`` without folding -- has no rate.  The reference
has no such step.
"""
import argparse
import contextlib
import sys

import numpy as np

from . import seqio
from .apply import lca_pattern, read_partition

DEFAULT_BUDGET = 1 << 27  # counters of one kp_pred_regions call (8 bytes each: 1 GiB)


@contextlib.contextmanager
def session(names, fold=True, host=False):
    """A kp_pred session of the patterns ``names`` (disjoint IUPAC patterns of one length, order
    kept): yields the object whose ``pred_regions`` / ``pred_track`` / ``pred_sites`` /
    ``pred_stats`` run in it -- the first visible GPU's ``engine.Device``, or with ``host=True``
    the host session."""
    from . import engine
    names = list(names)
    if not names:
        raise ValueError("no patterns")
    k = len(names[0])
    if any(len(x) != k for x in names):
        raise ValueError("patterns of different lengths")
    words = [engine.pattern_word(x) for x in names]
    s = engine.HostPred() if host else engine.get_device(engine.visible_devices()[0])
    s.pred_begin(k, words, engine.pattern_word(lca_pattern(names)), fold)
    try:
        yield s
    finally:
        s.pred_end()


def _region_array(reg):
    reg = np.asarray(reg, dtype=np.int64).reshape(-1, 2)
    if np.any(reg < 0) or np.any(reg[:, 0] > reg[:, 1]):
        raise ValueError("a region with a negative bound or start > end")
    return reg.astype(np.uint64)


def _contig_regions(s, seq, reg, P, rates, want_hist, budget):
    """One contig's regions in batches of at most ``budget`` counters a call."""
    m = reg.shape[0]
    step = max(1, int(budget) // max(P, 1))
    hist = np.zeros((m, P), np.uint64) if want_hist else None
    other = np.zeros((m, 2), np.uint64)
    exp = np.zeros(m, np.float64) if rates is not None else None
    for b in range(0, m, step):
        h, o, e = s.pred_regions(seq, reg[b:b + step], rates, want_hist)
        other[b:b + step] = o
        if want_hist:
            hist[b:b + step] = h
        if exp is not None:
            exp[b:b + step] = e
    return hist, other, exp


def region_counts(contigs, names, regions, rates=None, fold=True, want_hist=True, host=False, budget=DEFAULT_BUDGET):
    """The patterns ``names`` counted over regions of ``contigs`` (an iterable of ``(name, uint8
    array)``).  ``regions``: ``{contig: [m, 2]}`` 0-based half-open intervals, in any order,
    overlapping or not; each is one output row.  Returns ``{contig: (hist, other, expected)}`` for
    the contigs of the genome that have regions: ``hist`` uint64 ``[m, P]`` (None without
    ``want_hist``), ``other`` uint64 ``[m, 2]`` = positions without a pattern, positions without
    a valid window; ``expected`` float64 ``[m]`` = the sum of ``hist * rates`` in pattern order
    (None without ``rates``).  A call's ``m x P`` counters are cut into batches of at most
    ``budget``; batching changes no result."""
    names = list(names)
    out = {}
    with session(names, fold, host) as s:
        for name, seq in contigs:
            if name in regions:
                out[name] = _contig_regions(s, seq, _region_array(regions[name]), len(names), rates, want_hist, budget)
    return out


def track(seq_or_contigs, names, fold=True, host=False, begin=0, end=None):
    """The pattern index at every position: int32, -1 where no pattern matches, -2 where the
    window holds an invalid byte or runs off the contig.  For one contig (a uint8 array; with
    ``begin`` / ``end`` a range of it) the array; for an iterable of ``(name, array)`` a dict of
    whole-contig arrays."""
    with session(names, fold, host) as s:
        if isinstance(seq_or_contigs, (np.ndarray, bytes, bytearray)):
            seq = np.frombuffer(seq_or_contigs, np.uint8) if not isinstance(seq_or_contigs, np.ndarray) else seq_or_contigs
            return s.pred_track(seq, begin, end)
        return {name: s.pred_track(seq) for name, seq in seq_or_contigs}


def rates_of(pid, rates):
    """The rate of every pattern index of ``pid``; ``nan`` where ``pid < 0``."""
    pid = np.asarray(pid)
    r = np.concatenate([np.asarray(rates, np.float64).reshape(-1), [np.nan]])
    return r[np.where(pid < 0, r.shape[0] - 1, pid)]


def site_patterns(contigs, names, sites, fold=True, host=False):
    """:func:`track`'s code at given sites: ``sites`` is ``{contig: 0-based positions}`` (each
    below the contig's length), the result ``{contig: int32 array}``, duplicates included."""
    out = {}
    with session(names, fold, host) as s:
        for name, seq in contigs:
            if name in sites:
                out[name] = s.pred_sites(seq, sites[name])
    return out


def _bed_lines(path):
    """``(chrom, start, end, name or None)`` of every BED line, in file order."""
    rows = []
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok or tok[0].startswith("#") or tok[0] in ("track", "browser"):
                continue
            try:
                rows.append((tok[0], int(tok[1]), int(tok[2]), tok[3] if len(tok) > 3 else None))
            except (ValueError, IndexError):
                raise ValueError(f"bad BED line:\n{line.strip()}") from None
            if rows[-1][1] < 0 or rows[-1][1] > rows[-1][2]:
                raise ValueError(f"bad BED line (start > end or negative):\n{line.strip()}")
    return rows


def _site_lines(path):
    """``(chrom, pos1, ref, alt)`` of every single-nucleotide line of a sites file, in file order,
    and the number of lines that are none (seqio.read_sites' rules)."""
    rows, skipped = [], 0
    with open(path) as f:
        for line in f:
            tok = line.split()
            if not tok or tok[0].startswith("#"):
                continue
            if len(tok) < 4:
                raise ValueError(f"bad sites line (CHROM POS REF ALT):\n{line.strip()}")
            try:
                pos = int(tok[1])
            except ValueError:
                raise ValueError(f"bad sites line (CHROM POS REF ALT):\n{line.strip()}") from None
            if pos < 1:
                raise ValueError(f"POS is 1-based:\n{line.strip()}")
            ref, alt = tok[2].upper(), tok[3].upper()
            if len(ref) != 1 or len(alt) != 1 or ref not in "ACGT" or alt not in "ACGT" or ref == alt:
                skipped += 1
                continue
            rows.append((tok[0], pos, tok[2], tok[3]))
    return rows, skipped


def _by_contig(rows):
    """Row indices per contig, in order."""
    per = {}
    for i, row in enumerate(rows):
        per.setdefault(row[0], []).append(i)
    return per


def _run_regions(args, names, rates, fold, host, report, out):
    rows = _bed_lines(args.bed)
    per = _by_contig(rows)
    n = len(rows)
    other = np.zeros((n, 2), np.uint64)
    exp = np.zeros(n, np.float64)
    seen = set()
    with session(names, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            if name in per:
                seen.add(name)
                idx = np.array(per[name])
                reg = np.array([(rows[i][1], rows[i][2]) for i in per[name]], np.uint64)
                _, o, e = _contig_regions(s, seq, reg, len(names), rates, False, DEFAULT_BUDGET)
                other[idx], exp[idx] = o, e
        st = s.pred_stats()
    report.update(assigned=st["assigned"], unmatched=st["unmatched"], invalid=st["invalid"],
                  unknown_contig_regions=sum(len(v) for name, v in per.items() if name not in seen))
    lines = []
    for (chrom, b, e, label), o, x in zip(rows, other.tolist(), exp.tolist()):
        known = chrom in seen
        head = f"{chrom} {b} {e}" + (f" {label}" if label is not None else "")
        lines.append(f"{head} {(e - b - o[0] - o[1]) if known else 0} {o[0]} {o[1]} {x!r}\n")
    out.write("".join(lines))


def _run_track(args, names, rates, fold, host, report, out):
    regions = seqio.read_bed(args.bed) if args.bed else None
    seen = set()
    positions = 0
    with session(names, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            seen.add(name)
            if regions is None:
                ranges = [(0, seq.shape[0])]
            else:
                ranges = regions.get(name, np.zeros((0, 2), np.uint64)).tolist()
            for b, e in ranges:
                if e > seq.shape[0]:
                    raise ValueError(f"region {name} {b} {e} ends past the contig's {seq.shape[0]} bases")
                pid = s.pred_track(seq, b, e)
                if not pid.shape[0]:
                    continue
                first = np.flatnonzero(np.concatenate([[True], pid[1:] != pid[:-1]]))  # where a run starts
                last = np.concatenate([first[1:], [pid.shape[0]]])
                keep = pid[first] >= 0
                positions += int((last - first)[keep].sum())
                out.write("".join(f"{name} {b + x} {b + y} {rates[p]!r}\n" for x, y, p in
                                  zip(first[keep].tolist(), last[keep].tolist(), pid[first][keep].tolist())))
    report["positions_with_a_rate"] = positions
    if regions is not None:
        report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in seen)


def _run_sites(args, names, rates, fold, host, report, out):
    rows, skipped = _site_lines(args.sites)
    per = _by_contig(rows)
    pid = np.full(len(rows), -3, np.int32)  # -3: not looked up
    report.update(lines=len(rows) + skipped, not_snv=skipped, off_contig=0, ref_mismatch=0)
    seen = set()
    with session(names, fold, host) as s:
        for name, seq in seqio.read_genome(args.genome):
            if name in per:
                seen.add(name)
                idx = np.array(per[name])
                pos = np.array([rows[i][1] - 1 for i in per[name]], np.uint64)
                ref = np.array([ord(rows[i][2].upper()) for i in per[name]], np.uint8)
                on = pos < np.uint64(seq.shape[0])
                same = np.zeros(pos.shape[0], bool)
                same[on] = (seq[pos[on].astype(np.intp)] & 0xDF) == ref[on]
                report["off_contig"] += int((~on).sum())
                report["ref_mismatch"] += int((on & ~same).sum())
                pid[idx[same]] = s.pred_sites(seq, pos[same])
    report["unknown_contig"] = sum(len(v) for name, v in per.items() if name not in seen)
    report["without_pattern"] = int(((pid == -1) | (pid == -2)).sum())
    out.write("".join(f"{c} {p} {r} {a} " + (f"{names[j]} {rates[j]!r}\n" if j >= 0 else "NA NA\n")
                      for (c, p, r, a), j in zip(rows, pid.tolist())))


def get_parser():
    p = argparse.ArgumentParser(prog="kmerpapa-predict",
                                description="Applies a fitted k-mer pattern partition to the positions of a genome")
    sub = p.add_subparsers(dest="command", required=True)

    def common(q):
        q.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
        q.add_argument("--partition", required=True, metavar="FILE",
                       help="Output table of kmerpapa (short or -l format): the patterns and their rates")
        q.add_argument("--no-fold", action="store_true",
                       help="Match every window as read; default: a window with G or T in the centre is matched "
                            "as its reverse complement")
        q.add_argument("-o", "--output", default="-", metavar="PATH", help="Output file (default: standard output)")
        q.add_argument("--verbosity", type=int, default=1,
                       help="Amount of info printed to stderr during execution. 0:silent, 1:default")

    reg = sub.add_parser("regions", help="positions per region with a pattern, and the mutations the rates expect there")
    common(reg)
    reg.add_argument("--bed", metavar="FILE", required=True, help="The regions; a 4th column is carried through as a name")
    trk = sub.add_parser("track", help="the rate at every position, as bedGraph")
    common(trk)
    trk.add_argument("--bed", metavar="FILE", help="Only the positions of these regions")
    sit = sub.add_parser("sites", help="the pattern and rate at given sites")
    common(sit)
    sit.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    return p


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 1 with a message if the patterns overlap; 2 on input
    errors."""
    import io

    from .engine import KPError, apply_host, pattern_word
    args = get_parser().parse_args(args=argv)
    report = {}
    buf = io.StringIO()
    try:
        with open(args.partition) as f:
            names, _, rates = read_partition(f)
        if not names:
            raise ValueError("the partition file holds no pattern")
        k = len(names[0])
        if any(len(x) != k for x in names):
            raise ValueError("patterns of different lengths")
        fold = not args.no_fold
        if not 1 <= k <= 15:
            raise ValueError("the patterns must be 1..15 positions long")
        if fold and k % 2 == 0:
            raise ValueError("strand folding needs an odd k (use --no-fold)")
        seqio.is_2bit(args.genome)  # (a genome that cannot be opened is reported before a GPU is touched)
        run = {"regions": _run_regions, "track": _run_track, "sites": _run_sites}[args.command]
        try:
            if args.command == "track" and args.output != "-":
                # a genome's track is too long to hold: it is written contig by contig
                with open(args.output, "w") as out:
                    run(args, names, rates, fold, host, report, out)
            else:
                run(args, names, rates, fold, host, report, sys.stdout if args.command == "track" else buf)
        except KPError as e:
            if e.code == -1 and "not a partition" in str(e):
                words = [pattern_word(x) for x in names]
                st = apply_host(k, words, pattern_word(lca_pattern(names)), [], [], [])[4]
                print(f"kmerpapa-predict: the patterns are not a partition: {st['overlap_pairs']} pairs of patterns "
                      "share k-mers", file=sys.stderr)
                return 1
            raise
    except (ValueError, OSError, KeyError, KPError) as e:
        if isinstance(e, KPError) and e.code != -1:  # only KP_E_ARG is the input's fault
            raise
        print(f"kmerpapa-predict: input error: {e}", file=sys.stderr)
        return 2
    if args.verbosity > 0:
        for key, v in report.items():
            print(f"{key}={v}", file=sys.stderr)
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
        print(f"kmerpapa-predict: cannot write the output: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
