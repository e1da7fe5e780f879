"""k-mer context counts of a genome and of its mutation sites: ``python -m kmerpapa_amd.count``
(the ``kmerpapa-count`` command).

This is the step before everything else the package does: it turns a genome (FASTA or
``.2bit``), optionally a BED file of regions, and a list of mutations into the ``kmer count``
files the main program reads with ``-b`` and ``-p``.  The reference has no such step (its
README names an external tool); the semantics are this project's own, stated in
include/kmerpapa_hip.h: a window counts only if all its k bytes are ``ACGTacgt``; a window
belongs to the region its centre (position ``start + k // 2``) lies in; by default a window with
G or T in the centre is counted as its reverse complement.  The counting runs on the GPU
(``engine.Device.seq_*``, kp_seq.h), contig by contig into one dense table of ``4^k`` counters
per column.
"""
import argparse
import sys

import numpy as np

from . import seqio
from .io_utils import KmerCounts


INDEL_COLUMNS = ("ins", "del_start", "del_end")  # the positive columns of an indel session, in order


def count_genome(contigs, k, fold=True, regions=None, sites=None, host=False):
    """Count the ``k``-mer windows of ``contigs`` (an iterable of ``(name, uint8 array)``).

    ``regions``: None = every contig whole; a dict ``{name: [m, 2]}`` of 0-based half-open
    intervals (merged here; a contig without an entry is not scanned); False = no background
    scan.  ``sites``: None, or a dict ``{name: 0-based positions}``, each counted once per
    occurrence.  ``host=True`` runs the session on the host (``engine.seq_host``).

    Returns ``(pos_counts, bg_counts, stats)``: dense uint64 ``[4^k]`` tables in code order (2
    bits per letter, A = 0 .. T = 3, first letter most significant) and the session's figures
    (``engine.KPSeqStats`` as a dict)."""
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
            pos = sites.get(name) if sites is not None else None
            if reg is not False or (pos is not None and len(pos)):
                yield seq, reg, pos

    if host:
        return engine.seq_host(k, fold, jobs())
    return engine.get_device(engine.visible_devices()[0]).seq_count(k, fold, jobs())


def _region_jobs(contigs, regions):
    """``(index, name, seq, regions for seq_scan or False)`` of every contig, in order."""
    for index, (name, seq) in enumerate(contigs):
        if regions is None:
            reg = None
        elif regions is False or name not in regions:
            reg = False
        else:
            reg = seqio.merge_regions(regions[name])
            reg = reg if reg.shape[0] else False
        yield index, name, seq, reg


def _seq_calls(host):
    from . import engine
    return engine.HostSeq() if host else engine.get_device(engine.visible_devices()[0])


def count_strands(contigs, k, strands="both", regions=None, host=False):
    """The background of ``contigs`` without strand folding, any ``k`` in 1..15: every valid window
    adds 1 at its code and, with ``strands="both"``, 1 at its reverse complement's (a palindromic
    window 2 in one cell).  ``regions`` as :func:`count_genome`'s.  Returns ``(bg_counts, stats)``."""
    if strands not in ("both", "forward"):
        raise ValueError("strands must be 'both' or 'forward'")
    jobs = ((seq, reg) for _, _, seq, reg in _region_jobs(contigs, regions))
    return _seq_calls(host).seq_count_strands(k, strands == "both", jobs)


def count_indels(contigs, k, sites, strands="both", place="left", seed=None, regions=None, host=False):
    """Count the breakpoint contexts of short insertions and deletions at even ``k`` (semantics:
    include/kmerpapa_hip.h).  ``contigs``: an iterable of ``(name, uint8 array)``; a contig's
    position in it is the index its placement draws are keyed by, so pass the whole genome in its
    order.  ``sites``: ``{name: seqio.IndelSites}`` (or ``{name: engine.indel_sites(...)}``).
    ``strands``: ``"both"`` (every add with its mirror on the other strand) or ``"forward"``.
    ``place``: ``"left"``, ``"right"`` or ``"sample"`` (needs ``seed``) within a site's equivalence
    interval.  ``regions``: the background scan, as :func:`count_genome`'s (False = none).

    Returns ``(ins, del_start, del_end, bg, stats, resolved)``: four dense uint64 ``[4^k]`` tables,
    the session's figures plus ``ambiguous`` (sites with hi > lo), and ``{name: uint64 [m, 3]}``
    with lo, hi and the chosen breakpoint of every site passed, skipped ones included."""
    from . import engine
    if strands not in ("both", "forward"):
        raise ValueError("strands must be 'both' or 'forward'")
    if place not in engine.INDEL_PLACE:
        raise ValueError("place must be 'left', 'right' or 'sample'")
    if place == "sample" and seed is None:
        raise ValueError("place='sample' needs a seed")
    names = []

    def jobs():
        for index, name, seq, reg in _region_jobs(contigs, regions):
            s = sites.get(name) if sites is not None else None
            if s is not None and not isinstance(s, tuple):
                s = s.arrays()
            if s is not None and not len(s[0]):
                s = None
            if reg is not False or s is not None:
                names.append(name)
                yield seq, reg, index, s

    cols, bg, stats, res = _seq_calls(host).seq_count_indels(k, strands == "both", jobs(), place, seed or 0)
    resolved = {name: r for name, r in zip(names, res) if r is not None}
    stats = dict(stats, ambiguous=sum(int((r[:, 1] > r[:, 0]).sum()) for r in resolved.values()))
    return cols[0], cols[1], cols[2], bg, stats, resolved


def table_of(k, pos_counts, bg_counts):
    """The count table of two dense columns: rows = the k-mers with a non-zero background
    count, M = positive, U = background - positive.  ``ValueError`` if a k-mer has more
    positives than background (read_postive_and_other's rule)."""
    bad = np.flatnonzero(pos_counts > bg_counts)
    if bad.shape[0]:
        kmer = KmerCounts(k, bad[:1], [0], [0]).kmer_at(0)
        raise ValueError("background counts should be larger than the positive counts so that a negative set can "
                         f"be created by subtraction. Problematic k-mer: {kmer}")
    codes = np.flatnonzero(bg_counts)
    return KmerCounts(k, codes, pos_counts[codes].astype(np.int64),
                      (bg_counts[codes] - pos_counts[codes]).astype(np.int64))


def count_table(contigs, k, fold=True, regions=None, sites=None, host=False):
    """:func:`count_genome` as an ``io_utils.KmerCounts`` (:func:`table_of`): what the fit, the
    CV driver, ``kp_greedy`` and ``kp_apply`` take, with no text in between."""
    pos, bg, _ = count_genome(contigs, k, fold, regions, sites, host)
    return table_of(k, pos, bg)


def write_counts(out, k, counts):
    """``kmer count`` lines of the non-zero k-mers in sorted order (the format of ``-p``/``-b``)."""
    codes = np.flatnonzero(counts)
    keys = KmerCounts(k, codes, counts[codes].astype(np.int64), np.zeros(codes.shape[0], np.int64))._key_list()
    out.write("".join(f"{key} {c}\n" for key, c in zip(keys, counts[codes].tolist())))
    out.flush()


def get_parser():
    p = argparse.ArgumentParser(prog="kmerpapa-count",
                                description="Counts the k-mer contexts of a genome or of mutation sites in it")
    sub = p.add_subparsers(dest="command", required=True)

    def common(q):
        q.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
        size = q.add_mutually_exclusive_group(required=True)
        size.add_argument("-k", type=int, help="Length of the k-mers (1..15; odd unless --no-fold)")
        size.add_argument("--radius", type=int, help="Bases on each side of the centre: k = 2 * radius + 1")
        q.add_argument("--no-fold", action="store_true",
                       help="Count every window as read; default: a window with G or T in the centre is counted "
                            "as its reverse complement")
        q.add_argument("-o", "--output", default="-", metavar="PATH",
                       help="Output file, written once the counting has succeeded (default: standard output)")
        q.add_argument("--verbosity", type=int, default=1,
                       help="Amount of info printed to stderr during execution. 0:silent, 1:default")

    bg = sub.add_parser("background", help="k-mer counts of the whole genome or of the regions of a BED file")
    common(bg)
    bg.add_argument("--bed", metavar="FILE", help="Count only windows whose centre lies in these regions")
    bg.add_argument("--strands", choices=("both", "forward"),
                    help="Count without centre folding, at any k: every window as read and, with 'both', also as "
                         "its reverse complement (the background of an indel table)")
    indel = sub.add_parser("indel", help="k-mer counts around the breakpoints of short insertions and deletions")
    indel.add_argument("genome", help="Genome as FASTA (plain text) or UCSC .2bit")
    indel.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    indel.add_argument("column", choices=INDEL_COLUMNS, help="The table to write: insertions, deletion starts or deletion ends")
    size = indel.add_mutually_exclusive_group(required=True)
    size.add_argument("-k", type=int, help="Length of the k-mers (even, 2..14)")
    size.add_argument("--radius", type=int, help="Bases on each side of the breakpoint: k = 2 * radius")
    indel.add_argument("--strands", choices=("both", "forward"), default="both",
                       help="both (default): every site is also counted as read on the other strand")
    indel.add_argument("--place", choices=("left", "right", "sample"), default="left",
                       help="Where an indel inside a repeat is counted: the leftmost (default) or rightmost equivalent "
                            "placement, or one drawn per site (needs --seed)")
    indel.add_argument("--seed", type=int, help="Seed of --place sample")
    indel.add_argument("--resolved", metavar="FILE",
                       help="Write CHROM LO HI CHOSEN KIND LEN (0-based breakpoints) of every site handed to the counter")
    indel.add_argument("-o", "--output", default="-", metavar="PATH",
                       help="Output file, written once the counting has succeeded (default: standard output)")
    indel.add_argument("--verbosity", type=int, default=1,
                       help="Amount of info printed to stderr during execution. 0:silent, 1:default")
    snv = sub.add_parser("snv", help="k-mer counts around single-nucleotide variants")
    common(snv)
    snv.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    snv.add_argument("--type", metavar="X>Y", help="Count only mutations of this type after strand folding (G>A is C>T)")
    return p


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 2 on input errors."""
    args = get_parser().parse_args(args=argv)
    from .engine import KPError
    resolved_text = None
    try:
        if args.command == "indel":
            k = args.k if args.k is not None else 2 * args.radius
            fold = False
            if not 2 <= k <= 14 or k % 2:
                raise ValueError("k must be even and 2..14 (the window of a breakpoint has k/2 bases on each side)")
            if args.place == "sample" and args.seed is None:
                raise ValueError("--place sample needs --seed")
            if args.seed is not None and not 0 <= args.seed < 1 << 64:
                raise ValueError("--seed must be 0..2^64 - 1")
        else:
            k = args.k if args.k is not None else 2 * args.radius + 1
            fold = not args.no_fold and getattr(args, "strands", None) is None
            if not 1 <= k <= 15:
                raise ValueError("k must be 1..15")
            if fold and k % 2 == 0:
                raise ValueError("strand folding needs an odd k (use --no-fold)")
        report = {}
        seqio.is_2bit(args.genome)  # (a genome that cannot be opened is reported before a GPU is touched)
        if args.command == "indel":
            raw, report = seqio.read_indels(args.sites)
            report.update(off_contig=0, ref_mismatch=0)
            seen = []

            def contigs():  # (every contig, so that a contig's index is its place in the genome)
                for name, seq in seqio.read_genome(args.genome):
                    if name in raw:
                        seen.append(name)
                        raw[name], off, bad = seqio.match_indel_ref(seq, raw[name])
                        report["off_contig"] += off
                        report["ref_mismatch"] += bad
                    yield name, seq

            *cols, _, st, resolved = count_indels(contigs(), k, raw, args.strands, args.place, args.seed, regions=False,
                                                  host=host)
            counts = cols[INDEL_COLUMNS.index(args.column)]
            report["unknown_contig"] = sum(len(v) for name, v in raw.items() if name not in seen)
            report.update(sites=st["sites"], sites_skipped=st["sites_skipped"], ambiguous=st["ambiguous"])
            if args.resolved:
                lines = []
                for name in seen:
                    s = raw[name]
                    for (lo, hi, p), dl, il in zip(resolved.get(name, np.zeros((0, 3), np.uint64)).tolist(), s.del_len.tolist(),
                                                   (s.ins_off[1:] - s.ins_off[:-1]).tolist()):
                        lines.append(f"{name} {lo} {hi} {p} {'del' if dl else 'ins'} {dl or il}\n")
                resolved_text = "".join(lines)
        elif args.command == "background":
            regions = seqio.read_bed(args.bed) if args.bed else None
            names = set()

            def named():
                for name, seq in seqio.read_genome(args.genome):
                    names.add(name)
                    yield name, seq

            if args.strands is not None:
                counts, st = count_strands(named(), k, args.strands, regions=regions, host=host)
            else:
                _, counts, st = count_genome(named(), k, fold, regions=regions, host=host)
            report.update(windows=st["windows"], windows_invalid=st["windows_invalid"])
            if regions is not None:  # (merged) regions on contigs the genome does not have
                report["unknown_contig_regions"] = sum(len(v) for name, v in regions.items() if name not in names)
        else:
            raw, report = seqio.read_sites(args.sites, seqio.parse_type(args.type) if args.type else None)
            report.update(off_contig=0, ref_mismatch=0)
            seen = set()

            def contigs():
                for name, seq in seqio.read_genome(args.genome):
                    if name in raw:
                        seen.add(name)
                        pos, off, bad = seqio.match_ref(seq, *raw[name])
                        report["off_contig"] += off
                        report["ref_mismatch"] += bad
                        raw[name] = pos
                        yield name, seq

            counts, _, st = count_genome(contigs(), k, fold, regions=False, sites=raw, host=host)
            report["unknown_contig"] = sum(len(v[0]) for name, v in raw.items() if name not in seen)
            report.update(sites=st["sites"], sites_skipped=st["sites_skipped"])
    except (ValueError, OSError, KPError) as e:
        if isinstance(e, KPError) and e.code != -1:  # only KP_E_ARG is the input's fault
            raise
        print(f"kmerpapa-count: input error: {e}", file=sys.stderr)
        return 2
    if args.verbosity > 0:
        for key, v in report.items():
            print(f"{key}={v}", file=sys.stderr)
    try:
        if resolved_text is not None:
            with open(args.resolved, "w") as out:
                out.write(resolved_text)
        if args.output == "-":
            write_counts(sys.stdout, k, counts)
        else:
            with open(args.output, "w") as out:
                write_counts(out, k, counts)
    except OSError as e:
        print(f"kmerpapa-count: cannot write the output: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
