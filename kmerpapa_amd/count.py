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
    snv = sub.add_parser("snv", help="k-mer counts around single-nucleotide variants")
    common(snv)
    snv.add_argument("sites", help="File of CHROM POS REF ALT lines, POS 1-based")
    snv.add_argument("--type", metavar="X>Y", help="Count only mutations of this type after strand folding (G>A is C>T)")
    return p


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 2 on input errors."""
    args = get_parser().parse_args(args=argv)
    from .engine import KPError
    try:
        k = args.k if args.k is not None else 2 * args.radius + 1
        fold = not args.no_fold
        if not 1 <= k <= 15:
            raise ValueError("k must be 1..15")
        if fold and k % 2 == 0:
            raise ValueError("strand folding needs an odd k (use --no-fold)")
        report = {}
        seqio.is_2bit(args.genome)  # (a genome that cannot be opened is reported before a GPU is touched)
        if args.command == "background":
            regions = seqio.read_bed(args.bed) if args.bed else None
            names = set()

            def named():
                for name, seq in seqio.read_genome(args.genome):
                    names.add(name)
                    yield name, seq

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
