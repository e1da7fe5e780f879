"""Apply a fitted partition to new k-mer counts: ``python -m kmerpapa_amd.apply`` (the
``kmerpapa-apply`` command).

The partition is the table the main program printed -- its short format ``pattern p_neg p_pos
p_rate`` or its ``-l`` format -- and the counts are given with the main program's count-file
flags.  Every k-mer of the new table is matched against every pattern on the GPU
(``engine.Device.apply``, kp_apply: mask matching, no enumeration, so the table may be a
sparse list of observed k-mers), which gives the table's counts per pattern and its -2
log-likelihood under the fitted rates -- the held-out score model comparisons use.  The
reference has no such step.
"""
import argparse
import sys

from .io_utils import read_input_table
from .papa import Pattern

_SHORT = ["pattern", "p_neg", "p_pos", "p_rate"]
_LONG = ["context", "c_neg", "c_pos", "c_rate"] + _SHORT


def _partition_rows(f):
    """The ``[pattern, p_neg, p_pos, p_rate]`` tokens of a partition file, one list per
    pattern in order of first appearance."""
    header = f.readline().split()
    if header == _SHORT:
        first = 0
    elif header == _LONG:
        first = 4
    else:
        raise ValueError("not a kmerpapa output table: the first line must be "
                         f"'{' '.join(_SHORT)}' or '{' '.join(_LONG)}'")
    rows, seen = [], set()
    for line in f:
        tok = line.split()
        if not tok:
            continue
        if len(tok) != first + 4:
            raise ValueError(f"bad line in the partition file:\n{line.strip()}")
        if first and tok[4] in seen:
            continue
        seen.add(tok[first])
        rows.append(tok[first:])
    return rows


def read_partition(f):
    """Read a partition from either output format of the CLI.  Returns ``(names, counts,
    rates)``: the patterns in file order (the ``-l`` format: order of first appearance), their
    training counts ``(p_pos, p_neg)`` -- (M, U), as ``KmerCounts.pattern_counts`` orders
    them -- and their rates as ``float(token)``: Python prints the shortest text that reads
    back to the same float, so these are the fitted rates bit for bit."""
    rows = _partition_rows(f)
    return ([r[0] for r in rows], [(int(r[2]), int(r[1])) for r in rows], [float(r[3]) for r in rows])


def lca_pattern(names):
    """The smallest pattern that holds every pattern of ``names``."""
    from .engine import pattern_word, word_pattern
    w = 0
    for name in names:
        w |= pattern_word(name)
    return word_pattern(w, len(names[0]))


def apply_partition(names, table, rates=None, want_pid=True, host=False):
    """``names`` (patterns in any order, kept) applied to ``table`` (io_utils.KmerCounts):
    ``(pid, pat_M, pat_U, ll, stats)`` of ``engine.Device.apply`` with the patterns' LCA as
    the super pattern; ``host=True`` computes it on the host (``engine.apply_host``)."""
    from . import engine
    k = len(names[0])
    if any(len(x) != k for x in names):
        raise ValueError("patterns of different lengths")
    if table.k != k:
        raise ValueError(f"the table holds {table.k}-mers, the partition {k}-mers")
    words = [engine.pattern_word(x) for x in names]
    sw = engine.pattern_word(lca_pattern(names))
    if host:
        return engine.apply_host(k, words, sw, table.codes, table.M, table.U, rates, want_pid)
    dev = engine.get_device(engine.visible_devices()[0])
    return dev.apply(k, words, sw, table.codes, table.M, table.U, rates, want_pid)


def get_parser():
    p = argparse.ArgumentParser(prog="kmerpapa-apply",
                                description="Applies a fitted k-mer pattern partition to new k-mer counts")
    p.add_argument("--partition", type=argparse.FileType("r"), required=True, metavar="FILE",
                   help="Output table of kmerpapa (short or -l format): the patterns and their rates")
    p.add_argument("-p", "--positive", type=argparse.FileType("r"),
                   help="File with k-mer counts in positive set")
    p.add_argument("-n", "--negative", type=argparse.FileType("r"),
                   help="File with k-mer counts in negative set.")
    p.add_argument("-b", "--background", type=argparse.FileType("r"),
                   help="File with k-mer counts in backgound set (includes both positive and negative regions).")
    p.add_argument("-j", "--joint_context_counts", type=argparse.FileType("r"),
                   help="File with k-mer counts in positive set and background set.")
    p.add_argument("-s", "--super_pattern", type=str,
                   help="Only consider k-mers that match this pattern.")
    p.add_argument("-o", "--output", type=argparse.FileType("w"), default="-", metavar="PATH",
                   help="Output file (default: standard output)")
    p.add_argument("-l", "--long_output", action="store_true",
                   help="Print one row per k-mer of the count table with its pattern and rate.")
    p.add_argument("--verbosity", type=int, default=1,
                   help="Amount of info printed to stderr during execution. 0:silent, 1:default")
    return p


def main(argv=None, host=False):
    """Run the program.  Exit code 0; 1 with a message if the patterns overlap; 2 on input
    errors.  k-mers that match no pattern are reported on stderr and are not fatal: a
    partition fitted under ``-s NNCNN`` leaves the other k-mers of a full table unmatched."""
    args = get_parser().parse_args(args=argv)
    try:
        rows = _partition_rows(args.partition)
        args.partition.close()
        if not rows:
            raise ValueError("the partition file holds no pattern")
        names = [r[0] for r in rows]
        rates = [float(r[3]) for r in rows]
        super_pattern = Pattern(args.super_pattern) if args.super_pattern is not None else None
        table, _, _ = read_input_table(args, super_pattern)
        pid, pat_M, pat_U, ll, st = apply_partition(names, table, rates, want_pid=args.long_output, host=host)
    except (ValueError, AssertionError, StopIteration) as e:
        print(f"kmerpapa-apply: input error: {e}", file=sys.stderr)
        return 2
    if st["overlap_pairs"]:
        print(f"kmerpapa-apply: the patterns are not a partition: {st['overlap_pairs']} pairs of patterns share "
              f"k-mers ({st['multi']} k-mers of the count table match several patterns)", file=sys.stderr)
        return 1
    if args.verbosity > 0:
        print(f"LL_test={float(ll[0])!r}", file=sys.stderr)
        for key in ("unmatched", "multi"):
            if st[key]:
                print(f"{key}={st[key]}", file=sys.stderr)
    out = args.output
    if args.long_output:
        print("context", "c_neg", "c_pos", "pattern", "p_rate", file=out)
        tails = [f" {r[0]} {r[3]}\n" for r in rows] + [" NA NA\n"]  # the last: no pattern matches the row
        none = len(rows)
        out.write("".join(f"{key} {u} {m}{tails[j if j >= 0 else none]}" for key, m, u, j in
                          zip(table._key_list(), table.M.tolist(), table.U.tolist(), pid.tolist())))
    else:
        print(*_SHORT, "t_neg", "t_pos", file=out)
        for r, m, u in zip(rows, pat_M.tolist(), pat_U.tolist()):
            print(*r, u, m, file=out)
    out.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
