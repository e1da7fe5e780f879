"""Readers for the inputs of :mod:`kmerpapa_amd.count` (host code, numpy): genomes as FASTA or
UCSC ``.2bit``, regions as BED, mutation sites as ``CHROM POS REF ALT`` lines, and for
:mod:`kmerpapa_amd.spectrum` the CDS of transcripts as GTF or BED6.

A contig is ``(name, uint8 array)``, one byte per base, exactly as the file spells it: lower-case
soft-masking is kept, since the counting kernel reads either case, and every byte other than
``ACGTacgt`` (``N``, IUPAC ambiguity letters) stays what it is and invalidates the windows over
it.  The genome readers are generators, so only one contig of a genome is in memory at a time.
"""
import struct

import numpy as np

TWOBIT_MAGIC = 0x1A412743
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def _read_all(path_or_file):
    if hasattr(path_or_file, "read"):
        data = path_or_file.buffer.read() if hasattr(path_or_file, "buffer") else path_or_file.read()
        return data.encode() if isinstance(data, str) else bytes(data)
    with open(path_or_file, "rb") as f:
        return f.read()


def read_fasta(path_or_file):
    """Contigs of a plain-text FASTA file: ``>`` headers (the name is the header's first word),
    sequence lines of any length, ``\\n`` or ``\\r\\n``."""
    data = np.frombuffer(_read_all(path_or_file), dtype=np.uint8)
    if data.shape[0] == 0:
        return
    starts = np.flatnonzero(data == 10) + 1  # line starts
    starts = np.concatenate([[0], starts[starts < data.shape[0]]])
    heads = starts[data[starts] == ord(">")]
    if heads.shape[0] == 0 or np.any(~np.isin(data[:heads[0]], (10, 13, 32))):
        raise ValueError("not a FASTA file: sequence before the first '>' header")
    ends = np.concatenate([heads[1:], [data.shape[0]]])
    for h, e in zip(heads.tolist(), ends.tolist()):
        nl = np.flatnonzero(data[h:e] == 10)
        eol = h + int(nl[0]) if nl.shape[0] else e
        words = data[h + 1:eol].tobytes().decode("ascii", errors="replace").split()
        if not words:
            raise ValueError("FASTA header without a name")
        body = data[eol:e]
        yield words[0], np.ascontiguousarray(body[(body != 10) & (body != 13)])


_TWOBIT_LETTERS = np.frombuffer(b"TCAG", dtype=np.uint8)
# the four letters of every packed byte, first base in the two highest bits
_TWOBIT_LUT = _TWOBIT_LETTERS[(np.arange(256)[:, None] >> np.array([6, 4, 2, 0])[None, :]) & 3]


def read_2bit(path):
    """Contigs of a UCSC ``.2bit`` file, either byte order: packed bases T = 0, C = 1, A = 2,
    G = 3, four per byte; N blocks become ``N`` bytes; mask blocks (soft-masking) are ignored,
    so every base is upper case."""
    with open(path, "rb") as f:
        head = f.read(16)
        if len(head) < 16:
            raise ValueError("not a .2bit file: shorter than its header")
        for order in "<>":
            if struct.unpack(order + "I", head[:4])[0] == TWOBIT_MAGIC:
                break
        else:
            raise ValueError("not a .2bit file: bad signature")
        _, version, count, _ = struct.unpack(order + "4I", head)
        if version != 0:
            raise ValueError(f".2bit version {version} is not supported")
        index = []
        for _ in range(count):
            size = f.read(1)[0]
            name = f.read(size).decode("ascii")
            index.append((name, struct.unpack(order + "I", f.read(4))[0]))

        def words(n):
            return np.frombuffer(f.read(4 * n), dtype=order + "u4").astype(np.int64)

        for name, offset in index:
            f.seek(offset)
            dna_size, n_blocks = words(2).tolist()
            n_starts, n_sizes = words(n_blocks), words(n_blocks)
            mask_blocks = int(words(1)[0])
            f.seek(8 * mask_blocks + 4, 1)  # mask starts and sizes, the reserved word
            packed = np.frombuffer(f.read((dna_size + 3) // 4), dtype=np.uint8)
            if packed.shape[0] != (dna_size + 3) // 4:
                raise ValueError(f".2bit file ends inside contig {name}")
            seq = _TWOBIT_LUT[packed].reshape(-1)[:dna_size].copy()
            for s, length in zip(n_starts.tolist(), n_sizes.tolist()):
                seq[s:s + length] = ord("N")
            yield name, seq


def is_2bit(path):
    with open(path, "rb") as f:
        head = f.read(4)
    return len(head) == 4 and TWOBIT_MAGIC in (struct.unpack("<I", head)[0], struct.unpack(">I", head)[0])


def read_genome(path):
    """Contigs of a ``.2bit`` (by its signature) or FASTA file."""
    return read_2bit(path) if is_2bit(path) else read_fasta(path)


def merge_regions(regions):
    """0-based half-open intervals ``[m, 2]`` sorted, with overlapping and adjacent ones merged
    and empty ones dropped: no position is covered twice."""
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    if np.any(reg < 0) or np.any(reg[:, 0] > reg[:, 1]):
        raise ValueError("a region with a negative bound or start > end")
    reg = reg[reg[:, 0] < reg[:, 1]]
    if reg.shape[0] == 0:
        return np.zeros((0, 2), np.uint64)
    reg = reg[np.argsort(reg[:, 0], kind="stable")]
    reach = np.maximum.accumulate(reg[:, 1])
    first = np.concatenate([[True], reg[1:, 0] > reach[:-1]])  # starts a new merged run
    idx = np.flatnonzero(first)
    out = np.stack([reg[idx, 0], np.maximum.reduceat(reg[:, 1], idx)], axis=1)
    return out.astype(np.uint64)


def read_bed(path_or_file):
    """``chrom start end`` lines (extra columns ignored; ``#``, ``track`` and ``browser`` lines
    skipped) as ``{chrom: merged regions [m, 2]}``."""
    per = {}
    for line in _read_all(path_or_file).decode("ascii", errors="replace").splitlines():
        tok = line.split()
        if not tok or tok[0].startswith("#") or tok[0] in ("track", "browser"):
            continue
        if len(tok) < 3:
            raise ValueError(f"bad BED line:\n{line.strip()}")
        try:
            per.setdefault(tok[0], []).append((int(tok[1]), int(tok[2])))
        except ValueError:
            raise ValueError(f"bad BED line:\n{line.strip()}") from None
    return {name: merge_regions(v) for name, v in per.items()}


class Transcript:
    """The CDS of one transcript: ``name``, ``gene`` (or None), ``contig``, ``strand`` (0 = ``+``,
    1 = ``-``) and ``segments``, ascending 0-based half-open ``(begin, end)`` pairs."""

    def __init__(self, name, gene, contig, strand, segments):
        self.name, self.gene, self.contig, self.strand = name, gene, contig, strand
        self.segments = segments

    @property
    def length(self):
        return sum(e - b for b, e in self.segments)


def _transcripts(rows, what):
    """``rows``: ``(name, gene, contig, strand text, begin, end)`` in file order.  Transcripts in
    the order of their first line, segments sorted.  A transcript on two contigs or strands, or
    with overlapping segments, is a ValueError."""
    out = {}
    for name, gene, contig, strand, b, e in rows:
        if strand not in ("+", "-"):
            raise ValueError(f"{what}: transcript {name} has strand {strand!r}, not + or -")
        if b < 0 or b >= e:
            raise ValueError(f"{what}: transcript {name} has an empty or reversed segment {b} {e}")
        t = out.setdefault(name, Transcript(name, gene, contig, "+-".index(strand), []))
        if t.contig != contig:
            raise ValueError(f"{what}: transcript {name} lies on two contigs, {t.contig} and {contig}")
        if t.strand != "+-".index(strand):
            raise ValueError(f"{what}: transcript {name} lies on both strands")
        if t.gene is None:
            t.gene = gene
        t.segments.append((b, e))
    for t in out.values():
        t.segments.sort()
        for (_, e0), (b1, _) in zip(t.segments[:-1], t.segments[1:]):
            if b1 < e0:
                raise ValueError(f"{what}: transcript {t.name} has overlapping segments")
    return list(out.values())


def _gtf_attributes(text):
    out = {}
    for field in text.split(";"):
        tok = field.strip().split(None, 1)
        if len(tok) == 2:
            out.setdefault(tok[0], tok[1].strip().strip('"'))
    return out


def read_gtf_cds(path_or_file):
    """The ``CDS`` lines of a GTF file as :class:`Transcript` objects grouped by
    ``transcript_id``, in the order of their first line; ``gene`` is the ``gene_name`` attribute,
    or ``gene_id`` without one.  Coordinates are 1-based inclusive; the frame column is ignored;
    ``#`` lines and other features are skipped.  (GFF3 is not read.)"""
    rows = []
    for line in _read_all(path_or_file).decode("ascii", errors="replace").splitlines():
        if not line.strip() or line.startswith("#"):
            continue
        tok = line.rstrip("\r\n").split("\t")
        if len(tok) < 9:
            raise ValueError(f"bad GTF line (nine tab-separated columns):\n{line.strip()}")
        if tok[2] != "CDS":
            continue
        attr = _gtf_attributes(tok[8])
        if "transcript_id" not in attr:
            raise ValueError(f"a CDS line without a transcript_id:\n{line.strip()}")
        try:
            b, e = int(tok[3]) - 1, int(tok[4])
        except ValueError:
            raise ValueError(f"bad GTF line:\n{line.strip()}") from None
        rows.append((attr["transcript_id"], attr.get("gene_name", attr.get("gene_id")), tok[0], tok[6], b, e))
    return _transcripts(rows, "GTF")


def read_cds_bed(path_or_file):
    """BED6 lines, one per CDS segment: column 4 the transcript's name, column 6 its strand
    (0-based half-open coordinates; ``#``, ``track`` and ``browser`` lines skipped)."""
    rows = []
    for line in _read_all(path_or_file).decode("ascii", errors="replace").splitlines():
        tok = line.split()
        if not tok or tok[0].startswith("#") or tok[0] in ("track", "browser"):
            continue
        if len(tok) < 6:
            raise ValueError(f"bad BED6 line (chrom start end name score strand):\n{line.strip()}")
        try:
            rows.append((tok[3], None, tok[0], tok[5], int(tok[1]), int(tok[2])))
        except ValueError:
            raise ValueError(f"bad BED6 line:\n{line.strip()}") from None
    return _transcripts(rows, "BED")


def fold_type(ref, alt):
    """``REF>ALT`` on the strand where REF is A or C: ``G>A`` is ``C>T``."""
    ref, alt = ref.upper(), alt.upper()
    if ref in "GT":
        ref, alt = _COMPLEMENT[ref], _COMPLEMENT[alt]
    return f"{ref}>{alt}"


def parse_type(text):
    """A ``--type`` argument ``X>Y`` (two different bases), folded."""
    part = text.upper().split(">")
    if len(part) != 2 or any(len(x) != 1 or x not in _COMPLEMENT for x in part) or part[0] == part[1]:
        raise ValueError(f"mutation type must be X>Y with two different bases of ACGT, not {text!r}")
    return fold_type(*part)


def read_sites(path_or_file, kind=None):
    """``CHROM POS REF ALT`` lines (1-based POS; further columns are ignored, ``#`` lines
    skipped; a VCF's ID column has to be cut out first).  Only single-base ``ACGT`` REF != ALT lines are
    sites; with ``kind`` (:func:`parse_type`) only those whose folded REF>ALT equals it.
    Returns ``({chrom: (pos0 uint64 [m], ref uint8 [m])}, stats)``, positions 0-based in file
    order, ``stats`` counting ``lines``, ``not_snv`` and ``other_type``."""
    per = {}
    stats = {"lines": 0, "not_snv": 0, "other_type": 0}
    for line in _read_all(path_or_file).decode("ascii", errors="replace").splitlines():
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
        stats["lines"] += 1
        ref, alt = tok[2].upper(), tok[3].upper()
        if len(ref) != 1 or len(alt) != 1 or ref not in _COMPLEMENT or alt not in _COMPLEMENT or ref == alt:
            stats["not_snv"] += 1
            continue
        if kind is not None and fold_type(ref, alt) != kind:
            stats["other_type"] += 1
            continue
        pl, rl = per.setdefault(tok[0], ([], []))
        pl.append(pos - 1)
        rl.append(ord(ref))
    return {name: (np.array(p, np.uint64), np.array(r, np.uint8)) for name, (p, r) in per.items()}, stats


def read_sites_alt(path_or_file):
    """:func:`read_sites` without a type filter that also returns ALT: ``({chrom: (pos0 uint64
    [m], ref uint8 [m], alt uint8 [m])}, stats)``, upper-case bytes, positions in file order.
    ``stats`` counts ``lines``, ``not_snv`` and, of those, ``alt_equals_ref``: the lines whose REF
    and ALT are the same single base."""
    per = {}
    stats = {"lines": 0, "not_snv": 0, "alt_equals_ref": 0}
    for line in _read_all(path_or_file).decode("ascii", errors="replace").splitlines():
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
        stats["lines"] += 1
        ref, alt = tok[2].upper(), tok[3].upper()
        if len(ref) != 1 or len(alt) != 1 or ref not in _COMPLEMENT or alt not in _COMPLEMENT or ref == alt:
            stats["not_snv"] += 1
            stats["alt_equals_ref"] += len(ref) == 1 and ref == alt and ref in _COMPLEMENT
            continue
        pl, rl, al = per.setdefault(tok[0], ([], [], []))
        pl.append(pos - 1)
        rl.append(ord(ref))
        al.append(ord(alt))
    return {name: (np.array(p, np.uint64), np.array(r, np.uint8), np.array(a, np.uint8))
            for name, (p, r, a) in per.items()}, stats


def trim_alleles(ref, alt):
    """REF and ALT without their longest common prefix and then, of what is left, their longest
    common suffix: ``(prefix length, ref, alt)``."""
    q = 0
    while q < len(ref) and q < len(alt) and ref[q] == alt[q]:
        q += 1
    ref, alt = ref[q:], alt[q:]
    t = 0
    while t < len(ref) and t < len(alt) and ref[-1 - t] == alt[-1 - t]:
        t += 1
    return q, ref[:len(ref) - t], alt[:len(alt) - t]


class IndelSites:
    """The indels of one contig in file order: 0-based ``pos`` (the breakpoint of an insertion, the
    first deleted base of a deletion), ``del_len`` (0 = an insertion), the inserted strings as one
    upper-case pool ``ins`` with offsets ``ins_off`` ``[m + 1]``, ``key`` (the 0-based number of the
    site's line in its file) and, for :func:`match_indel_ref`, the whole REF as spelled: ``ref``
    pool, ``ref_off`` ``[m + 1]`` and its 0-based position ``ref_pos``."""

    def __init__(self, pos, del_len, ins, ins_off, key, ref_pos, ref, ref_off):
        self.pos, self.del_len, self.ins, self.ins_off, self.key = pos, del_len, ins, ins_off, key
        self.ref_pos, self.ref, self.ref_off = ref_pos, ref, ref_off

    def __len__(self):
        return self.pos.shape[0]

    def arrays(self):
        """What ``engine.Device.seq_indels`` takes."""
        return self.pos, self.del_len, self.ins, self.ins_off, self.key

    def take(self, keep):
        """The sites where the bool array ``keep`` is set."""
        def pool(data, off):
            off = off.astype(np.int64)
            lens = (off[1:] - off[:-1])[keep]
            idx = np.repeat(off[:-1][keep], lens) + (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens))
            return data[idx], np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)

        ins, ins_off = pool(self.ins, self.ins_off)
        ref, ref_off = pool(self.ref, self.ref_off)
        return IndelSites(self.pos[keep], self.del_len[keep], ins, ins_off, self.key[keep], self.ref_pos[keep], ref, ref_off)


def read_indels(path_or_file):
    """``CHROM POS REF ALT`` lines (1-based POS; further columns ignored, ``#`` lines skipped; ``-``
    or ``.`` spells an empty allele) that are short insertions or deletions.  REF and ALT lose their
    longest common prefix, then the longest common suffix of the rest (:func:`trim_alleles`);
    exactly one of them must be empty afterwards: an insertion of ALT before the base POS + prefix,
    or a deletion of REF from there.  Everything else is counted and dropped: ``not_indel`` (an SNV,
    REF == ALT, a symbolic or comma-separated ALT, a letter other than ACGT in an insertion or in
    either allele's spelling) or ``complex`` (both left non-empty: MNVs and delins).
    Returns ``({chrom: IndelSites}, stats)``, ``stats`` counting ``lines``, ``not_indel`` and
    ``complex``.  A site's key is the 0-based number of its line in the file (every line counts)."""
    per = {}
    stats = {"lines": 0, "not_indel": 0, "complex": 0}
    for number, line in enumerate(_read_all(path_or_file).decode("ascii", errors="replace").splitlines()):
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
        stats["lines"] += 1
        ref, alt = ("" if x in ("-", ".") else x.upper() for x in tok[2:4])
        if any(c not in _COMPLEMENT for c in ref + alt):  # (symbolic <DEL>, *, commas, IUPAC letters)
            stats["not_indel"] += 1
            continue
        q, r, a = trim_alleles(ref, alt)
        if r and a:
            stats["not_indel" if len(r) == 1 and len(a) == 1 else "complex"] += 1
            continue
        if not r and not a:
            stats["not_indel"] += 1
            continue
        lists = per.setdefault(tok[0], ([], [], [], [], [], []))
        for lst, v in zip(lists, (pos - 1 + q, len(r), a, number, pos - 1, ref)):
            lst.append(v)
    out = {}
    for name, (p, dl, ins, key, rp, ref) in per.items():
        def pool(strings):
            off = np.concatenate([[0], np.cumsum([len(x) for x in strings])]).astype(np.uint64)
            return np.frombuffer("".join(strings).encode("ascii"), np.uint8), off

        out[name] = IndelSites(np.array(p, np.uint64), np.array(dl, np.uint64), *pool(ins), np.array(key, np.uint64),
                               np.array(rp, np.uint64), *pool(ref))
    return out, stats


def match_indel_ref(seq, sites):
    """The :class:`IndelSites` that lie on the contig ``seq`` and whose whole REF equals the contig
    there case-insensitively: ``(kept sites, n_off_contig, n_ref_mismatch)``.  A site is off the
    contig if its REF, its breakpoint or its deleted bases reach past the end."""
    n = np.uint64(seq.shape[0])
    ref_len = sites.ref_off[1:] - sites.ref_off[:-1]
    on = (sites.ref_pos + ref_len <= n) & (sites.pos + sites.del_len <= n)
    lens = np.where(on, ref_len, np.uint64(0)).astype(np.int64)  # (a site off the contig compares nothing)
    start = np.cumsum(lens) - lens
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(start, lens)
    at = np.repeat(sites.ref_pos.astype(np.int64), lens) + within
    want = sites.ref[np.repeat(sites.ref_off[:-1].astype(np.int64), lens) + within]
    wrong = np.concatenate([[0], np.cumsum((seq[at] & 0xDF) != want)])
    same = wrong[start + lens] == wrong[start]
    return sites.take(on & same), int((~on).sum()), int((on & ~same).sum())


def match_ref(seq, pos, ref):
    """The positions of ``pos`` that lie on the contig ``seq`` and whose base there equals
    ``ref`` case-insensitively: ``(kept positions, n_off_contig, n_ref_mismatch)``."""
    on = pos < np.uint64(seq.shape[0])
    pos_on, ref_on = pos[on], ref[on]
    same = (seq[pos_on.astype(np.intp)] & 0xDF) == ref_on
    return pos_on[same], int((~on).sum()), int((~same).sum())
