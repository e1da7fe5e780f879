"""An independent oracle for the k-mer context counts (kmerpapa_amd.count, kp_seq.h): a plain
Python loop over windows with string slicing, a complement dictionary and collections.Counter.
It shares no code with the library.  Also the small .2bit writer the reader tests need."""
import struct
from collections import Counter

import numpy as np

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}
COUNT_STATS = ("windows", "windows_invalid", "sites", "sites_skipped")


def revcomp(kmer):
    return "".join(COMPLEMENT[c] for c in reversed(kmer))


def text(seq):
    return seq if isinstance(seq, str) else bytes(np.asarray(seq, np.uint8)).decode("latin-1")


def window(seq, centre, k, fold):
    """The k-mer counted for the window centred at ``centre``: "off" if it leaves the contig,
    None if it holds an invalid byte."""
    start = centre - k // 2
    if start < 0 or start + k > len(seq):
        return "off"
    w = seq[start:start + k].upper()
    if any(c not in COMPLEMENT for c in w):
        return None
    if fold and w[k // 2] in "GT":
        w = revcomp(w)
    return w


def count(k, fold, jobs):
    """``jobs``: ``(seq, regions, sites)`` per contig, as engine.Device.seq_count takes them
    (regions None = whole contig, False = no scan; they may overlap: a centre counts once).
    Returns ``(pos Counter, bg Counter, stats)``."""
    pos, bg = Counter(), Counter()
    st = dict.fromkeys(COUNT_STATS, 0)
    for seq, regions, sites in jobs:
        seq = text(seq)
        if regions is not False:
            centres = set(range(len(seq)))
            if regions is not None:
                centres = set()
                for b, e in regions:
                    centres.update(range(int(b), int(e)))
            for c in sorted(centres):
                w = window(seq, c, k, fold)
                if w is None:
                    st["windows_invalid"] += 1
                elif w != "off":
                    bg[w] += 1
                    st["windows"] += 1
        for p in ([] if sites is None else sites):
            w = window(seq, int(p), k, fold)
            if w is None or w == "off":
                st["sites_skipped"] += 1
            else:
                pos[w] += 1
                st["sites"] += 1
    return pos, bg, st


def dense(counter, k):
    """A Counter of k-mers as the dense uint64 table in code order."""
    out = np.zeros(4 ** k, np.uint64)
    for kmer, c in counter.items():
        code = 0
        for ch in kmer:
            code = 4 * code + "ACGT".index(ch)
        out[code] = c
    return out


def kmer_of(code, k):
    return "".join("ACGT"[(code >> (2 * (k - 1 - i))) & 3] for i in range(k))


def random_seq(rng, n, lower=0.0, invalid=0.0, letters="ACGT"):
    """``n`` random bases as a uint8 array; a share ``lower`` of them lower case and a share
    ``invalid`` replaced by bytes that are no bases."""
    seq = np.frombuffer(letters.encode(), np.uint8)[rng.randint(0, len(letters), size=n)].copy()
    seq[rng.random_sample(n) < lower] |= 0x20
    bad = np.flatnonzero(rng.random_sample(n) < invalid)
    seq[bad] = np.frombuffer(b"NnRYKM-*.x\x00\xff", np.uint8)[rng.randint(0, 12, size=bad.shape[0])]
    return seq


def _runs(flags):
    """(start, length) of every run of True."""
    f = np.concatenate([[False], np.asarray(flags, bool), [False]])
    edge = np.flatnonzero(f[1:] != f[:-1])
    return [(int(s), int(e - s)) for s, e in zip(edge[0::2], edge[1::2])]


def write_2bit(path, contigs, order="<"):
    """Write ``(name, uint8 array)`` contigs as a UCSC .2bit file in byte order ``order``: runs of
    bytes that are no bases become N blocks, lower-case runs mask blocks."""
    packed_of = {ord("T"): 0, ord("C"): 1, ord("A"): 2, ord("G"): 3}
    records = []
    for name, seq in contigs:
        seq = np.asarray(seq, np.uint8)
        up = seq & 0xDF
        digit = np.zeros(seq.shape[0] + (-seq.shape[0]) % 4, np.uint8)
        isbase = np.zeros(seq.shape[0], bool)
        for letter, d in packed_of.items():
            digit[:seq.shape[0]][up == letter] = d
            isbase |= up == letter
        q = digit.reshape(-1, 4)
        packed = ((q[:, 0] << 6) | (q[:, 1] << 4) | (q[:, 2] << 2) | q[:, 3]).astype(np.uint8).tobytes()
        nb = _runs(~isbase)
        mb = _runs(isbase & ((seq & 0x20) != 0))
        rec = struct.pack(order + "II", seq.shape[0], len(nb))
        rec += struct.pack(order + f"{len(nb)}I", *[s for s, _ in nb]) + struct.pack(order + f"{len(nb)}I", *[n for _, n in nb])
        rec += struct.pack(order + "I", len(mb))
        rec += struct.pack(order + f"{len(mb)}I", *[s for s, _ in mb]) + struct.pack(order + f"{len(mb)}I", *[n for _, n in mb])
        rec += struct.pack(order + "I", 0) + packed
        records.append((name.encode("ascii"), rec))
    offset = 16 + sum(1 + len(name) + 4 for name, _ in records)
    with open(path, "wb") as f:
        f.write(struct.pack(order + "4I", 0x1A412743, 0, len(records), 0))
        for name, rec in records:
            f.write(bytes([len(name)]) + name + struct.pack(order + "I", offset))
            offset += len(rec)
        for _, rec in records:
            f.write(rec)


def write_fasta(path, contigs, width=60, newline="\n"):
    with open(path, "w", newline="", encoding="latin-1") as f:
        for name, seq in contigs:
            s = text(seq)
            f.write(f">{name} some description{newline}")
            for i in range(0, len(s), width):
                f.write(s[i:i + width] + newline)
