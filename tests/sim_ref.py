"""An independent oracle for kp_spec_simulate (kp_sim.h): Philox4x32-10 on Python integers, the
pattern ids of a position from tests.spec_ref.track, the cumulative pick and the un-folding of
ALT written out directly.  It shares no code with the library or with kmerpapa_amd.engine."""
import numpy as np

from tests import spec_ref as R

M32 = 0xFFFFFFFF
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def philox(counter, key):
    """Philox4x32 with 10 rounds: ``counter`` four and ``key`` two 32-bit integers."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform(seed, contig_id, pos, replicate):
    x = philox((pos & M32, pos >> 32, contig_id, replicate), (seed & M32, seed >> 32))
    return float(((x[1] << 32 | x[0]) >> 11)) * 2.0 ** -53  # (an integer below 2^53: exact)


def cumulative(ids, rates, scale):
    """``(c0, c1, c2)`` of a position's three pattern ids."""
    r = [float(rates[i]) * float(scale) if i >= 0 else 0.0 for i in ids]
    c0 = r[0]
    c1 = c0 + r[1]
    c2 = c1 + r[2]
    return c0, c1, c2


def forward_alt(base, slot, fold):
    """The ALT letter on the forward strand of slot ``slot`` at a position whose base is ``base``."""
    base = base.upper()
    flipped = fold and base in "GT"
    ref = COMPLEMENT[base] if flipped else base
    alt = [b for b in "ACGT" if b != ref][slot]
    return COMPLEMENT[alt] if flipped else alt


def simulate(seq, names, ptype, rates, fold, regions, seed, contig_id=0, replicate=0, scale=1.0, pid=None):
    """``(pos uint64, alt uint8, pid int32, windows)`` of kp_spec_simulate over ``regions``
    (ascending, disjoint).  ``pid``: the whole contig's ``spec_ref.track``, if the caller has it."""
    text = R.text(seq)
    if pid is None:
        pid = R.track(text, names, ptype, fold)
    pos, alt, out, windows = [], [], [], 0
    for b, e in regions:
        for p in range(int(b), int(e)):
            ids = [int(pid[s, p]) for s in range(3)]
            if ids[0] == R.INVALID:
                continue
            windows += 1
            c0, c1, c2 = cumulative(ids, rates, scale)
            u = uniform(seed, contig_id, p, replicate)
            slot = 0 if u < c0 else 1 if u < c1 else 2 if u < c2 else None
            if slot is not None:
                pos.append(p)
                alt.append(ord(forward_alt(text[p], slot, fold)))
                out.append(ids[slot])
    return np.array(pos, np.uint64), np.array(alt, np.uint8), np.array(out, np.int32), windows
