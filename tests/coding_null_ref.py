"""An independent oracle for kp_spec_coding_null (kp_cnull.h), written from the definition in
include/kmerpapa_hip.h: per replicate tests.sim_ref.simulate draws the whole contig's mutation set,
tests.coding_ref.coding_sites classes every (hit, transcript) pair, and numpy adds the classes up.
It shares no code with the library or with kmerpapa_amd.engine."""
import numpy as np

from tests import coding_ref as C
from tests import sim_ref as S
from tests import spec_ref as R


def positions_of(transcripts, splice):
    """Per transcript its coding and essential splice positions, each once."""
    out = []
    for _, segs in transcripts:
        segs = [(int(b), int(e)) for b, e in segs]
        out.append([g for b, e in segs for g in range(b, e)] + C.splice_positions(segs, splice))
    return out


def table(seq, names, ptype, rates, fold, transcripts, splice, seed, contig_id=0, first=0, reps=1, scale=1.0):
    """``(counts uint32 [T, reps, 5], stats)`` of kp_spec_coding_null; ``stats``: ``positions``,
    ``drawing``, ``hits`` and ``unclassed`` as kp_spec_last_coding_null gives them."""
    n, T = len(seq), len(transcripts)
    counts = np.zeros((T, reps, 5), np.uint32)
    track = R.track(seq, names, ptype, fold)
    where = positions_of(transcripts, splice)
    rated = np.zeros(n, bool)  # a valid window and c2 > 0
    for slot in range(3):
        ids = track[slot]
        rated |= (ids >= 0) & (np.asarray(rates, np.float64)[np.maximum(ids, 0)] * float(scale) > 0.0)
    stats = {"positions": sum(len(w) for w in where), "drawing": sum(int(rated[w].sum()) for w in where if w),
             "hits": 0, "unclassed": 0}
    for j in range(reps):
        pos, alt, _, _ = S.simulate(seq, names, ptype, rates, fold, [[0, n]], seed, contig_id, first + j, scale, pid=track)
        if not len(pos) or not T:
            continue
        hp = np.repeat(pos, T)
        ha = np.repeat(alt, T)
        ht = np.tile(np.arange(T, dtype=np.uint32), len(pos))
        cls, _, _ = C.coding_sites(seq, names, ptype, fold, transcripts, splice, hp, ha, ht)
        assert not (cls == C.ALT_IS_REF).any()
        ok = cls >= 0
        np.add.at(counts, (ht[ok], j, cls[ok]), 1)
        stats["unclassed"] += int((cls == C.NO_CLASS).sum())
    stats["hits"] = int(counts.sum())
    return counts, stats
