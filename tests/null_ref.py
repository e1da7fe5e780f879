"""An independent oracle for kp_spec_null (kp_null.h): per replicate the whole contig's mutation set
from tests.sim_ref.simulate, binned by region with searchsorted (and by the type of the hit's
pattern for the typed table).  It shares no code with the library or with kmerpapa_amd.engine.
Pure Python per position and replicate: a few thousand positions times a few replicates."""
import numpy as np

from tests import sim_ref as S
from tests import spec_ref as R


def uniforms(seed, contig_id, pos, reps):
    """float64 ``[len(pos), len(reps)]``: ``sim_ref.uniform`` of every (position, replicate) pair,
    Philox4x32-10 written out on numpy uint64 (a product of two 32-bit words fits)."""
    m32 = np.uint64(0xFFFFFFFF)
    pos = np.asarray(pos, np.uint64).reshape(-1, 1)
    c0, c1 = pos & m32, pos >> np.uint64(32)
    c2 = np.full_like(pos, contig_id)
    c3 = np.asarray(reps, np.uint64).reshape(1, -1)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return (((c1 << np.uint64(32)) | c0) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def table(seq, names, ptype, rates, fold, regions, seed, contig_id=0, rep_first=0, n_reps=1, scale=1.0, by_type=False,
          pid=None):
    """uint32 ``[m, n_reps]`` (``[m, n_reps, 12]`` with ``by_type``) of kp_spec_null over
    ``regions`` (any order, overlapping or not).  ``pid``: the contig's ``spec_ref.track``."""
    if pid is None:
        pid = R.track(R.text(seq), names, ptype, fold)
    reg = np.asarray(regions, np.int64).reshape(-1, 2)
    ptype = np.asarray(ptype, np.int64)
    out = np.zeros((reg.shape[0], n_reps, 12), np.uint32)
    for j in range(n_reps):
        pos, _, hit_pid, _ = S.simulate(seq, names, ptype, rates, fold, [(0, len(seq))], seed, contig_id, rep_first + j, scale,
                                        pid=pid)
        pos = pos.astype(np.int64)
        kinds = ptype[hit_pid]
        for t in range(12):
            own = pos[kinds == t]  # (ascending, as pos is)
            out[:, j, t] = np.searchsorted(own, reg[:, 1], "left") - np.searchsorted(own, reg[:, 0], "left")
    return out if by_type else out.sum(axis=2, dtype=np.uint32)
