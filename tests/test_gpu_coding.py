"""Coding consequences on the GPU (kp_coding_scan_kernel, kp_coding_sites_kernel) against the host
session of the same per-pair functions (engine.HostSpec, itself pinned to an independent oracle in
tests/test_coding.py).  Bar: ``hist``, ``other``, ``cls``, ``pid`` and ``codons`` equal, ``expected``
bit for bit, and equal ``items``, ``positions`` and ``pairs``, for every knob.

Every device call goes through the ``_guard`` of tests/test_gpu_simulate.py: after a HIP error (a
fault included) every later test fails before it starts anything on the GPU."""
import numpy as np
import pytest

from kmerpapa_amd import engine
from tests import coding_cases as K
from tests import spec_ref as R
from tests.test_gpu_simulate import _guard

pytestmark = pytest.mark.gpu

KNOBS = ("KP_CODING_GRID", "KP_CODING_GLOBAL", "KP_CODING_LDS_P", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
ENVS = [{}, {"KP_CODING_GRID": 1}, {"KP_CODING_GRID": 3}, {"KP_CODING_GLOBAL": 1}, {"KP_CODING_LDS_P": 0}]
ENV_IDS = ["default", "one_workgroup", "three", "global", "lds_p_0"]
LDS_P = 65536 // 20  # most patterns with LDS counters


@pytest.fixture(scope="module")
def dev():
    with _guard():
        engine.load()
        assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
        return engine.get_device(engine.visible_devices()[0])


@pytest.fixture(scope="module")
def tile(dev):
    with _guard():
        dev.spec_begin(1, [K.word("A")], [0], False)
        dev.spec_end()
        return dev.spec_stats()["tile"]


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


def _session(s, k, fold, jobs, leaves=6):
    """One session over ``jobs`` = ``(seq, transcripts, splice)``: the results of each, and the
    path of the last kp_spec_coding call."""
    _, words, ptype, rates = K.model(k, fold, leaves)
    out = []
    with _guard():
        s.spec_begin(k, words, ptype, fold)
        try:
            for seq, txs, splice in jobs:
                out.append(K.run(s, seq, txs, splice, rates))
            path = s.spec_coding_stats()["path"]
        finally:
            s.spec_end()
    return out, path


_host_cache = {}


def _host(key, k, fold, jobs, leaves=6):
    """The host session of a case, computed once and shared by the knobs."""
    if key not in _host_cache:
        _host_cache[key] = _session(engine.HostSpec(), k, fold, jobs, leaves)[0]
    return _host_cache[key]


def _compare(dev, key, k, fold, jobs, leaves=6, path=engine.SPEC_PATH_LDS):
    got, took = _session(dev, k, fold, jobs, leaves)
    ref = _host(key, k, fold, jobs, leaves)
    assert took == path
    for g, r, (_, txs, splice) in zip(got, ref, jobs):
        K.same(g, r)
        K.check_identities(g, txs, splice)
    return got


@pytest.mark.parametrize("k,fold", K.KSETS)
def test_small_cases(dev, monkeypatch, k, fold):
    """The cases of tests/test_coding.py: the class table, every segment split and intron length,
    invalid bytes, the contig's ends and overlapping transcripts, for splice 0, 2 and 8."""
    _set(monkeypatch, {})
    jobs = [(seq, txs, splice) for seq, txs in K.small_cases().values() for splice in K.SPLICES]
    _compare(dev, ("small", k, fold), k, fold, jobs)


def _rseq(n, seed):
    return R.random_seq(np.random.RandomState(seed), n, lower=0.25)


def _tile_case(tile, start, k):
    """A segment of tile + 35 bases whose spliced start is ``start`` modulo 3, on both strands: its
    codons cross every thread-run boundary and the boundary of its two work items; invalid bytes
    next to both."""
    long = tile + 35
    last = 1 + (-(start + long + 1)) % 3
    seq = _rseq(tile + 200, seed=start)
    segs = [(20, 20 + start), (60, 60 + long), (60 + long + 30, 60 + long + 30 + last)]
    run = tile // 256
    for p in (60 + k // 2 + 5 * run + 1, 60 + tile - 1, 60 + tile + 2):
        seq[p] = ord("N")
    return seq, [(0, segs), (1, segs)]


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
@pytest.mark.parametrize("k,fold", [(3, True), (7, True), (4, False)])
def test_codons_across_runs_and_items(dev, tile, monkeypatch, env, k, fold):
    _set(monkeypatch, env)
    jobs = [_tile_case(tile, start, k) + (2,) for start in (1, 2)]
    lds = not ("KP_CODING_GLOBAL" in env or "KP_CODING_LDS_P" in env)
    got = _compare(dev, ("tile", k, fold), k, fold, jobs, path=engine.SPEC_PATH_LDS if lds else engine.SPEC_PATH_GLOBAL)
    assert got[0]["counts"][0] == 2 * (1 + 2 + 1 + 2 + 2)  # the long segment is two items; two introns of two intervals


@pytest.mark.parametrize("k,fold", [(1, True), (7, True), (4, False)])
def test_segments_at_the_contig_ends(dev, monkeypatch, k, fold):
    """Segments within k / 2 of both ends: centres whose window leaves the contig are the host's."""
    _set(monkeypatch, {})
    seq = _rseq(40, seed=k)
    jobs = []
    for d in range(0, k // 2 + 2):
        segs = [(d, d + 3), (40 - d - 3, 40 - d)]
        jobs.append((seq, [(0, segs), (1, segs), (0, [(0, 3), (3, 6)]), (1, [(34, 40)])], 2))
    got = _compare(dev, ("ends", k, fold), k, fold, jobs)
    if k > 1:
        assert got[0]["other"][:, 5].min() > 0  # pairs with a class and no window


@pytest.mark.parametrize("env", ENVS, ids=ENV_IDS)
@pytest.mark.parametrize("k,fold", [(5, True), (4, False)])
def test_random_transcripts(dev, monkeypatch, env, k, fold):
    """300 random transcripts on a 20,000-base contig, on both strands, overlapping."""
    _set(monkeypatch, env)
    seq, txs = K.random_case(3, 20000, 300)
    lds = not ("KP_CODING_GLOBAL" in env or "KP_CODING_LDS_P" in env)
    got = _compare(dev, ("random", k, fold), k, fold, [(seq, txs, 2)],
                   path=engine.SPEC_PATH_LDS if lds else engine.SPEC_PATH_GLOBAL)
    o = got[0]["other"].sum(axis=0)
    assert o[:5].min() > 0 and o[6] > 0 and o[7] > 0  # every class, pairs without a pattern, positions without a class


def test_more_patterns_than_lds_counters(dev, monkeypatch):
    """A model whose 5 P counters do not fit 64 KiB takes global atomics and gives the same."""
    _set(monkeypatch, {})
    k, fold, leaves = 7, True, 700
    assert len(K.model(k, fold, leaves)[0]) > LDS_P
    seq, txs = K.random_case(4, 6000, 60)
    _compare(dev, ("big", k, fold), k, fold, [(seq, txs, 2)], leaves, path=engine.SPEC_PATH_GLOBAL)


def test_regions_after_coding_in_one_session(dev, monkeypatch):
    """The lookup table survives a kp_spec_coding call: a kp_spec_regions call after it equals the
    host's."""
    _set(monkeypatch, {})
    k, fold = 5, True
    _, words, ptype, rates = K.model(k, fold)
    seq, txs = K.random_case(5, 5000, 40)
    regions = np.array([(0, 5000), (100, 2300), (4990, 5000)], np.uint64)
    res = []
    for s in (dev, engine.HostSpec()):
        with _guard():
            s.spec_begin(k, words, ptype, fold)
            try:
                first = s.spec_regions(seq, regions, rates)
                coding = K.run(s, seq, txs, 2, rates)
                res.append((first, coding, s.spec_regions(seq, regions, rates)))
            finally:
                s.spec_end()
    (d0, dc, d1), (h0, hc, h1) = res
    K.same(dc, hc)
    for d, h in ((d0, h0), (d1, h1)):
        assert np.array_equal(d[0], h[0]) and np.array_equal(d[1], h[1]) and np.array_equal(K.bits(d[2]), K.bits(h[2]))
