"""Null tables built on the GPU (kp_null_kernel) against the host session of the same per-window
functions (engine.HostSpec, itself pinned to an independent oracle in tests/test_null.py).  Bar: the
table byte for byte, and equal ``windows``, ``draws``, ``hits`` and ``items``, for every grid and
every replicate chunk.  The host computes a case's table once with the most replicates the case
uses; fewer replicates are its leading columns (the identity tests/test_null.py checks).

The contigs, models and the guard are tests/test_gpu_simulate.py's: a HIP error (a fault included)
in either file is recorded and every later test of both fails before it starts anything on the
GPU."""
import numpy as np
import pytest

from kmerpapa_amd import engine, spectrum
from tests import spec_ref as R
from tests.test_gpu_simulate import THREADS, _contig, _guard, _model, dev, tile  # noqa: F401 (dev, tile: fixtures)

pytestmark = pytest.mark.gpu

KNOBS = ("KP_NULL_REPS", "KP_NULL_GRID", "KP_SIM_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
UNTYPED_MAX, TYPED_MAX = 3072, 256  # replicates of a chunk at most (include/kmerpapa_hip.h)


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


class _session:
    def __init__(self, s, k, fold, model):
        self.s, self.args = s, (k, model[0], model[1], fold)

    def __enter__(self):
        self.guard = _guard()
        self.guard.__enter__()
        self.s.spec_begin(*self.args)
        return self.s

    def __exit__(self, *exc):
        try:
            self.s.spec_end()
        finally:
            self.guard.__exit__(*exc)


def _null(s, seq, regions, rates, n_reps, by_type, first=3, seed=5, contig_id=1, scale=1.0):
    """One call in the open session: (table, stats)."""
    with _guard():
        got = s.spec_null(seq, regions, rates, seed, contig_id, first, n_reps, scale, by_type)
        return got, s.spec_null_stats()


_host_cache = {}


def _host(key, k, fold, model, seq, regions, n_reps, **kw):
    """The host session's typed table of a case with ``n_reps`` replicates, computed once."""
    if key not in _host_cache:
        with _session(engine.HostSpec(), k, fold, model) as s:
            _host_cache[key] = _null(s, seq, regions, model[2], n_reps, True, **kw)
    assert _host_cache[key][0].shape[1] == n_reps
    return _host_cache[key]


def _same(got, ref, n_reps, by_type):
    """``got`` = (table, stats) of ``n_reps`` replicates, ``ref`` the host's typed one of at least as many."""
    want = ref[0][:, :n_reps] if by_type else ref[0][:, :n_reps].sum(axis=2, dtype=np.uint32)
    assert got[0].dtype == np.uint32 and got[0].shape == want.shape and got[0].tobytes() == want.tobytes()
    assert got[1]["windows"] == ref[1]["windows"] and got[1]["items"] == ref[1]["items"]
    assert got[1]["draws"] * ref[0].shape[1] == ref[1]["draws"] * n_reps and got[1]["hits"] == int(want.sum())


@pytest.mark.parametrize("env", [{}, {"KP_NULL_GRID": 1}, {"KP_NULL_GRID": 3}], ids=["default", "one_workgroup", "three"])
@pytest.mark.parametrize("k,fold", [(3, True), (3, False), (5, True), (5, False)])
def test_contig_lengths_around_the_tile(dev, tile, monkeypatch, env, k, fold):
    """Dense rates on contigs of tile - 1, tile, tile + 1 and 2 tile + 5 bases and one shorter than
    k; 1, 63, 64, 65 and 130 replicates: whole and partial groups of 64 lanes."""
    _set(monkeypatch, env)
    model = _model(k, fold, "dense")
    with _session(dev, k, fold, model) as s:
        for n in (tile - 1, tile, tile + 1, 2 * tile + 5, k - 1):
            seq = _contig(n, tile, k, seed=n % 97)
            ref = _host(("len", k, fold, n), k, fold, model, seq, [(0, n)], 130)
            for n_reps in (1, 63, 64, 65, 130):
                for by_type in (False, True):
                    got = _null(s, seq, [(0, n)], model[2], n_reps, by_type)
                    _same(got, ref, n_reps, by_type)
                    if n >= k:
                        assert got[1]["null_ms"] > 0 and got[1]["passes"] == 1 and got[1]["reps_per_pass"] == n_reps
                    else:
                        assert got[1]["null_ms"] == 0 and got[1]["items"] == got[1]["hits"] == 0
            if n >= k:
                assert ref[1]["items"] == -(-(n - k + 1) // tile) and 0 < ref[1]["hits"] < ref[1]["draws"]
                assert ref[0][0].sum(axis=1).min() > n // 100  # every replicate has hits


@pytest.mark.parametrize("by_type", [False, True], ids=["total", "by_type"])
@pytest.mark.parametrize("reps", [1, 3, 64])
def test_replicate_chunks(dev, tile, monkeypatch, reps, by_type):
    """KP_NULL_REPS = 1, 3, 64 with 1, 4, 65 and 130 replicates: several passes over an item, a
    partial last chunk and partial last lanes."""
    _set(monkeypatch, {"KP_NULL_REPS": reps})
    k, fold = 5, True
    model = _model(k, fold, "dense")
    n = 2 * tile + 5
    seq = _contig(n, tile, k, seed=n % 97)
    regions = [(0, n), (tile // 2, tile + 77)]
    ref = _host(("chunks", n), k, fold, model, seq, regions, 130)
    with _session(dev, k, fold, model) as s:
        for grid in (0, 2):
            monkeypatch.setenv("KP_NULL_GRID", str(grid))
            for n_reps in (1, 4, 65, 130):
                got = _null(s, seq, regions, model[2], n_reps, by_type)
                _same(got, ref, n_reps, by_type)
                per = min(n_reps, reps)
                assert got[1]["reps_per_pass"] == per and got[1]["passes"] == -(-n_reps // per)


def test_the_largest_chunks(dev, tile, monkeypatch):
    """Without the knob a chunk holds 3,072 replicates, 256 by type: one replicate more is a second
    pass with one column."""
    _set(monkeypatch, {})
    k, fold = 3, True
    model = _model(k, fold, "dense")
    n = tile // 4 + 3
    seq = _contig(n, tile, k, seed=5)
    regions = [(0, n), (40, 41)]
    ref = _host("largest", k, fold, model, seq, regions, UNTYPED_MAX + 1)
    with _session(dev, k, fold, model) as s:
        for n_reps, by_type, passes in ((UNTYPED_MAX, False, 1), (UNTYPED_MAX + 1, False, 2), (TYPED_MAX, True, 1),
                                        (TYPED_MAX + 1, True, 2)):
            got = _null(s, seq, regions, model[2], n_reps, by_type)
            _same(got, ref, n_reps, by_type)
            assert got[1]["passes"] == passes and got[1]["reps_per_pass"] == n_reps - (passes - 1)


def _region_set(n, tile):
    """Overlapping, unordered, empty, shorter than a thread's run, across an item boundary, starting
    off a multiple of 32, repeated -- and runs of short regions that are consecutive work items."""
    run = tile // THREADS
    regs = [(tile - 9, tile + 40), (0, n), (5, 5), (run + 3, run + 3 + run - 1), (tile // 2 + 13, 2 * tile + 1), (n, n),
            (run + 3, run + 3 + run - 1), (7, 3 * run + 1), (n - 2, n), (0, 1), (tile + 17, n)]
    regs += [(100 + 37 * i, 100 + 37 * i + 1 + i % 45) for i in range(120)]  # 120 items of 1 .. 45 centres
    regs += [(tile - 20 + i, tile + 11 + i) for i in range(40)]
    return np.array(regs, np.uint64)


@pytest.mark.parametrize("env", [{}, {"KP_NULL_GRID": 1}, {"KP_NULL_GRID": 2, "KP_NULL_REPS": 7}],
                         ids=["default", "one_workgroup", "two_and_chunks"])
@pytest.mark.parametrize("k,fold", [(3, False), (5, True)])
def test_regions(dev, tile, monkeypatch, env, k, fold):
    _set(monkeypatch, env)
    model = _model(k, fold, "dense")
    n = 2 * tile + 37
    seq = _contig(n, tile, k, seed=3)
    regions = _region_set(n, tile)
    ref = _host(("regions", k, fold), k, fold, model, seq, regions, 70)
    assert ref[1]["items"] > len(regions) - 3 and np.array_equal(ref[0][3], ref[0][6]) and not ref[0][[2, 5]].any()
    with _session(dev, k, fold, model) as s:
        for n_reps, by_type in ((70, False), (70, True), (2, True)):
            _same(_null(s, seq, regions, model[2], n_reps, by_type), ref, n_reps, by_type)
        # a row does not depend on the other regions
        alone = _null(s, seq, regions[4:5], model[2], 70, True)
        assert np.array_equal(alone[0][0], ref[0][4])


@pytest.mark.parametrize("env", [{}, {"KP_NULL_GRID": 1, "KP_NULL_REPS": 64}], ids=["default", "one_workgroup_chunks"])
def test_sparse_rates_and_units_without_hits(dev, tile, monkeypatch, env):
    """Rates of 2e-5: most (item, chunk) pairs flush nothing.  One region per item, so a row is an item."""
    _set(monkeypatch, env)
    k, fold, model = 5, True, _model(5, True, "sparse")
    n = 6 * tile + 5
    seq = _contig(n, tile, k, seed=21)
    regions = [(b, min(b + tile, n)) for b in range(0, n, tile)] + [(0, n)]
    ref = _host("sparse", k, fold, model, seq, regions, 130)
    per_unit = ref[0][:-1].sum(axis=2)  # [item, replicate]
    assert (per_unit == 0).mean() > 0.5 and (per_unit > 0).sum() > 10 and ref[1]["draws"] == 130 * ref[1]["windows"]
    assert np.array_equal(per_unit.sum(axis=0), ref[0][-1].sum(axis=1))
    with _session(dev, k, fold, model) as s:
        for n_reps, by_type in ((130, False), (130, True), (65, False)):
            _same(_null(s, seq, regions, model[2], n_reps, by_type), ref, n_reps, by_type)
        none = _null(s, seq, regions, model[2], 65, True, scale=0.0)
        assert not none[0].any() and none[1]["draws"] == none[1]["hits"] == 0 and none[1]["windows"] == ref[1]["windows"]


@pytest.mark.parametrize("env", [{}, {"KP_NULL_REPS": 3}], ids=["default", "chunks"])
@pytest.mark.parametrize("k,fold", [(3, True), (5, False)])
def test_rate_one_touches_every_counter(dev, tile, monkeypatch, env, k, fold):
    """Slot 0 at rate 1.0: in every replicate a region's count is its valid windows (the host's
    stats), all of it in the types of slot 0."""
    _set(monkeypatch, env)
    model = _model(k, fold, "one")
    n = 2 * tile + 3
    seq = _contig(n, tile, k, seed=8)
    with _session(engine.HostSpec(), k, fold, model) as h:
        windows = [_null(h, seq, [r], model[2], 1, False)[1]["windows"] for r in ((0, n), (9, tile + 9))]
    assert windows[0] > n // 2
    with _session(dev, k, fold, model) as s:
        for n_reps in (1, 65, 130):
            got = _null(s, seq, [(0, n), (9, tile + 9)], model[2], n_reps, True)
            assert np.array_equal(got[0].sum(axis=2), np.repeat(np.array(windows, np.uint32)[:, None], n_reps, axis=1))
            assert not got[0][:, :, [1, 2, 4, 5, 7, 8, 10, 11]].any()
            assert got[1]["hits"] == got[1]["draws"] == n_reps * sum(windows) == n_reps * got[1]["windows"]


def test_agrees_with_the_device_simulate(dev, tile, monkeypatch):
    """The columns of a table are the device's own kp_spec_simulate sets, binned with numpy."""
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = model = _model(k, fold, "dense")
    n = 2 * tile + 91
    seq = _contig(n, tile, k, seed=14)
    regions = _region_set(n, tile)
    with _session(dev, k, fold, model) as s:
        got = _null(s, seq, regions, rates, 4, True, first=7, seed=31, contig_id=4)[0]
        for j in range(4):
            with _guard():
                pos, _, pid = s.spec_simulate(seq, [(0, n)], rates, 31, 4, 7 + j)
            kinds = np.asarray(ptype)[pid]
            for t in range(12):
                own = pos[kinds == t].astype(np.int64)
                want = np.searchsorted(own, regions[:, 1].astype(np.int64)) - np.searchsorted(own, regions[:, 0].astype(np.int64))
                assert np.array_equal(got[:, j, t], want), (j, t)
    assert got[1].sum() > 1000


def test_the_session_survives_a_null_call(dev, tile, monkeypatch):
    """A null call's buffers follow the table in the arena: spec_regions, spec_track and
    spec_simulate after it still equal the host session, and spec_regions equals itself before."""
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = model = _model(k, fold, "dense")
    n = 2 * tile + 91
    seq = _contig(n, tile, k, seed=14)
    regions = np.array([(0, n), (5, tile + 3), (tile + 3, n - 1)], np.uint64)
    out = {}
    for name, s in (("host", engine.HostSpec()), ("device", dev)):
        with _session(s, k, fold, model):
            before = s.spec_regions(seq, regions, rates)
            a = s.spec_null(seq, regions, rates, 31, 4, 0, 300, by_type=True)  # (more than its own counters: two passes)
            b = s.spec_regions(seq, regions, rates)
            c = s.spec_track(seq, 3, n - 2)
            d = s.spec_simulate(seq, [(0, n)], rates, 31, 4, 1)
            e = s.spec_null(seq, regions[::-1], rates, 31, 4, 1, 1)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before, b))
            out[name] = [a] + list(b) + [c] + list(d) + [e]
    assert len(out["host"]) == len(out["device"]) == 9
    for x, y in zip(out["host"], out["device"]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert out["device"][8][2, 0] == len(out["device"][5]) > 1000


def test_null_table_batching_on_the_device(dev, tile, monkeypatch):
    """spectrum.null_table on three contigs: a budget that forces region batches and replicate
    batches gives the table of one call, and the host's."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(6)
    names, ptype, _ = R.random_model(rng, 5, True, 6, 9)
    model = spectrum.Model(names, ptype, rng.uniform(0.001, 0.05, size=len(names)))
    contigs = [("a", R.random_seq(rng, tile + 50, lower=0.1, invalid=0.001)), ("b", R.random_seq(rng, 900)), ("c", R.random_seq(rng, 3))]
    regions = {"a": [(100, 400), (350, tile), (5, 5), (0, tile + 50)], "b": [(0, 900), (0, 450)], "c": [(0, 3)]}
    ref = spectrum.null_table(contigs, model, regions, 123, 9, first=3, by_type=True, host=True)
    stats = {}
    with _guard():
        whole = spectrum.null_table(contigs, model, regions, 123, 9, first=3, by_type=True, stats=stats)
        small = spectrum.null_table(contigs, model, regions, 123, 9, first=3, by_type=True, budget=12 * 4)
        flat = spectrum.null_table(contigs, model, regions, 123, 9, first=3, budget=2)
    assert sorted(ref) == ["a", "b", "c"] and stats["hits"] == sum(int(x.sum()) for x in ref.values()) > 500
    for name in ref:
        assert whole[name].tobytes() == ref[name].tobytes() == small[name].tobytes()
        assert np.array_equal(flat[name], ref[name].sum(axis=2))
