"""Mutation sets drawn on the GPU (kp_sim_count_kernel, kp_sim_offsets_kernel, kp_sim_write_kernel)
against the host session of the same per-position functions (engine.HostSpec, itself pinned to an
independent oracle in tests/test_simulate.py).  Bar: ``pos``, ``alt`` and ``pid`` byte for byte, and
equal ``windows``, ``hits`` and ``items``, for every grid.

Every device call of this file goes through ``_guard``: a HIP error (a fault included) is recorded
and every later test of the file fails before it starts anything on the GPU.  The guard does not
cover a kernel that hangs: the tests run in this process, as tests/test_gpu_spectrum.py does, so a
hang ends with the time limit of the command that runs pytest."""
import ctypes

import numpy as np
import pytest

from kmerpapa_amd import engine, spectrum
from tests import spec_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("KP_SIM_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
THREADS = 256  # of a workgroup: a thread owns tile / 256 consecutive centres
word = engine.pattern_word
_hip_error = []


class _guard:
    """Nothing more is started on the GPU after a HIP error."""

    def __enter__(self):
        assert not _hip_error, f"an earlier GPU step failed, nothing more is started: {_hip_error[0]}"

    def __exit__(self, kind, exc, tb):
        if isinstance(exc, engine.KPError) and exc.code == -3:
            _hip_error.append(str(exc))
        return False


@pytest.fixture(scope="module")
def dev():
    with _guard():
        engine.load()
        assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
        return engine.get_device(engine.visible_devices()[0])


@pytest.fixture(scope="module")
def tile(dev):
    with _guard():
        dev.spec_begin(1, [word("A")], [0], False)
        dev.spec_end()
        t = dev.spec_stats()["tile"]
    assert t >= THREADS and t % THREADS == 0
    return t


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


_model_cache = {}


def _model(k, fold, kind):
    """(words, ptype, rates) of a random model of every type: ``dense`` rates 0.005 .. 0.08 (about
    four hits per thread run of 32 centres, and a run in fifty without one), ``sparse`` 2e-5 (most
    work items without a hit), ``one``: rate 1.0 for slot 0 and 0.0 for the others."""
    key = (k, fold, kind)
    if key not in _model_cache:
        rng = np.random.RandomState(7 * k + fold)
        names, ptype, _ = R.random_model(rng, k, fold, 6 if fold else 12, 6)
        if kind == "dense":
            rates = rng.uniform(0.005, 0.08, size=len(names))
        elif kind == "sparse":
            rates = np.full(len(names), 2e-5)
        else:
            rates = np.array([1.0 if t % 3 == 0 else 0.0 for t in ptype])
        _model_cache[key] = ([word(x) for x in names], ptype, rates)
    return _model_cache[key]


def _contig(n, tile, k, seed):
    """``n`` mixed-case bases with an invalid byte k - 1 bases before and after every work-item
    boundary of a whole-contig call and around a few thread-run boundaries."""
    rng = np.random.RandomState(seed)
    seq = R.random_seq(rng, n, lower=0.25)
    run = tile // THREADS
    first = k // 2
    marks = []
    for i in (1, 2, 3):
        b = first + i * tile
        marks += [b - (k - 1), b + (k - 1), b - k // 2 - (k - 1), b - k // 2 + 2 * (k - 1)]
    for d in range(1, k):
        b = first + (7 + 9 * d) * run
        marks += [b - d, b + 3 * run + d - 1]
    for m in marks:
        if 0 <= m < n:
            seq[m] = ord("N")
    return seq


def _regions(n, tile):
    """Ascending and disjoint: regions that end inside a thread's run, adjacent and empty ones, and
    one that begins at every item boundary of the whole contig."""
    run = tile // THREADS
    cuts = [0, 0, 3, run + 5, run + 5, 2 * run - 1, 2 * run - 1, tile // 2 + 13]
    regs = [(min(b, n), min(e, n)) for b, e in zip(cuts[:-1], cuts[1:])]
    for b in range(tile, n, tile):
        regs += [(b - 7, b), (b, min(n, b + tile // 3 + 1)), (min(n, b + tile // 3 + 1), min(n, b + tile // 3 + 1))]
    regs.append((max(n - 3, regs[-1][1]), n))
    return np.array(regs, np.uint64)


def _sim(s, k, fold, model, seq, regions, seed=5, contig_id=1, replicate=2, scale=1.0, cap=None):
    """One session with one simulate call: (pos, alt, pid, sim stats)."""
    words, ptype, rates = model
    with _guard():
        s.spec_begin(k, words, ptype, fold)
        try:
            got = s.spec_simulate(seq, regions, rates, seed, contig_id, replicate, scale, cap)
            st = s.spec_sim_stats()
        finally:
            s.spec_end()
    return got + (st,)


_host_cache = {}


def _host(key, *args, **kw):
    """The host session of a case, computed once and shared by the grids."""
    if key not in _host_cache:
        _host_cache[key] = _sim(engine.HostSpec(), *args, **kw)
    return _host_cache[key]


def _same(got, ref):
    for g, r in zip(got[:3], ref[:3]):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    for x in ("windows", "hits", "items"):
        assert got[3][x] == ref[3][x], x


def _per_item(ref, n, tile, k):
    """Hits per work item of a whole-contig call."""
    items = -(-(n - k + 1) // tile)
    return np.bincount((ref[0].astype(np.int64) - k // 2) // tile, minlength=items)


@pytest.mark.parametrize("env", [{}, {"KP_SIM_GRID": 1}, {"KP_SIM_GRID": 3}], ids=["default", "one_workgroup", "three"])
@pytest.mark.parametrize("k,fold", [(3, True), (3, False), (5, True), (5, False)])
def test_contig_lengths_around_the_tile(dev, tile, monkeypatch, env, k, fold):
    """Dense rates -- most threads have several hits, some none -- on contigs of tile - 1, tile,
    tile + 1 and 3 tile + 37 bases, one shorter than k and an empty one."""
    _set(monkeypatch, env)
    model = _model(k, fold, "dense")
    for n in (tile - 1, tile, tile + 1, 3 * tile + 37, k - 1, 0):
        seq = _contig(n, tile, k, seed=n % 97)
        got = _sim(dev, k, fold, model, seq, [(0, n)])
        ref = _host(("len", k, fold, n), k, fold, model, seq, [(0, n)])
        _same(got, ref)
        if n >= k:
            assert ref[3]["items"] == -(-(n - k + 1) // tile) and 0 < ref[3]["hits"] < ref[3]["windows"] < n - k + 1
            assert got[3]["count_ms"] > 0 and got[3]["write_ms"] > 0
            run = tile // THREADS
            runs = (n - k + 1) // run  # whole thread runs of the contig
            per_thread = np.bincount((ref[0].astype(np.int64) - k // 2) // run, minlength=runs)[:runs]
            assert (per_thread >= 2).sum() > runs // 2 and (per_thread == 0).any()
        else:
            assert ref[3]["items"] == ref[3]["hits"] == ref[3]["windows"] == 0 and got[3]["count_ms"] == 0


@pytest.mark.parametrize("env", [{}, {"KP_SIM_GRID": 1}], ids=["default", "one_workgroup"])
@pytest.mark.parametrize("k,fold", [(3, False), (5, True)])
def test_regions(dev, tile, monkeypatch, env, k, fold):
    """Regions that end inside a thread's run, adjacent and empty regions and one per item boundary:
    the draws are those of the whole contig."""
    _set(monkeypatch, env)
    model = _model(k, fold, "dense")
    n = 3 * tile + 37
    seq = _contig(n, tile, k, seed=3)
    regions = _regions(n, tile)
    got = _sim(dev, k, fold, model, seq, regions)
    ref = _host(("regions", k, fold), k, fold, model, seq, regions)
    _same(got, ref)
    whole = _host(("regions_whole", k, fold), k, fold, model, seq, [(0, n)])
    inside = np.zeros(n, bool)
    for b, e in regions.tolist():
        inside[b:e] = True
    keep = inside[whole[0].astype(np.intp)]
    assert 100 < keep.sum() < len(keep) and ref[3]["items"] > whole[3]["items"]
    for w, g in zip(whole[:3], got[:3]):
        assert w[keep].tobytes() == g.tobytes()


@pytest.mark.parametrize("env", [{}, {"KP_SIM_GRID": 1}], ids=["default", "one_workgroup"])
def test_sparse_rates_and_items_without_hits(dev, tile, monkeypatch, env):
    _set(monkeypatch, env)
    k, fold, model = 5, True, _model(5, True, "sparse")
    n = 12 * tile + 5
    seq = _contig(n, tile, k, seed=21)
    got = _sim(dev, k, fold, model, seq, [(0, n)])
    ref = _host("sparse", k, fold, model, seq, [(0, n)])
    _same(got, ref)
    per_item = _per_item(ref, n, tile, k)
    assert (per_item == 0).any() and (per_item > 0).sum() >= 2
    # the same model at fifty times the rates, and nothing at scale 0
    _same(_sim(dev, k, fold, model, seq, [(0, n)], scale=50.0), _host("sparse50", k, fold, model, seq, [(0, n)], scale=50.0))
    none = _sim(dev, k, fold, model, seq, [(0, n)], scale=0.0)
    assert none[3]["hits"] == 0 and none[3]["write_ms"] == 0 and none[3]["windows"] == ref[3]["windows"]


@pytest.mark.parametrize("k,fold", [(3, True), (5, False)])
def test_rate_one_fills_every_window(dev, tile, monkeypatch, k, fold):
    """Slot 0 at rate 1.0: an item's hits equal its valid windows, the most the scan inside an item
    and a thread's staging buffer see."""
    _set(monkeypatch, {})
    model = _model(k, fold, "one")
    n = 2 * tile + 3
    seq = _contig(n, tile, k, seed=8)
    got = _sim(dev, k, fold, model, seq, [(0, n)])
    ref = _host(("one", k, fold), k, fold, model, seq, [(0, n)])
    _same(got, ref)
    assert ref[3]["hits"] == ref[3]["windows"] > n // 2
    clean = R.random_seq(np.random.RandomState(1), tile + k - 1)  # one item, every thread's run full
    full = _sim(dev, k, fold, model, clean, [(0, tile + k - 1)])
    _same(full, _host(("one_clean", k, fold), k, fold, model, clean, [(0, tile + k - 1)]))
    assert full[3]["hits"] == tile and full[3]["items"] == 1


def _raw(s, seq, regions, rates, seed, cap, fill=0x5A):
    """kp_spec_simulate itself: ``(rc, n_hits, pos, alt, pid)`` with the outputs pre-filled."""
    reg = np.asarray(regions, np.uint64).reshape(-1, 2)
    rb, re = np.ascontiguousarray(reg[:, 0]), np.ascontiguousarray(reg[:, 1])
    rates = np.ascontiguousarray(rates, np.float64)
    pos, alt, pid = np.full(cap + 1, fill, np.uint64), np.full(cap + 1, fill, np.uint8), np.full(cap + 1, fill, np.int32)
    n_hits = ctypes.c_uint64(0)
    p = engine._ptr
    rc = engine.load().kp_spec_simulate(s._h, p(seq), ctypes.c_uint64(seq.shape[0]), ctypes.c_uint32(0), p(rb), p(re),
                                        ctypes.c_uint64(reg.shape[0]), p(rates), ctypes.c_double(1.0), ctypes.c_uint64(seed),
                                        ctypes.c_uint32(0), ctypes.c_uint64(cap), p(pos), p(alt), p(pid), ctypes.byref(n_hits))
    return rc, n_hits.value, pos, alt, pid


def test_cap_too_small_then_exact(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = _model(k, fold, "dense")
    n = tile + 700
    seq = _contig(n, tile, k, seed=2)
    want = _host("cap", k, fold, (words, ptype, rates), seq, [(0, n)], seed=9, contig_id=0, replicate=0)
    h = want[3]["hits"]
    assert h > 300
    with _guard():
        dev.spec_begin(k, words, ptype, fold)
        try:
            rc, n_hits, pos, alt, pid = _raw(dev, seq, [(0, n)], rates, 9, h - 1)
            st = dev.spec_sim_stats()
            assert rc == 0 and n_hits == h and st["hits"] == h and st["write_ms"] == 0 and st["count_ms"] > 0
            assert np.all(pos == 0x5A) and np.all(alt == 0x5A) and np.all(pid == 0x5A)
            rc, n_hits, pos, alt, pid = _raw(dev, seq, [(0, n)], rates, 9, h)
            assert rc == 0 and n_hits == h and dev.spec_sim_stats()["write_ms"] > 0
            assert pos[:h].tobytes() == want[0].tobytes() and alt[:h].tobytes() == want[1].tobytes()
            assert pid[:h].tobytes() == want[2].tobytes() and pos[h] == 0x5A and alt[h] == 0x5A and pid[h] == 0x5A
            # the wrapper's own first guess, and guesses that are too small
            for cap in (None, 0, h - 1, h, 4 * n):
                got = dev.spec_simulate(seq, [(0, n)], rates, 9, cap=cap)
                assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want[:3])), cap
        finally:
            dev.spec_end()


def test_the_session_survives_a_simulate_call(dev, tile, monkeypatch):
    """A simulate call's buffers follow the table in the arena: spec_regions and spec_track after it,
    and a second simulate call, still equal the host session."""
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = _model(k, fold, "dense")
    n = 2 * tile + 91
    seq = _contig(n, tile, k, seed=14)
    regions = np.array([(0, n), (5, tile + 3), (tile + 3, n - 1)], np.uint64)
    out = {}
    for name, s in (("host", engine.HostSpec()), ("device", dev)):
        with _guard():
            s.spec_begin(k, words, ptype, fold)
            try:
                a = s.spec_simulate(seq, regions[1:], rates, 31, 4, 0, cap=3 * n)  # (room for every centre)
                b = s.spec_regions(seq, regions, rates)
                c = s.spec_track(seq, 3, n - 2)
                d = s.spec_simulate(seq, [(0, n)], rates, 31, 4, 1)
                e = s.spec_sites(seq, d[0], d[1])
                out[name] = list(a) + list(b) + [c] + list(d) + [e]
            finally:
                s.spec_end()
    assert len(out["host"]) == len(out["device"]) == 11
    for x, y in zip(out["host"], out["device"]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert np.array_equal(out["device"][10], out["device"][9]) and len(out["device"][0]) > 1000


def test_simulate_api_on_the_device(dev, tile, monkeypatch):
    """spectrum.simulate on two contigs with regions: the device yields what the host yields."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(6)
    names, ptype, _ = R.random_model(rng, 5, True, 6, 9)
    model = spectrum.Model(names, ptype, rng.uniform(0.001, 0.05, size=len(names)))
    contigs = [("a", R.random_seq(rng, tile + 50, lower=0.1, invalid=0.001)), ("b", R.random_seq(rng, 900)), ("c", R.random_seq(rng, 3))]
    regions = {"a": [(100, 400), (350, tile), (5, 5)], "c": [(0, 3)]}
    for reg in (None, regions):
        with _guard():
            got = list(spectrum.simulate(contigs, model, 123, regions=reg, replicate=3))
        ref = list(spectrum.simulate(contigs, model, 123, regions=reg, replicate=3, host=True))
        assert [x[0] for x in got] == ["a", "b", "c"] and sum(len(x[1]) for x in ref) > 100
        for g, r in zip(got, ref):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(g[1:], r[1:]))
