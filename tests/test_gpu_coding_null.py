"""Null tables per transcript by coding consequence on the GPU (kp_cnull_stage_kernel,
kp_cnull_draw_kernel) against the host session of the same per-pair functions (engine.HostSpec,
itself pinned to an independent oracle in tests/test_coding_null.py).  Bar: the table byte for byte,
and equal ``positions``, ``drawing``, ``hits`` and ``unclassed``, for every grid and every replicate
chunk.

The contigs, models and the guard are tests/test_gpu_simulate.py's: a HIP error (a fault included)
in either file is recorded and every later test of both fails before it starts anything on the
GPU."""
import numpy as np
import pytest

from kmerpapa_amd import engine, spectrum
from tests import coding_cases as K
from tests import spec_ref as R
from tests.test_gpu_simulate import _contig, _guard, _model, dev, tile  # noqa: F401 (dev, tile: fixtures)

pytestmark = pytest.mark.gpu

KNOBS = ("KP_CNULL_REPS", "KP_CNULL_GRID", "KP_CODING_GRID", "KP_CODING_GLOBAL", "KP_CODING_LDS_P", "KP_NULL_REPS",
         "KP_NULL_GRID", "KP_SIM_GRID", "KP_SPEC_GLOBAL", "KP_SPEC_LDS_P", "KP_SPEC_GRID")
CHUNK_MAX, PIECE_MAX = 256, 4095  # replicates of a chunk, records of a unit at most (include/kmerpapa_hip.h)
SCALE = 4.0  # the dense rates of 0.005 .. 0.08 become 0.02 .. 0.32


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


def _run(s, seq, txs, rates, n_reps, first=3, seed=5, contig_id=1, scale=SCALE, splice=2):
    """One call in the open session: (table, stats)."""
    with _guard():
        got = s.spec_coding_null(seq, txs, rates, seed, contig_id, first, n_reps, scale, splice)
        return got, s.spec_coding_null_stats()


_host_cache = {}


def _host(key, k, fold, model, jobs):
    """The host session's results of ``jobs`` = ``(seq, txs, n_reps, keywords)``, computed once."""
    if key not in _host_cache:
        with _session(engine.HostSpec(), k, fold, model) as s:
            _host_cache[key] = [_run(s, seq, txs, model[2], n_reps, **kw) for seq, txs, n_reps, kw in jobs]
    return _host_cache[key]


def _same(got, ref):
    assert got[0].dtype == np.uint32 and got[0].shape == ref[0].shape and got[0].tobytes() == ref[0].tobytes()
    for key in ("positions", "drawing", "hits", "unclassed"):
        assert got[1][key] == ref[1][key], key
    assert got[1]["hits"] == int(got[0].sum())


def _compare(dev, key, k, fold, model, jobs):
    ref = _host(key, k, fold, model, jobs)
    out = []
    with _session(dev, k, fold, model) as s:
        for (seq, txs, n_reps, kw), r in zip(jobs, ref):
            out.append(_run(s, seq, txs, model[2], n_reps, **kw))
            _same(out[-1], r)
    return out


@pytest.mark.parametrize("k,fold", K.KSETS)
def test_small_cases(dev, monkeypatch, k, fold):
    """The cases of tests/test_coding_null.py: the class table, every segment split and intron
    length, invalid bytes, the contig's ends and overlapping transcripts, for splice 0, 2 and 8."""
    _set(monkeypatch, {})
    model = _model(k, fold, "dense")
    jobs = [(seq, txs, 5, {"splice": splice, "seed": 100 * i + splice, "contig_id": i % 3})
            for i, (_, (seq, txs)) in enumerate(sorted(K.small_cases().items())) for splice in K.SPLICES]
    got = _compare(dev, ("small", k, fold), k, fold, model, jobs)
    total = sum(g[0].sum(axis=(0, 1)).astype(np.int64) for g in got)
    assert total.min() > 0  # every class is drawn
    if k == 1:
        assert sum(g[1]["unclassed"] for g in got) > 0


def _rseq(n, seed):
    return R.random_seq(np.random.RandomState(seed), n, lower=0.25)


def _tile_case(tile, start, k):
    """tests/test_gpu_coding.py's: a segment of tile + 35 bases whose spliced start is ``start``
    modulo 3, on both strands, with invalid bytes beside thread-run and work-item boundaries of the
    scans (here: inside a piece of records and beside its end)."""
    long = tile + 35
    last = 1 + (-(start + long + 1)) % 3
    seq = _rseq(tile + 200, seed=start)
    segs = [(20, 20 + start), (60, 60 + long), (60 + long + 30, 60 + long + 30 + last)]
    run = tile // 256
    for p in (60 + k // 2 + 5 * run + 1, 60 + tile - 1, 60 + tile + 2):
        seq[p] = ord("N")
    return seq, [(0, segs), (1, segs)]


@pytest.mark.parametrize("env", [{}, {"KP_CNULL_GRID": 1}, {"KP_CNULL_GRID": 3, "KP_CNULL_REPS": 64}],
                         ids=["default", "one_workgroup", "three_and_chunks"])
@pytest.mark.parametrize("k,fold", [(3, True), (7, True), (4, False)])
def test_a_segment_longer_than_a_tile_and_than_a_piece(dev, tile, monkeypatch, env, k, fold):
    """A transcript of more records than a unit holds: its pieces add into one row."""
    _set(monkeypatch, env)
    assert tile + 35 > PIECE_MAX
    model = _model(k, fold, "dense")
    jobs = [_tile_case(tile, start, k) + (n_reps, {}) for start in (1, 2) for n_reps in (5, 130)]
    got = _compare(dev, ("tile", k, fold), k, fold, model, jobs)
    coding = sum(e - b for b, e in jobs[0][1][0][1])
    assert coding % 3 == 0 and got[0][1]["positions"] == 2 * (coding + 8) and got[0][0].sum(axis=(1, 2)).min() > tile // 4
    if k < 7:  # (an N in a codon whose other bases have a valid window)
        assert sum(g[1]["unclassed"] for g in got) > 0


@pytest.mark.parametrize("k,fold", [(5, True), (4, False)])
def test_random_transcripts_and_lane_groups(dev, tile, monkeypatch, k, fold):
    """300 overlapping transcripts on both strands; 1, 63, 64, 65, 130 and 257 replicates: partial
    lane groups, waves that split a piece's records (up to 128) and more than one chunk."""
    _set(monkeypatch, {})
    model = _model(k, fold, "dense")
    seq, txs = K.random_case(3, 2 * tile + 200, 300)
    jobs = [(seq, txs, n_reps, {}) for n_reps in (1, 63, 64, 65, 130, 192, 257)]
    got = _compare(dev, ("random", k, fold), k, fold, model, jobs)
    for (_, _, n_reps, _), g in zip(jobs, got):
        assert g[1]["stage_ms"] > 0 and g[1]["draw_ms"] > 0
        assert g[1]["reps_per_pass"] == min(n_reps, CHUNK_MAX) and g[1]["passes"] == -(-n_reps // CHUNK_MAX)
    whole = got[-1][0]
    assert whole.sum(axis=(0, 1)).min() > 0 and (whole.sum(axis=2) == 0).any() and got[-1][1]["drawing"] < got[-1][1]["positions"]
    for (_, _, n_reps, _), g in zip(jobs, got):  # (fewer replicates are the leading columns)
        assert np.array_equal(g[0], whole[:, :n_reps])


def test_short_segments_short_introns_and_the_contig_ends(dev, monkeypatch):
    """A single-base segment, a 2-base intron, and transcripts at base 0 and at base n."""
    _set(monkeypatch, {})
    seq = _rseq(60, seed=4)
    txs = [(0, [(0, 3)]), (1, [(57, 60)]), (0, [(5, 6), (8, 10)]), (1, [(20, 24), (26, 28)]), (0, [(0, 1), (30, 31), (59, 60)]),
           (1, [(0, 60)])]
    for k, fold in ((1, True), (5, True), (4, False)):
        model = _model(k, fold, "dense")
        jobs = [(seq, txs, 70, {"splice": splice}) for splice in K.SPLICES]
        got = _compare(dev, ("short", k, fold), k, fold, model, jobs)
        assert got[1][1]["positions"] == 3 + 3 + (3 + 2) + (6 + 2) + (3 + 8) + 60 and got[1][0][[2, 3]].sum() > 0
        if k > 1:
            assert got[1][1]["drawing"] < got[1][1]["positions"]  # (windows that leave the contig draw nothing)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("reps", [1, 3, 64])
def test_replicate_chunks(dev, monkeypatch, reps, grid):
    """KP_CNULL_REPS = 1, 3, 64 with 1, 4, 65 and 130 replicates: several passes over a piece, a
    partial last chunk and partial last lanes."""
    _set(monkeypatch, {"KP_CNULL_REPS": reps, "KP_CNULL_GRID": grid})
    k, fold = 5, True
    model = _model(k, fold, "dense")
    seq, txs = K.random_case(7, 4000, 40)
    jobs = [(seq, txs, n_reps, {}) for n_reps in (1, 4, 65, 130)]
    got = _compare(dev, "chunks", k, fold, model, jobs)
    for (_, _, n_reps, _), g in zip(jobs, got):
        per = min(n_reps, reps)
        assert g[1]["reps_per_pass"] == per and g[1]["passes"] == -(-n_reps // per)


def test_the_largest_chunk(dev, monkeypatch):
    """Without the knob a chunk holds 256 replicates: one more is a second pass with one column."""
    _set(monkeypatch, {})
    k, fold = 3, True
    model = _model(k, fold, "dense")
    seq, txs = K.random_case(9, 400, 6)
    jobs = [(seq, txs, n_reps, {}) for n_reps in (CHUNK_MAX, CHUNK_MAX + 1)]
    got = _compare(dev, "largest", k, fold, model, jobs)
    assert [(g[1]["passes"], g[1]["reps_per_pass"]) for g in got] == [(1, CHUNK_MAX), (2, CHUNK_MAX)]
    assert np.array_equal(got[0][0], got[1][0][:, :CHUNK_MAX]) and got[1][0][:, CHUNK_MAX].sum() > 0


@pytest.mark.parametrize("env", [{}, {"KP_CNULL_GRID": 1, "KP_CNULL_REPS": 64}], ids=["default", "one_workgroup_chunks"])
def test_sparse_rates_and_units_without_hits(dev, tile, monkeypatch, env):
    """Rates of 2e-5: most (piece, chunk) units flush nothing."""
    _set(monkeypatch, env)
    k, fold, model = 5, True, _model(5, True, "sparse")
    seq, txs = K.random_case(3, 2 * tile + 200, 300)
    jobs = [(seq, txs, 130, {"scale": 1.0}), (seq, txs, 65, {"scale": 0.0})]
    got = _compare(dev, "sparse", k, fold, model, jobs)
    cells = got[0][0].sum(axis=2)
    assert (cells == 0).mean() > 0.9 and (cells > 0).sum() > 10
    assert not got[1][0].any() and got[1][1]["drawing"] == got[1][1]["hits"] == 0 and got[1][1]["positions"] == got[0][1]["positions"]


@pytest.mark.parametrize("env", [{}, {"KP_CNULL_REPS": 3}], ids=["default", "chunks"])
@pytest.mark.parametrize("k,fold", [(3, True), (5, False)])
def test_rate_one_counts_every_drawing_position(dev, monkeypatch, env, k, fold):
    """Slot 0 at rate 1.0 on a contig without invalid bytes: every position with a valid window
    hits in every replicate, so a row sums to the host's ``drawing`` of that transcript alone."""
    _set(monkeypatch, env)
    model = _model(k, fold, "one")
    seq, txs = K.random_case(5, 3000, 30)
    seq = _rseq(3000, seed=8)
    with _session(engine.HostSpec(), k, fold, model) as h:
        drawing = [_run(h, seq, [t], model[2], 1, scale=1.0)[1]["drawing"] for t in txs]
    assert min(drawing) > 0
    jobs = [(seq, txs, n_reps, {"scale": 1.0}) for n_reps in (1, 65, 130)]
    for (_, _, n_reps, _), g in zip(jobs, _compare(dev, ("one", k, fold), k, fold, model, jobs)):
        assert np.array_equal(g[0].sum(axis=2), np.repeat(np.array(drawing, np.uint32)[:, None], n_reps, axis=1))
        assert g[1]["unclassed"] == 0 and g[1]["hits"] == n_reps * sum(drawing) == n_reps * g[1]["drawing"]


def test_agrees_with_the_device_simulate_and_coding_sites(dev, tile, monkeypatch):
    """The columns of a table are the device's own kp_spec_simulate sets, classed by its own
    kp_spec_coding_sites and added up with numpy."""
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = model = _model(k, fold, "dense")
    seq, txs = K.random_case(3, 2 * tile + 200, 300)
    n, T = seq.shape[0], len(txs)
    unclassed = 0
    with _session(dev, k, fold, model) as s:
        got, st = _run(s, seq, txs, rates, 4, first=7, seed=31, contig_id=4)
        for j in range(4):
            with _guard():
                pos, alt, _ = s.spec_simulate(seq, [(0, n)], rates, 31, 4, 7 + j, SCALE)
                cls, _, _ = s.spec_coding_sites(seq, txs, np.repeat(pos, T), np.repeat(alt, T),
                                                np.tile(np.arange(T, dtype=np.uint32), len(pos)), 2)
            cls = cls.reshape(len(pos), T)
            want = np.stack([(cls == c).sum(axis=0) for c in range(5)], axis=1)
            assert np.array_equal(got[:, j], want), j
            unclassed += int((cls == -2).sum())
    assert st["unclassed"] == unclassed and got.sum() > 1000


def test_the_session_survives_a_coding_null_call(dev, tile, monkeypatch):
    """A call's records and table follow the lookup table in the arena: spec_regions, spec_coding,
    spec_null and spec_simulate after it still equal the host session."""
    _set(monkeypatch, {})
    k, fold = 5, True
    words, ptype, rates = model = _model(k, fold, "dense")
    seq, txs = K.random_case(5, tile + 300, 60)
    n = seq.shape[0]
    regions = np.array([(0, n), (5, tile + 3), (tile + 3, n - 1)], np.uint64)
    out = {}
    for name, s in (("host", engine.HostSpec()), ("device", dev)):
        with _session(s, k, fold, model):
            before = s.spec_regions(seq, regions, rates)
            a = s.spec_coding_null(seq, txs, rates, 31, 4, 0, 257, SCALE)  # (two passes)
            b = s.spec_regions(seq, regions, rates)
            c = s.spec_coding(seq, txs, 2, rates)
            d = s.spec_null(seq, regions, rates, 31, 4, 1, 3, SCALE, by_type=True)
            e = s.spec_simulate(seq, [(0, n)], rates, 31, 4, 1, SCALE)
            f = s.spec_coding_null(seq, txs[::-1], rates, 31, 4, 1, 1, SCALE)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(before, b))
            out[name] = [a] + list(b) + list(c) + [d] + list(e) + [f]
    assert len(out["host"]) == len(out["device"]) == 12
    for x, y in zip(out["host"], out["device"]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert out["device"][0].sum() > 1000


def test_coding_null_table_batching_on_the_device(dev, monkeypatch):
    """spectrum.coding_null_table on two contigs: a budget that forces transcript batches and
    replicate batches gives the table of one call, and the host's."""
    _set(monkeypatch, {})
    from kmerpapa_amd import seqio
    rng = np.random.RandomState(6)
    names, ptype, _ = R.random_model(rng, 5, True, 6, 9)
    model = spectrum.Model(names, ptype, rng.uniform(0.01, 0.2, size=len(names)))
    seq_a, raw_a = K.random_case(2, 1500, 12)
    seq_c, raw_c = K.random_case(3, 900, 7)
    contigs = [("a", seq_a), ("b", R.random_seq(rng, 3)), ("c", seq_c)]
    txs = [seqio.Transcript(f"{c}{i}", None, c, st, segs) for c, raw in (("c", raw_c), ("a", raw_a))
           for i, (st, segs) in enumerate(raw)]
    ref = spectrum.coding_null_table(contigs, model, txs, 123, 9, first=3, host=True)
    stats = {}
    with _guard():
        whole = spectrum.coding_null_table(contigs, model, txs, 123, 9, first=3, stats=stats)
        small = spectrum.coding_null_table(contigs, model, txs, 123, 9, first=3, budget=5 * 4 * 3)
    assert stats["hits"] == int(ref["counts"].sum()) > 500
    assert whole["counts"].tobytes() == ref["counts"].tobytes() == small["counts"].tobytes()
    assert not whole["status"].any() and np.array_equal(small["status"], ref["status"])
