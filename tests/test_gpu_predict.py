"""A fitted partition taken back to the genome on the GPU (kp_pred_lut_kernel, kp_pred_scan_kernel,
kp_pred_track_kernel, kp_pred_sites_kernel, kp_pred_sums_kernel) against the host session of the
same per-base and per-code functions (engine.HostPred, itself pinned to an independent oracle in
tests/test_predict.py).  Bar: every count equal and ``expected`` bit-identical, on both counter
paths and every knob setting; the path a case ran is asserted from the session's stats, so a
silent fallback cannot pass for the path under test."""
import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, predict, score_utils
from kmerpapa_amd.papa import PatternPartition
from tests import pred_ref as R

pytestmark = pytest.mark.gpu

LDS, GLOBAL = engine.PRED_PATH_LDS, engine.PRED_PATH_GLOBAL
KNOBS = ("KP_PRED_GLOBAL", "KP_PRED_LDS_P", "KP_PRED_GRID")
THREADS = 256  # of a scan workgroup: a thread owns tile / 256 consecutive centres
ENVS = [({}, LDS), ({"KP_PRED_GLOBAL": 1}, GLOBAL)]
ENV_IDS = ["lds", "global"]


@pytest.fixture(scope="module")
def dev():
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine.get_device(engine.visible_devices()[0])


@pytest.fixture(scope="module")
def tile(dev):
    dev.pred_begin(1, [engine.pattern_word("N")], engine.pattern_word("N"), False)
    dev.pred_end()
    t = dev.pred_stats()["tile"]
    assert t >= THREADS and t % THREADS == 0
    return t


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


_part_cache = {}


def _partition(gp, P, seed=0):
    """(pattern words, super word, rates, names) of a random partition of ``gp`` into ``P``."""
    key = (gp, P, seed)
    if key not in _part_cache:
        rng = np.random.RandomState(1000 * seed + P + len(gp))
        names = R.random_partition(rng, gp, P)
        _part_cache[key] = ([engine.pattern_word(x) for x in names], engine.pattern_word(gp), R.wide_rates(rng, P), names)
    return _part_cache[key]


def _general(k, fold):
    return "N" * (k // 2) + "M" + "N" * (k // 2) if fold else "N" * k


def _session(s, k, fold, part, seq, regions=None, track=None, sites=None, want_hist=True):
    """One session of one contig: (hist, other, expected, track pid, site pid, stats)."""
    words, sw, rates, _ = part
    s.pred_begin(k, words, sw, fold)
    try:
        h = o = e = t = p = None
        if regions is not None:
            h, o, e = s.pred_regions(seq, regions, rates, want_hist)
        if track is not None:
            t = s.pred_track(seq, *track)
        if sites is not None:
            p = s.pred_sites(seq, sites)
        st = s.pred_stats()
    finally:
        s.pred_end()
    return h, o, e, t, p, st


_host_cache = {}


def _host(key, *args, **kw):
    """The host session of a case, computed once and shared by the knob settings."""
    if key not in _host_cache:
        _host_cache[key] = _session(engine.HostPred(), *args, **kw)
    return _host_cache[key]


def _same(got, ref):
    for g, r in zip(got[:5], ref[:5]):
        assert (g is None) == (r is None)
        if g is not None:
            assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    for x in ("assigned", "unmatched", "invalid", "items", "tile", "lut_bytes"):
        assert got[5][x] == ref[5][x], x


def _boundary_contig(tile, k, seed=3):
    """3 * tile + 17 mixed-case bases with an invalid byte k - 1 bases before and after every
    work-item boundary (= workgroup boundary: the items go round the grid) and around one
    thread-run boundary per offset 1 .. k - 1, on both sides."""
    rng = np.random.RandomState(seed + k)
    n = 3 * tile + 17
    seq = R.random_seq(rng, n, lower=0.25)
    run = tile // THREADS
    first = k // 2  # the first centre
    marks = []
    for i in (1, 2, 3):  # item boundaries, as bytes of the window's first and last base
        b = first + i * tile
        marks += [b - (k - 1), b + (k - 1), b - k // 2 - (k - 1), b - k // 2 + 2 * (k - 1)]
    for d in range(1, k):  # thread-run boundaries far from each other and from the item boundaries
        b = first + (7 + 9 * d) * run
        marks += [b - d, b + 3 * run + d - 1, b + 6 * run - k // 2 - d, b + 6 * run - k // 2 + k - 1 + d]
    for m in marks:
        if 0 <= m < n:
            seq[m] = ord("N")
    return seq


# (k = 3 has 64 k-mers: no partition of 1,025 patterns; its 37 are cut from NNN, so the patterns
# with G or T in the centre match nothing under folding)
BOUNDARY = [(3, True, "NNN", 1), (3, True, "NNN", 37), (7, True, None, 1), (7, True, None, 37), (7, True, None, 1025),
            (9, True, None, 1), (9, True, None, 37), (9, True, None, 1025), (11, True, None, 1), (11, True, None, 37),
            (11, True, None, 1025), (8, False, None, 1), (8, False, None, 37), (8, False, None, 1025)]


@pytest.mark.parametrize("env,path", ENVS, ids=ENV_IDS)
@pytest.mark.parametrize("k,fold,gp,P", BOUNDARY, ids=[f"k{c[0]}_P{c[3]}" for c in BOUNDARY])
def test_boundary_contig(dev, tile, monkeypatch, k, fold, gp, P, env, path):
    _set(monkeypatch, env)
    part = _partition(gp or _general(k, fold), P)
    seq = _boundary_contig(tile, k)
    n = seq.shape[0]
    regions = np.array([(0, n), (tile - 5, 2 * tile + 40), (0, 0), (n - 1, n), (0, 1), (17, n - 3)])
    got = _session(dev, k, fold, part, seq, regions)
    _same(got, _host(("b", k, fold, gp, P), k, fold, part, seq, regions))
    assert got[5]["path"] == path and got[5]["scan_ms"] > 0 and got[5]["lut_ms"] > 0
    assert got[5]["lut_bytes"] == 4 * 4 ** k
    assert got[5]["items"] == 4 + 2 + 3  # (n - 1, n) and (0, 1) hold no centre whose window fits: no item
    assert 0 < int(got[1][0, 1]) < 40 * k * k and int(got[0][0].sum() + got[1][0].sum()) == n
    if gp is None and fold:  # a super pattern with M in the centre and folding: every valid window has a pattern
        assert int(got[1][0, 0]) == 0


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_PRED_GRID": 1}, LDS), ({"KP_PRED_GLOBAL": 1}, GLOBAL),
                                      ({"KP_PRED_GRID": 1, "KP_PRED_GLOBAL": 1}, GLOBAL)],
                         ids=["lds", "lds_one_workgroup", "global", "global_one_workgroup"])
def test_many_short_overlapping_regions(dev, tile, monkeypatch, env, path):
    """About 3,000 regions of 1..300 bases in random order.  With one workgroup walking every
    item, counters left over from the item before, or flushed to the wrong row, show."""
    _set(monkeypatch, env)
    rng = np.random.RandomState(51)
    n = 2 * tile
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.002)
    begin = rng.randint(2, n - 302, size=3000)  # (every region keeps a centre whose window fits: one item each)
    regions = np.stack([begin, begin + rng.randint(1, 301, size=3000)], axis=1)
    k, part = 5, _partition("NNCNN", 37)  # no folding under NNCNN: most windows match no pattern
    got = _session(dev, k, False, part, seq, regions)
    _same(got, _host("short", k, False, part, seq, regions))
    assert got[5]["path"] == path and got[5]["items"] == 3000 and got[5]["unmatched"] > got[5]["assigned"] > 0


def test_regions_at_item_boundaries(dev, tile, monkeypatch):
    """Regions of tile - 1, tile and tile + 1 centres, one ending where the next begins."""
    k, t = 7, tile
    n = 6 * t + 50
    seq = R.random_seq(np.random.RandomState(17), n, lower=0.1, invalid=0.001)
    regions = np.array([(5, 5 + t - 1), (5 + t - 1, 5 + 2 * t - 1), (5 + 2 * t - 1, 5 + 3 * t), (3 * t + 40, 3 * t + 41),
                        (4 * t, 4 * t), (4 * t + 3, 5 * t + 2), (n - 6, n), (0, 5), (0, n)])
    part = _partition(_general(k, True), 37)
    ref = _host("items", k, True, part, seq, regions)
    for env, path in ENVS + [({"KP_PRED_GRID": 1}, LDS), ({"KP_PRED_GRID": 3, "KP_PRED_GLOBAL": 1}, GLOBAL)]:
        _set(monkeypatch, env)
        got = _session(dev, k, True, part, seq, regions)
        _same(got, ref)
        # (n - 6, n) keeps its 3 centres with a window, (0, 5) its 2; the whole contig is 7 items
        assert got[5]["path"] == path and got[5]["items"] == 1 + 1 + 2 + 1 + 0 + 1 + 1 + 1 + 7


def test_path_threshold(dev, tile, monkeypatch):
    seq = _boundary_contig(tile, 8)
    regions = np.array([(0, seq.shape[0]), (100, tile + 100)])
    for P, env, path in ((64, {"KP_PRED_LDS_P": 64}, LDS), (65, {"KP_PRED_LDS_P": 64}, GLOBAL), (16384, {}, LDS),
                         (16385, {}, GLOBAL), (1, {"KP_PRED_LDS_P": 0}, GLOBAL)):
        _set(monkeypatch, env)
        part = _partition("N" * 8, P)
        got = _session(dev, 8, False, part, seq, regions, want_hist=P < 1000)
        _same(got, _host(("thr", P), 8, False, part, seq, regions, want_hist=P < 1000))
        assert got[5]["path"] == path, P
    _set(monkeypatch, {"KP_PRED_LDS_P": 16385})  # the counters would not fit beside a second workgroup's
    with pytest.raises(engine.KPError) as e:
        _session(dev, 8, False, part, seq, regions)
    assert e.value.code == -1


@pytest.mark.parametrize("env,path", ENVS + [({"KP_PRED_GRID": 1}, LDS)], ids=ENV_IDS + ["lds_one_workgroup"])
def test_low_complexity(dev, monkeypatch, env, path):
    """A 200,000-base homopolymer, then a dinucleotide repeat: every lane adds to one LDS counter,
    and one row receives the flushes of many items."""
    _set(monkeypatch, env)
    seq = np.concatenate([np.full(200_000, ord("a"), np.uint8), np.frombuffer(b"CA" * 30_000, np.uint8),
                          np.frombuffer(b"N", np.uint8), np.full(70_001, ord("G"), np.uint8)])
    n = seq.shape[0]
    regions = np.array([(0, n), (1000, 250_000)])
    k, part = 7, _partition(_general(7, True), 37)
    got = _session(dev, k, True, part, seq, regions)
    _same(got, _host("low", k, True, part, seq, regions))
    assert got[5]["path"] == path and int(got[0][0].max()) >= 200_000 - k > 1 << 16


def test_short_items_on_a_context_of_their_own(monkeypatch):
    """Short and unaligned work items, at a contig's end too, on a fresh context, whose input
    allocation is never larger than these small contigs need (smallest first: it only grows).  The
    threads of a short item that own no centre must load nothing: the bytes their position
    stands for lie kilobytes past that allocation."""
    own = engine.Device(engine.visible_devices()[0])
    try:
        rng = np.random.RandomState(41)
        for n in (64, 1000):
            seq = R.random_seq(rng, n, lower=0.2, invalid=0.004)
            cases = [(7, [(n - 10, n)]), (7, [(3, 4), (n // 2 + 1, n // 2 + 17), (n - 15, n)]), (9, [(n - 7, n)]),
                     (3, [(0, n)]), (11, [(0, n)]), (5, [(n - 3, n - 2)])]
            for k, regions in cases:
                part = _partition(_general(k, True), 1 if k == 3 else 37)
                args = (k, True, part, seq, np.array(regions))
                kw = dict(track=(max(n - 40, 0), n), sites=[0, n - 1, n // 2])
                ref = _session(engine.HostPred(), *args, **kw)
                for env, path in ENVS:
                    _set(monkeypatch, env)
                    got = _session(own, *args, **kw)
                    _same(got, ref)
                    assert got[5]["path"] == path
    finally:
        own.close()


def test_table_is_rebuilt_after_the_arena_grew(monkeypatch):
    """On a context of its own the arena starts at the table plus its staged patterns (under 1 KiB
    for k = 3).  The sites call fits in it, the 592 KB of counters of 2,000 regions do not: the arena
    grows, which frees the table, and it is built again before the scan, the track and the second
    sites call read it."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(83)
    n = 333
    seq = R.random_seq(rng, n, lower=0.2)
    seq[150] = ord("N")
    begin = rng.randint(0, n - 5, size=2000)
    regions = np.stack([begin, begin + rng.randint(1, 6, size=2000)], axis=1)
    words, sw, rates, _ = _partition("NNN", 37)
    sites = [0, 151, n - 1]

    def calls(s):
        s.pred_begin(3, words, sw, True)
        try:
            first = s.pred_sites(seq, sites)
            hist, other, exp = s.pred_regions(seq, regions, rates, True)
            track = s.pred_track(seq, 0, n)
            return first, hist, other, exp, track, s.pred_sites(seq, sites)
        finally:
            s.pred_end()

    ref = calls(engine.HostPred())
    own = engine.Device(engine.visible_devices()[0])
    try:
        got = calls(own)
    finally:
        own.close()
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape and g.tobytes() == r.tobytes()
    assert ref[1].nbytes > 1 << 16 and int(ref[1].sum()) > 0 and (ref[4] == -2).sum() >= 5 and (ref[4] >= 0).any()


def test_track(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    rng = np.random.RandomState(61)
    n = 3 * tile + 3
    seq = R.random_seq(rng, n, lower=0.2, invalid=0.002)
    for k, fold, gp, P in ((9, True, None, 1025), (5, False, "NNCNN", 37), (8, False, None, 37)):
        part = _partition(gp or _general(k, fold), P)
        for b, e in ((0, n), (0, tile + 3), (13, 2 * tile + 7), (tile - 1, tile + 2), (5, 6), (n - 1, n), (0, 1), (7, 7),
                     (tile + 6, 2 * tile + 6), (n - 21, n)):
            got = _session(dev, k, fold, part, seq, track=(b, e))
            ref = _host(("track", k, b, e), k, fold, part, seq, track=(b, e))
            _same(got, ref)
            assert got[3].shape == (e - b,) and got[5]["items"] == -(-(e - b) // tile)
        whole = _host(("track", k, 0, n), k, fold, part, seq, track=(0, n))[3]
        assert (whole[:k // 2] == -2).all() and (whole[n - (k - 1 - k // 2):] == -2).all() and (whole >= 0).sum() > n // 8
        _set(monkeypatch, {"KP_PRED_GRID": 1})
        _same(_session(dev, k, fold, part, seq, track=(13, 2 * tile + 7)),
              _host(("track", k, 13, 2 * tile + 7), k, fold, part, seq, track=(13, 2 * tile + 7)))
        _set(monkeypatch, {})


def test_sites(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    rng = np.random.RandomState(29)
    n = 2 * tile + 9
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.003)
    sites = [0, 1, n - 1, n - 2] + [b + d for b in (tile, 2 * tile, 255, 256, 257) for d in (-1, 0, 0, 1, 4)]
    sites += rng.randint(0, n, size=1000).tolist() + [tile] * 70
    for k, fold, P in ((3, True, 1), (7, True, 37), (11, True, 1025), (4, False, 37)):
        part = _partition(_general(k, fold), P)
        got = _session(dev, k, fold, part, seq, sites=sites)
        _same(got, _session(engine.HostPred(), k, fold, part, seq, sites=sites))
        assert got[4][0] == -2 and got[4][2] == -2 and (got[4] >= 0).sum() > 900 and got[5]["path"] == 0
        track = _host(("sites", k), k, fold, part, seq, track=(0, n))[3]
        assert np.array_equal(got[4], track[np.array(sites)])


def test_second_session_and_errors(dev, tile, monkeypatch):
    """Another k and another partition on the same context: a stale lookup table or stale arena
    contents would show.  Calls out of order are KP_E_STATE, and kp_seq_begin / kp_greedy /
    kp_apply refuse to take the arena while a session holds its table in it."""
    _set(monkeypatch, {})
    seq = _boundary_contig(tile, 9)
    n = seq.shape[0]
    regions = np.array([(0, n), (5, 700)])
    first = None
    for k, fold, gp, P in ((9, True, None, 37), (5, False, "NNCNN", 37), (11, True, None, 1025), (5, True, None, 2),
                           (9, True, None, 37)):
        part = _partition(gp or _general(k, fold), P)
        got = _session(dev, k, fold, part, seq, regions, track=(3, 5000), sites=[5, 6])
        _same(got, _host(("second", k, fold, P), k, fold, part, seq, regions, track=(3, 5000), sites=[5, 6]))
        first = first or got
    assert got[0].tobytes() == first[0].tobytes() and got[2].tobytes() == first[2].tobytes()
    for call in (lambda: dev.pred_regions(seq, regions), lambda: dev.pred_track(seq), lambda: dev.pred_sites(seq, [1]),
                 lambda: dev.pred_end()):
        with pytest.raises(engine.KPError) as e:
            call()
        assert e.value.code == -4
    nn, word = engine.pattern_word("NN"), engine.pattern_word
    for k, fold, pats in ((16, False, [word("N" * 16)]), (0, False, [0]), (2, True, [nn]), (2, False, [nn, word("AN")]),
                          (2, False, []), (2, False, [word("N")])):
        with pytest.raises(engine.KPError) as e:
            dev.pred_begin(k, pats, nn if k == 2 else (1 << 64) - 1, fold)
        assert e.value.code == -1
    dev.seq_begin(3, True)
    try:
        with pytest.raises(engine.KPError) as e:
            dev.pred_begin(2, [nn], nn, False)
        assert e.value.code == -4
    finally:
        dev.seq_end(False, False)
    dev.pred_begin(2, [nn], nn, False)
    try:
        for call in (lambda: dev.pred_begin(2, [nn], nn, False), lambda: dev.seq_begin(3, True),
                     lambda: dev.greedy("NN", np.ones(16, np.uint64), np.ones(16, np.uint64), [(-1, -1, 1.0, 1.0, 1.0)]),
                     lambda: dev.apply(2, [nn], nn, [0], [1], [1])):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -4
        for bad in ([(10, 5)], [(0, n + 1)]):
            with pytest.raises(engine.KPError) as e:
                dev.pred_regions(seq, np.array(bad))
            assert e.value.code == -1
        for call in (lambda: dev.pred_sites(seq, [n]), lambda: dev.pred_track(seq, 5, 4), lambda: dev.pred_track(seq, 0, n + 1)):
            with pytest.raises(engine.KPError) as e:
                call()
            assert e.value.code == -1
        hist, other, _ = dev.pred_regions(seq[:100], [(0, 100)])
    finally:
        dev.pred_end()
    assert int(hist[0, 0]) == 99 and other.tolist() == [[0, 1]]


@pytest.mark.parametrize("env,path", ENVS, ids=ENV_IDS)
def test_expected_is_bit_identical(dev, tile, monkeypatch, env, path):
    """1,025 rates over twelve orders of magnitude: any other order of the adds rounds differently."""
    _set(monkeypatch, env)
    rng = np.random.RandomState(71)
    seq = R.random_seq(rng, tile + 500, lower=0.1, invalid=0.001)
    begin = rng.randint(0, tile, size=200)
    regions = np.stack([begin, begin + rng.randint(0, 500, size=200)], axis=1)
    part = _partition(_general(9, True), 1025)
    got = _session(dev, 9, True, part, seq, regions)
    ref = _host("expected", 9, True, part, seq, regions)
    assert got[2].tobytes() == ref[2].tobytes() and got[5]["path"] == path
    shuffled = np.array([float(np.sum((ref[0][r] * part[2])[::-1])) for r in range(200)])
    assert (shuffled != ref[2]).any()  # (the case can tell orders apart)


def test_command_line_on_the_gpu(dev, monkeypatch, tmp_path):
    """kmerpapa-predict's three subcommands on their default (GPU) path write what the host path writes."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(37)
    contigs = [("chr1", R.random_seq(rng, 20_011, lower=0.3, invalid=0.002)), ("chr2", R.random_seq(rng, 9_000))]
    fa, tb = str(tmp_path / "g.fa"), str(tmp_path / "g.2bit")
    R.write_fasta(fa, [(n, np.where(np.isin(s & 0xDF, list(b"ACGT")), s, ord("N")).astype(np.uint8)) for n, s in contigs])
    R.write_2bit(tb, contigs, ">")
    _, _, rates, names = _partition("NNMNN", 37)
    with open(tmp_path / "p.txt", "w") as f:
        f.write("pattern p_neg p_pos p_rate\n" + "".join(f"{x} 10 1 {float(r)!r}\n" for x, r in zip(names, rates)))
    with open(tmp_path / "r.bed", "w") as f:
        f.write("chr1 100 9000 geneA\nchr2 0 10 geneB\nchr1 8000 20011 geneC\nchrX 1 2 geneD\n")
    with open(tmp_path / "m.txt", "w") as f:
        for p in rng.choice(9_000, size=500, replace=False).tolist():
            ref = chr(contigs[1][1][p]).upper()
            f.write(f"chr2 {p + 1} {ref} {'ACGT'[('ACGT'.index(ref) + 1) % 4]}\n")
    out = {}
    part = ["--partition", str(tmp_path / "p.txt")]
    for host in (False, True):
        for name, argv in (("regions", ["regions", tb, "--bed", str(tmp_path / "r.bed")]), ("track", ["track", fa]),
                           ("track_bed", ["track", tb, "--bed", str(tmp_path / "r.bed")]),
                           ("sites", ["sites", fa, str(tmp_path / "m.txt")])):
            path = str(tmp_path / f"{name}{int(host)}.txt")
            assert predict.main(argv + part + ["-o", path, "--verbosity", "0"], host=host) == 0
            out[name, host] = open(path).read()
    for name in ("regions", "track", "track_bed", "sites"):
        assert out[name, False] == out[name, True] and len(out[name, False]) > 100
    assert len(out["sites", False].splitlines()) == 500 and len(out["regions", False].splitlines()) == 4


def test_count_greedy_predict(dev, monkeypatch):
    """End to end on the GPU: count a genome and its sites, fit the greedy partition, and take it
    back to the genome.  Over whole-contig regions the histograms sum to the partition's
    background counts of the table, and the expected counts equal the host's."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(31)
    contigs = [("a", R.random_seq(rng, 60_000, lower=0.2, invalid=0.001, letters="AACGTTT")),
               ("b", R.random_seq(rng, 30_001, letters="ACCGGT"))]
    cg = np.flatnonzero(np.isin(contigs[0][1] & 0xDF, (ord("C"), ord("G"))))
    sites = {"a": np.concatenate([rng.choice(cg, size=4000, replace=False), rng.choice(60_000, size=500, replace=False)]),
             "b": rng.choice(30_001, size=500, replace=False)}
    table = C.count_table(contigs, 5, sites=sites)
    gp, alpha, penalty = "NNMNN", 2.0, 3.0
    full = table.zero_filled(gp)
    _, M, U = full.match_rows(gp)
    beta = score_utils.get_betas(alpha, int(sum(M)), int(sum(U)))
    dev.greedy(gp, np.array(M, np.uint64), np.array(U, np.uint64), [(-1, -1, alpha, beta, penalty)])
    leaves = sorted(engine.word_pattern(w, 5) for w in dev.greedy_leaves(0))
    assert 1 < len(leaves) < 512
    pp = PatternPartition(list(leaves), superPattern=gp)
    counts = pp.counts(full)  # per pattern (M, U), the patterns sorted as `leaves`
    rates = [(m + 0.5) / (m + u + 1.0) for m, u in counts]
    regions = {name: [(0, seq.shape[0])] for name, seq in contigs}
    got = predict.region_counts(contigs, leaves, regions, rates)
    host = predict.region_counts(contigs, leaves, regions, rates, host=True)
    hist = sum(got[name][0][0] for name, _ in contigs)
    assert hist.tolist() == [m + u for m, u in counts]
    for name, _ in contigs:
        assert got[name][2].tobytes() == host[name][2].tobytes() and got[name][0].tobytes() == host[name][0].tobytes()
    assert sum(float(got[name][2][0]) for name, _ in contigs) == sum(float(host[name][2][0]) for name, _ in contigs)
