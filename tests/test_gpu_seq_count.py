"""k-mer context counts on the GPU (kp_seq_scan_kernel, kp_seq_sites_kernel) against the host
session of the same per-base code (engine.seq_host, itself pinned to an independent oracle in
tests/test_seq_count.py).  Bar: both count columns and every count stat equal, on both
accumulation paths and every knob setting; the path a case ran is asserted from the session's
stats, so a silent fallback cannot pass for the path under test."""
import numpy as np
import pytest

from kmerpapa_amd import count as C
from kmerpapa_amd import engine, score_utils
from kmerpapa_amd.papa import PatternPartition
from tests import seq_ref as R

pytestmark = pytest.mark.gpu

LDS, GLOBAL = engine.SEQ_PATH_LDS, engine.SEQ_PATH_GLOBAL
KNOBS = ("KP_SEQ_GLOBAL", "KP_SEQ_LDS_K", "KP_SEQ_GRID", "KP_SEQ_MERGE")
THREADS = 256  # of a scan workgroup: a thread owns tile / 256 consecutive centres


@pytest.fixture(scope="module")
def dev():
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine.get_device(engine.visible_devices()[0])


@pytest.fixture(scope="module")
def tile(dev):
    dev.seq_begin(1, False)
    dev.seq_end(False, False)
    t = dev.seq_stats()["tile"]
    assert t >= THREADS and t % THREADS == 0
    return t


def _set(monkeypatch, env):
    for key in KNOBS:
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))


_host_cache = {}


def _host(key, k, fold, jobs):
    """The host session of a case, computed once and shared by the knob settings."""
    if key not in _host_cache:
        _host_cache[key] = engine.seq_host(k, fold, jobs)
    return _host_cache[key]


def _same(got, ref):
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert {x: got[2][x] for x in R.COUNT_STATS} == {x: ref[2][x] for x in R.COUNT_STATS}
    assert got[2]["items"] == ref[2]["items"] and got[2]["tile"] == ref[2]["tile"]


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


@pytest.mark.parametrize("env,path", [({}, LDS), ({"KP_SEQ_GLOBAL": 1}, GLOBAL),
                                      ({"KP_SEQ_GLOBAL": 1, "KP_SEQ_MERGE": 0}, GLOBAL)],
                         ids=["lds", "global", "global_unmerged"])
@pytest.mark.parametrize("k", [3, 5, 7])
def test_boundary_contig_small_k(dev, tile, monkeypatch, k, env, path):
    _set(monkeypatch, env)
    seq = _boundary_contig(tile, k)
    got = dev.seq_count(k, True, [(seq, None, None)])
    _same(got, _host(("b", k), k, True, [(seq, None, None)]))
    assert got[2]["path"] == path and got[2]["items"] == 4 and got[2]["scan_ms"] > 0
    assert 0 < got[2]["windows_invalid"] < 40 * k * k


@pytest.mark.parametrize("merge", [1, 0], ids=["merged", "unmerged"])
@pytest.mark.parametrize("k,fold", [(9, True), (11, True), (8, False), (10, False)])
def test_boundary_contig_large_k(dev, tile, monkeypatch, k, fold, merge):
    _set(monkeypatch, {"KP_SEQ_MERGE": merge})
    seq = _boundary_contig(tile, k)
    got = dev.seq_count(k, fold, [(seq, None, None)])
    _same(got, _host(("b", k, fold), k, fold, [(seq, None, None)]))
    assert got[2]["path"] == GLOBAL


def test_threshold_moved(dev, tile, monkeypatch):
    """KP_SEQ_LDS_K = 5: k = 5 is the largest LDS k, k = 6 and 7 the smallest global ones."""
    for k, fold, path in ((5, True, LDS), (6, False, GLOBAL), (7, True, GLOBAL), (4, False, LDS)):
        _set(monkeypatch, {"KP_SEQ_LDS_K": 5})
        seq = _boundary_contig(tile, k)
        got = dev.seq_count(k, fold, [(seq, None, None)])
        _same(got, _host(("b", k, fold), k, fold, [(seq, None, None)]))
        assert got[2]["path"] == path, k
    _set(monkeypatch, {"KP_SEQ_LDS_K": 0})
    got = dev.seq_count(1, False, [(seq, None, None)])
    assert got[2]["path"] == GLOBAL and int(got[1].sum()) == got[2]["windows"]
    _set(monkeypatch, {"KP_SEQ_LDS_K": 8})  # 4^8 counters do not fit beside a second workgroup's
    with pytest.raises(engine.KPError) as e:
        dev.seq_count(3, True, [(seq, None, None)])
    assert e.value.code == -1


@pytest.mark.parametrize("k,env,path", [(5, {}, LDS), (7, {}, LDS), (7, {"KP_SEQ_GLOBAL": 1}, GLOBAL), (9, {}, GLOBAL),
                                        (9, {"KP_SEQ_MERGE": 0}, GLOBAL), (7, {"KP_SEQ_GRID": 1}, LDS)],
                         ids=["lds5", "lds7", "global7", "global9", "global9_unmerged", "lds7_one_workgroup"])
def test_low_complexity(dev, monkeypatch, k, env, path):
    """A 200,000-base homopolymer, then a dinucleotide repeat: whole waves hold one code (merged
    into one add, or 64 adds to one address), and LDS counters pass 2^16 (with one workgroup the
    homopolymer's counter holds them all)."""
    _set(monkeypatch, env)
    seq = np.concatenate([np.full(200_000, ord("a"), np.uint8), np.frombuffer(b"CA" * 30_000, np.uint8),
                          np.frombuffer(b"N", np.uint8), np.full(70_001, ord("G"), np.uint8)])
    got = dev.seq_count(k, True, [(seq, None, None)])
    _same(got, _host(("low", k), k, True, [(seq, None, None)]))
    assert got[2]["path"] == path and int(got[1].max()) > 200_000 - k > 1 << 16


def test_regions_at_tile_boundaries(dev, tile, monkeypatch):
    """Regions of tile - 1, tile and tile + 1 centres, one that ends where the next begins, one
    base long, at both ends of the contig; then with one workgroup walking every item."""
    k = 7
    n = 6 * tile + 50
    seq = R.random_seq(np.random.RandomState(17), n, lower=0.1, invalid=0.001)
    t = tile
    regions = np.array([(0, 5), (5, 5 + t - 1), (t + 10, 2 * t + 10), (2 * t + 10, 3 * t + 11), (3 * t + 40, 3 * t + 41),
                        (4 * t, 4 * t), (4 * t + 3, 5 * t + 2), (5 * t + 3, 5 * t + 3 + 2 * t // THREADS), (n - 6, n)])
    ref = _host("regions", k, True, [(seq, regions, None)])
    for env in ({}, {"KP_SEQ_GLOBAL": 1}, {"KP_SEQ_GRID": 1}, {"KP_SEQ_GRID": 3, "KP_SEQ_GLOBAL": 1}):
        _set(monkeypatch, env)
        got = dev.seq_count(k, True, [(seq, regions, None)])
        _same(got, ref)
        assert got[2]["path"] == (GLOBAL if "KP_SEQ_GLOBAL" in env else LDS) and got[2]["items"] == 9
    whole = dev.seq_count(k, True, [(seq, None, None)])
    assert whole[2]["items"] == 7
    _same(whole, _host("regions_whole", k, True, [(seq, None, None)]))


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
                     (3, None), (11, [(0, n)]), (5, [(n - 3, n - 2)])]
            for k, regions in cases:
                jobs = [(seq, None if regions is None else np.array(regions), [0, n - 1, n // 2])]
                ref = engine.seq_host(k, True, jobs)
                for env, path in (({}, LDS if k <= 7 else GLOBAL), ({"KP_SEQ_GLOBAL": 1}, GLOBAL),
                                  ({"KP_SEQ_GLOBAL": 1, "KP_SEQ_MERGE": 0}, GLOBAL)):
                    _set(monkeypatch, env)
                    got = own.seq_count(k, True, jobs)
                    _same(got, ref)
                    assert got[2]["path"] == (path if got[2]["items"] else 0)
    finally:
        own.close()


def test_three_contigs_one_session(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    rng = np.random.RandomState(23)
    parts = [R.random_seq(rng, n, lower=0.2, invalid=0.002) for n in (tile + 3, 40, 2 * tile + 1)]
    for k, fold in ((5, True), (9, True)):
        jobs = [(p, None, [0, 5, 5, p.shape[0] - 1, p.shape[0] // 2]) for p in parts]
        got = dev.seq_count(k, fold, jobs)
        _same(got, engine.seq_host(k, fold, jobs))
        singles = [dev.seq_count(k, fold, [j]) for j in jobs]
        assert np.array_equal(got[0], sum(s[0] for s in singles)) and np.array_equal(got[1], sum(s[1] for s in singles))
        assert got[2]["windows"] == sum(s[2]["windows"] for s in singles)


def test_sites_at_tile_boundaries(dev, tile, monkeypatch):
    _set(monkeypatch, {})
    rng = np.random.RandomState(29)
    n = 2 * tile + 9
    seq = R.random_seq(rng, n, lower=0.3, invalid=0.003)
    sites = [0, 1, n - 1, n - 2] + [b + d for b in (tile, 2 * tile, 255, 256, 257) for d in (-1, 0, 0, 1, 4)]
    sites += rng.randint(0, n, size=1000).tolist() + [tile] * 70
    for k, fold in ((3, True), (7, True), (11, True), (4, False)):
        got = dev.seq_count(k, fold, [(seq, False, sites)])
        _same(got, engine.seq_host(k, fold, [(seq, False, sites)]))
        assert got[2]["sites"] + got[2]["sites_skipped"] == len(sites) and got[2]["sites_skipped"] > 0
        assert got[2]["path"] == 0 and not got[1].any()


def test_second_session_and_errors(dev, tile, monkeypatch):
    """The table is zeroed again and the arena reused; calls out of order are KP_E_STATE, and
    kp_greedy / kp_apply refuse to take the arena while a session holds its table in it."""
    _set(monkeypatch, {})
    seq = _boundary_contig(tile, 9)
    first = dev.seq_count(9, True, [(seq, None, [5, 6])])
    for k in (9, 5, 11, 9):
        got = dev.seq_count(k, True, [(seq, None, [5, 6])])
        _same(got, _host(("second", k), k, True, [(seq, None, [5, 6])]))
    assert np.array_equal(got[1], first[1])
    for call in (lambda: dev.seq_scan(seq), lambda: dev.seq_sites(seq, [1]), lambda: dev.seq_end()):
        with pytest.raises(engine.KPError) as e:
            call()
        assert e.value.code == -4
    for k, fold in ((16, False), (0, False), (8, True)):
        with pytest.raises(engine.KPError) as e:
            dev.seq_begin(k, fold)
        assert e.value.code == -1
    dev.seq_begin(3, True)
    try:
        with pytest.raises(engine.KPError) as e:
            dev.seq_begin(3, True)
        assert e.value.code == -4
        with pytest.raises(engine.KPError) as e:
            dev.greedy("NN", np.ones(16, np.uint64), np.ones(16, np.uint64), [(-1, -1, 1.0, 1.0, 1.0)])
        assert e.value.code == -4
        with pytest.raises(engine.KPError) as e:
            dev.apply(2, [engine.pattern_word("NN")], engine.pattern_word("NN"), [0], [1], [1])
        assert e.value.code == -4
        for bad in ([(10, 20), (5, 8)], [(0, seq.shape[0] + 1)]):
            with pytest.raises(engine.KPError) as e:
                dev.seq_scan(seq, np.array(bad))
            assert e.value.code == -1
        with pytest.raises(engine.KPError) as e:
            dev.seq_sites(seq, [seq.shape[0]])
        assert e.value.code == -1
        dev.seq_scan(seq[:100])
    finally:
        pos, bg = dev.seq_end()
    assert not pos.any() and int(bg.sum()) == dev.seq_stats()["windows"] == 98


def test_command_line_on_the_gpu(dev, monkeypatch, tmp_path):
    """kmerpapa-count's two subcommands on their default (GPU) path write what the host path writes."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(37)
    contigs = [("chr1", R.random_seq(rng, 20_011, lower=0.3, invalid=0.002)), ("chr2", R.random_seq(rng, 9_000))]
    fa, tb = str(tmp_path / "g.fa"), str(tmp_path / "g.2bit")
    R.write_fasta(fa, [(n, np.where(np.isin(s & 0xDF, list(b"ACGT")), s, ord("N")).astype(np.uint8)) for n, s in contigs])
    R.write_2bit(tb, contigs, ">")
    with open(tmp_path / "r.bed", "w") as f:
        f.write("chr1 100 9000\nchr1 8000 20011\nchr2 0 10\n")
    with open(tmp_path / "m.txt", "w") as f:
        for p in (rng.choice(8_990, size=500, replace=False) + 5).tolist():  # (every window inside the contig)
            ref = chr(contigs[1][1][p]).upper()
            f.write(f"chr2 {p + 1} {ref} {'ACGT'[('ACGT'.index(ref) + 1) % 4]}\n")
    out = {}
    for host in (False, True):
        for name, argv in (("bg", ["background", tb, "--bed", str(tmp_path / "r.bed"), "--radius", "3"]),
                           ("bg_fa", ["background", fa, "-k", "9"]), ("snv", ["snv", fa, str(tmp_path / "m.txt"), "-k", "5"])):
            path = str(tmp_path / f"{name}{int(host)}.txt")
            assert C.main(argv + ["-o", path, "--verbosity", "0"], host=host) == 0
            out[name, host] = open(path).read()
    for name in ("bg", "bg_fa", "snv"):
        assert out[name, False] == out[name, True] and len(out[name, False]) > 1000
    assert sum(int(x.split()[1]) for x in out["snv", False].splitlines()) == 500


def test_count_table_feeds_greedy_and_apply(dev, monkeypatch):
    """End to end on the GPU: count a genome and its sites, fit the greedy partition on the
    table, and sum the table's counts per pattern."""
    _set(monkeypatch, {})
    rng = np.random.RandomState(31)
    contigs = [("a", R.random_seq(rng, 60_000, lower=0.2, invalid=0.001, letters="AACGTTT")),
               ("b", R.random_seq(rng, 30_001, letters="ACCGGT"))]
    # (most mutations at C or G, so the rate depends on the context and the partition splits)
    cg = np.flatnonzero(np.isin(contigs[0][1] & 0xDF, (ord("C"), ord("G"))))
    sites = {"a": np.concatenate([rng.choice(cg, size=4000, replace=False), rng.choice(60_000, size=500, replace=False)]),
             "b": rng.choice(30_001, size=500, replace=False)}
    table = C.count_table(contigs, 5, sites=sites)
    host = C.count_table(contigs, 5, sites=sites, host=True)
    assert np.array_equal(table.codes, host.codes) and np.array_equal(table.M, host.M) and np.array_equal(table.U, host.U)
    gp, alpha, penalty = "NNMNN", 2.0, 3.0
    full = table.zero_filled(gp)
    _, M, U = full.match_rows(gp)
    beta = score_utils.get_betas(alpha, int(sum(M)), int(sum(U)))
    dev.greedy(gp, np.array(M, np.uint64), np.array(U, np.uint64), [(-1, -1, alpha, beta, penalty)])
    leaves = [engine.word_pattern(w, 5) for w in dev.greedy_leaves(0)]
    assert 1 < len(leaves) < 512
    pp = PatternPartition(list(leaves), superPattern=gp)
    counts = pp.counts(full)
    assert counts == full.pattern_counts([str(p) for p in pp.patterns])
    assert sum(m for m, _ in counts) == int(table.M.sum()) and sum(u for _, u in counts) == int(table.U.sum())
