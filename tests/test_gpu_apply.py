"""A fitted partition applied to a count table on the GPU (kp_apply) against the host run of
the same per-row / per-pair / per-term code (kp_apply_host, itself pinned to brute force and
the reference's recorded runs in tests/test_apply.py).  Bar: pid, per-pattern counts, the four
error counts and the bytes of ll all equal, on every accumulation path; the path a case ran
is asserted from the call's stats, so a silent fallback cannot pass for the path under test."""
import numpy as np
import pytest

from kmerpapa_amd import apply as A
from kmerpapa_amd import engine, score_utils
from kmerpapa_amd.io_utils import KmerCounts
from kmerpapa_amd.papa import PatternPartition
from tests import apply_cases as C

pytestmark = pytest.mark.gpu

# accumulation paths: environment, and the (tiles > 0, lds_counters) the stats must show
# (None: kp_apply's own choice, _own_choice)
PATHS = {
    "default": ({}, (True, None)),
    "global": ({"KP_APPLY_GLOBAL": "1"}, (True, 0)),
    "lds_off": ({"KP_APPLY_LDS": "0"}, (True, 0)),
    "lds_on": ({"KP_APPLY_LDS": "1"}, (True, 1)),
    "scalar_lds": ({"KP_APPLY_TILE": "0", "KP_APPLY_LDS": "1"}, (False, 1)),
    "scalar_global": ({"KP_APPLY_TILE": "0", "KP_APPLY_GLOBAL": "1"}, (False, 0)),
}


@pytest.fixture(scope="module")
def dev():
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine.get_device(engine.visible_devices()[0])


def _set(monkeypatch, env):
    for key in ("KP_APPLY_TILE", "KP_APPLY_GLOBAL", "KP_APPLY_LDS", "KP_APPLY_GRID"):
        monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        monkeypatch.setenv(key, v)


def _own_choice(n, P, ncol, grid_cap=None):
    """What kp_apply does when nothing is forced and the counters fit LDS (include/kmerpapa_hip.h):
    LDS counters where the workgroups' flushes, workgroups x 2 P ncol, are no more global
    atomics than the 2 n ncol of adding every row directly.  512 rows per workgroup and step;
    every table here has fewer row blocks than the GPU holds workgroups."""
    blocks = -(-n // 512)
    return int(min(blocks, grid_cap or blocks) * 2 * P * ncol <= 2 * n * ncol)


def _both(dev, names, super_pat, k, codes, M, U, rates=None):
    """(GPU result, host result) in comparable form, and the GPU call's stats."""
    args = (k, C.words(names), engine.pattern_word(super_pat), codes, M, U, rates)
    got = dev.apply(*args)
    return C.observed(got), C.observed(engine.apply_host(*args)), got[4]


@pytest.mark.parametrize("which", C.GOLDEN, ids=[x[1] for x in C.GOLDEN])
def test_recorded_runs(dev, which):
    rec, (names, counts, rates) = C.golden(which)
    table, gp = C.table5()
    pid, pM, pU, ll, st = A.apply_partition(names, table, rates)
    assert C.observed((pid, pM, pU, ll, st)) == C.observed(A.apply_partition(names, table, rates, host=True))
    assert list(zip(pM.tolist(), pU.tolist())) == counts and C.bits(ll) == C.bits([C.recorded_ll(rec)])
    assert st["lds_counters"] == 1 and st["tiles"] == 1


@pytest.mark.parametrize("part", range(4))
def test_random_partitions_tile_of_8(dev, part, monkeypatch):
    """The 200 seeded cases with 8 patterns per tile: 1..4 tiles, P = 7, 8, 9 among them."""
    _set(monkeypatch, {"KP_APPLY_TILE": "8", "KP_APPLY_LDS": "1"})
    for i, (names, gp, k, codes, M, U, rates) in enumerate(C.random_cases()):
        if i % 4 != part:
            continue
        got, host, st = _both(dev, names, gp, k, codes, M, U, rates)
        assert got == host, (i, gp, names)
        assert st["tiles"] == (len(names) + 7) // 8 and st["lds_counters"] == 1
        if i % 16 == part:
            assert got == C.expected(C.random_expected(i))


def _rows_case(n, ncol, seed=11):
    """``n`` random rows of the 7-mer table against a 27-pattern partition of NNNNNNN."""
    rng = np.random.RandomState(seed)
    names = C.split_partition(rng, "NNNNNNN", 27)
    codes = np.sort(rng.choice(4 ** 7, size=n, replace=False)).astype(np.uint64)
    M = rng.randint(0, 1 << 40, size=(n, ncol), dtype=np.int64)
    U = rng.randint(0, 1 << 40, size=(n, ncol), dtype=np.int64)
    if ncol == 1:
        M, U = M[:, 0], U[:, 0]
    return names, "NNNNNNN", 7, codes, M, U, rng.uniform(0.001, 0.3, size=len(names))


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_row_counts_on_every_path(dev, n, path, monkeypatch):
    env, (tiled, ldsc) = PATHS[path]
    _set(monkeypatch, dict(env, KP_APPLY_TILE=env.get("KP_APPLY_TILE", "16")))
    got, host, st = _both(dev, *_rows_case(n, 1))
    assert got == host
    assert (st["tiles"], st["lds_counters"]) == (2 if tiled else 0, _own_choice(n, 27, 1) if ldsc is None else ldsc)
    assert _own_choice(1, 27, 1) == 0 and _own_choice(63, 27, 1) == 1


@pytest.mark.parametrize("path", sorted(PATHS))
def test_three_columns_and_several_steps(dev, path, monkeypatch):
    """ncol = 3 on every path, with the grid capped at 2 workgroups: 4,097 rows are 9 row
    blocks, so each workgroup runs 5 steps (and one of them past the table's end)."""
    env, (tiled, ldsc) = PATHS[path]
    _set(monkeypatch, dict(env, KP_APPLY_GRID="2"))
    got, host, st = _both(dev, *_rows_case(4097, 3))
    assert got == host
    assert (st["tiles"], st["lds_counters"]) == (1 if tiled else 0, _own_choice(4097, 27, 3, 2) if ldsc is None else ldsc)


def test_forced_lds_counters_that_do_not_fit(dev, monkeypatch):
    """4,096 patterns x 3 columns x 2 x 8 bytes = 196,608 bytes are more than a CU's LDS: the
    default falls back to global atomics (and says so), KP_APPLY_LDS=1 refuses."""
    rng = np.random.RandomState(5)
    names = [x + "NN" for x in C.kmers_of(rng.permutation(4 ** 6), 6)]
    codes = np.arange(0, 4 ** 8, 13, dtype=np.uint64)
    M = rng.randint(0, 1 << 30, size=(codes.shape[0], 3), dtype=np.int64)
    U = rng.randint(0, 1 << 30, size=(codes.shape[0], 3), dtype=np.int64)
    _set(monkeypatch, {})
    got, host, st = _both(dev, names, "N" * 8, 8, codes, M, U)
    assert got == host and (st["tiles"], st["lds_counters"]) == (4, 0)
    _set(monkeypatch, {"KP_APPLY_LDS": "1"})
    with pytest.raises(engine.KPError) as e:
        dev.apply(8, C.words(names), engine.pattern_word("N" * 8), codes, M, U)
    assert e.value.code == -1 and "do not fit LDS" in str(e.value)
    _set(monkeypatch, {"KP_APPLY_LDS": "1", "KP_APPLY_GLOBAL": "1"})
    with pytest.raises(engine.KPError, match="contradict"):
        dev.apply(8, C.words(names[:4]), engine.pattern_word("N" * 8), codes, M, U)
    # one column: 65,536 bytes of counters fit, but 10 workgroups flushing 8,192 counters each
    # are more atomics than 5,041 rows adding two counts: global unless LDS is forced
    assert _own_choice(codes.shape[0], 4096, 1) == 0
    _set(monkeypatch, {})
    got, host, st = _both(dev, names, "N" * 8, 8, codes, M[:, 0], U[:, 0])
    assert got == host and (st["tiles"], st["lds_counters"]) == (4, 0)
    _set(monkeypatch, {"KP_APPLY_LDS": "1"})
    got, host, st = _both(dev, names, "N" * 8, 8, codes, M[:, 0], U[:, 0])
    assert got == host and (st["tiles"], st["lds_counters"]) == (4, 1)


@pytest.mark.parametrize("path", ["default", "global"])
def test_one_pattern_65536_rows(dev, path, monkeypatch):
    """Every row of the 8-mer table adds to the same two 64-bit counters, counts near 2^40."""
    _set(monkeypatch, PATHS[path][0])
    rng = np.random.RandomState(8)
    codes = np.arange(4 ** 8, dtype=np.uint64)
    M = (1 << 40) - rng.randint(1, 1000, size=codes.shape[0], dtype=np.int64)
    U = (1 << 40) - rng.randint(1, 1000, size=codes.shape[0], dtype=np.int64)
    pid, pM, pU, ll, st = dev.apply(8, C.words(["NNNNNNNN"]), engine.pattern_word("NNNNNNNN"), codes, M, U, [0.25])
    assert pM.tolist() == [int(M.sum())] and pU.tolist() == [int(U.sum())] and int(M.sum()) > 1 << 55
    assert not pid.any() and st["unmatched"] == 0 == st["multi"] and st["lds_counters"] == (path == "default")
    assert C.bits(ll) == C.bits(engine.apply_host(8, C.words(["NNNNNNNN"]), 0xffffffff, codes, M, U, [0.25])[3])


def test_sparse_16mers(dev):
    names, codes, M, U = C.sparse16()
    got, host, st = _both(dev, names, "N" * 16, 16, codes, M, U, np.linspace(1e-5, 0.01, len(names)))
    assert got == host and got[4]["unmatched"] == 0 and sum(x[0] for x in got[1]) == int(M.sum())


@pytest.mark.parametrize("kind", C.BROKEN)
def test_broken_partitions(dev, kind):
    names, sup, k, codes, M, U, kmers = C.broken_case(kind)
    got, host, _ = _both(dev, names, sup, k, codes, M, U)
    assert got == host == C.expected(C.brute(names, sup, kmers, M, U, None))


def test_pairs_over_many_blocks(dev):
    """700 patterns (3 blocks of the pair kernel) with 40 duplicates spread among them."""
    rng = np.random.RandomState(9)
    names = C.split_partition(rng, "N" * 8, 660)
    names += [names[int(j)] for j in rng.choice(660, size=40, replace=False)]
    names = [names[int(j)] for j in rng.permutation(700)]
    z = np.zeros(0, np.int64)
    got, host, _ = _both(dev, names, "NNNNNNNM", 8, np.zeros(0, np.uint64), z, z)
    assert got == host and got[4]["overlap_pairs"] == 40 and got[4]["outside_super"] > 0


def test_edges_and_errors(dev):
    z = np.zeros(0, np.int64)
    got, host, st = _both(dev, ["NA", "NC", "NK"], "NN", 2, np.zeros(0, np.uint64), z, z, [0.5, 0.0, 1.0])
    assert got == host and got[3] == C.bits([0.0])
    got, host, st = _both(dev, ["NM"], "NM", 2, C.codes_of(["AA", "CG", "TC"]), [1, 2, 4], [8, 16, 32], [0.1])
    assert got == host and got[0] == [0, -1, 0]
    for what in sorted(C.BAD):
        with pytest.raises(engine.KPError) as e:
            C.bad_call(dev.apply, what)
        assert e.value.code == -1, what


def _table4096():
    rng = np.random.RandomState(77)
    bg = rng.randint(1, 30000, size=(4096, 3))
    M = rng.binomial(bg, rng.uniform(0.001, 0.05, size=(4096, 1))).astype(np.uint64)
    return M.sum(axis=1), bg.astype(np.uint64).sum(axis=1)


def test_greedy_fit_then_apply(dev):
    """End to end: the greedy partition of a 4,096-k-mer table, then the class on the same
    table: the counts of KmerCounts.pattern_counts and the loss of score_utils.get_loss."""
    gp, alpha, penalty = "NNNNNN", 2.0, 5.0
    M, U = _table4096()  # rows in matches(gp) order: position 0 fastest
    beta = score_utils.get_betas(alpha, int(M.sum()), int(U.sum()))
    dev.greedy(gp, M, U, [(-1, -1, alpha, beta, penalty)])
    leaves = [engine.word_pattern(w, 6) for w in dev.greedy_leaves(0)]
    assert 10 < len(leaves) < 4096
    row = np.arange(4096)
    code = sum(((row >> (2 * i)) & 3) << (2 * (5 - i)) for i in range(6))  # position i is letter i of the code
    order = np.argsort(code)
    table = KmerCounts(6, code[order], M[order], U[order])
    pp = PatternPartition(list(leaves), superPattern=gp)
    names = [str(p) for p in pp.patterns]
    counts = pp.counts(table)
    assert counts == table.pattern_counts(names) and counts == pp.counts(table, host=True)
    rates = [(m + alpha) / (m + u + alpha + beta) for m, u in counts]
    assert C.bits(pp.loglik(table, rates)) == C.bits(score_utils.get_loss(counts, alpha, beta))
    assert pp.check() == {"unmatched": 0, "multi": 0, "overlap_pairs": 0, "outside_super": 0}
    assert (pp.assign(table) >= 0).all()
