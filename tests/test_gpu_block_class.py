"""The class order of the block list on the GPU: a pass gives the oracle's cells under the
class order and under the plain one, the two agree bit for bit (cells, roots, leaf counts,
the fit's partition), and the device builds the list the host sorts.

Lattice: NNMNNN at max_block 16 -- one low position, five high (N M N N N): the slab is
(M, N, N), the two fast positions are N's with four digit levels each, so every part of the
key (class, digits without siblings, doubles, triples) orders blocks; 151,875 blocks of 15
cells, 14 high levels.  Bar: every cell of every lane and every root bit for bit (any NaN
equals any NaN)."""
import numpy as np
import pytest

from tests import build_cases as BC
from tests.fixtures import bits_equal

pytestmark = pytest.mark.gpu

GP, MAX_BLOCK = "NNMNNN", 16
ITYPES = {"uint32": np.uint32, "uint64": np.uint64}
ORDERS = {"class": "1", "plain": "0"}


@pytest.fixture(scope="module")
def eng():
    from kmerpapa_amd import engine
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine


_tables = {}


def _table(itype):
    """Seeded 3-fold counts of GP (scale 2e3 for uint32; 1e7 for uint64, one k-mer in eight
    scaled down so that the two alphas of a mixed group differ in float32), built once."""
    key = np.dtype(itype).name
    if key not in _tables:
        from kmerpapa_amd import engine
        from kmerpapa_amd.CV_tools import fold_tables
        from kmerpapa_amd.pattern_utils import generality, matches
        rng = np.random.RandomState(len(GP))
        scale = 1e7 if itype == np.uint64 else 2e3
        ctx = {}
        for k in matches(GP):
            bg = int(rng.poisson(scale * rng.lognormal(0, 0.5)))
            if itype == np.uint64 and rng.rand() < 0.125:
                bg = int(bg * 10.0 ** -rng.uniform(3, 7))
            ctx[k] = (int(rng.binomial(bg, 0.01 * rng.lognormal(0, 0.4))), bg)
        if itype == np.uint64:
            assert sum(m + u for m, u in ctx.values()) > 2 ** 32
        contexts, Mf, Uf = fold_tables(ctx, BC.NF, np.random.RandomState(3), itype)
        Mk, Uk = engine.counts_in_kmer_order(GP, contexts, Mf, Uf, generality(GP), itype)
        tot_m = Mf.sum(axis=0).astype(np.uint64)
        tot_u = Uf.sum(axis=0).astype(np.uint64)
        mtr, utr = tot_m.sum() - tot_m, tot_u.sum() - tot_u
        _tables[key] = dict(ctx=ctx, contexts=contexts, Mf=Mf, Uf=Uf, Mk=Mk, Uk=Uk, my=mtr / (mtr + utr),
                            bits=64 if itype == np.uint64 else 32, refs={})
    return _tables[key]


def _betas(case, alpha):
    return (alpha * (1.0 - case["my"])) / case["my"]


def _ref(case, alpha, pen):
    """oracle.cv_pass of one (alpha, penalty) over every fold, computed once and read-only."""
    key = (alpha, pen)
    if key not in case["refs"]:
        from oracle import oracle as O
        r = O.cv_pass(GP, case["contexts"], case["Mf"], case["Uf"], alpha, _betas(case, alpha), pen, case["bits"])
        for a in (r["score"], r["root_train"], r["root_test"]):
            a.setflags(write=False)
        case["refs"][key] = (r["score"], r["root_train"], r["root_test"])
    return case["refs"][key]


def _pass(eng, monkeypatch, order, case, groups, width, cut):
    """One pass under block order ``order``: the device list against the host's, then every
    lane's cells, the roots and the leaf counts."""
    monkeypatch.setenv("KP_BLOCK_CLASS", ORDERS[order])
    monkeypatch.setenv("KP_LANES_PER_WG", str(width))
    plan = eng.Plan(eng.get_device(0), GP, MAX_BLOCK)
    try:
        assert plan.info["nblocks"] == 151875 and plan.info["block"] == 15 and plan.info["high_levels"] == 14
        assert plan.block_check() == 0
        plan.set_counts(case["Mk"], case["Uk"])
        assert plan.info["lanes_per_workgroup"] == width
        assert eng.device_groups(groups, width) == cut
        rt, re, nlv = plan.run(groups)
        # (every cell through kp_gather_cells: kp_dump_lane copies block by block, seconds per
        # lane at 151,875 blocks)
        cells = np.arange(plan.info["npat"], dtype=np.uint64)
        scores = [plan.gather_cells(lane, cells) for lane in range(len(rt))]
    finally:
        plan.close()
    return scores, rt, re, nlv


@pytest.mark.parametrize("kind", ["2", "2+1"])
@pytest.mark.parametrize("itype", sorted(ITYPES))
def test_cv_pass_equals_oracle_under_both_orders(eng, monkeypatch, itype, kind):
    case = _table(ITYPES[itype])
    beta_of = lambda a, f: float(_betas(case, a)[f])  # noqa: E731
    if kind == "2":
        width, groups = 2, BC.single_groups(2, beta_of)
        cut = [(q * 2, 2, 0) for q in range(BC.NF)]
    else:
        width, groups = 3, BC.mixed_groups(2, 1, beta_of)
        cut = [(q * 3, 3, 1) for q in range(BC.NF)]
    lanes = [(f, a, pen) for f, a, _b, pens in groups for pen in pens]
    runs = {order: _pass(eng, monkeypatch, order, case, groups, width, cut) for order in ORDERS}
    for order, (scores, rt, re, _nlv) in runs.items():
        assert len(scores) == len(lanes)
        for lane, (f, alpha, pen) in enumerate(lanes):
            score, root_train, root_test = _ref(case, alpha, pen)
            assert bits_equal(scores[lane], score[:, f]), (order, lane, f, alpha, pen)
            assert bits_equal(rt[lane], root_train[f]), (order, lane)
            assert bits_equal(re[lane], root_test[f]), (order, lane)
    a, b = runs["class"], runs["plain"]
    for lane in range(len(lanes)):
        assert bits_equal(a[0][lane], b[0][lane]), lane
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3])


@pytest.mark.parametrize("itype", sorted(ITYPES))
def test_fit_partition_is_the_same_under_both_orders(eng, monkeypatch, itype):
    """All-data counts, two fit lanes: root, leaf count and the partition (names and order)
    equal oracle.fit's under both orders."""
    from kmerpapa_amd.pattern_utils import PatternEnumeration, generality
    from oracle import oracle as O
    dt = ITYPES[itype]
    case = _table(dt)
    contexts = list(case["ctx"])
    M = np.array([case["ctx"][k][0] for k in contexts], dt)
    U = np.array([case["ctx"][k][1] for k in contexts], dt)
    Mk, Uk = eng.counts_in_kmer_order(GP, contexts, M, U, generality(GP), dt)
    nm, nu = int(M.sum(dtype=np.uint64)), int(U.sum(dtype=np.uint64))
    beta = (BC.ALPHA1 * (1.0 - nm / (nm + nu))) / (nm / (nm + nu))
    pens = [3.0, 9.0]
    groups = [(-1, BC.ALPHA1, beta, pens)]
    PE = PatternEnumeration(GP)
    want = [O.fit(GP, contexts, M, U, BC.ALPHA1, beta, pen, case["bits"]) for pen in pens]
    got = {}
    for order in ORDERS:
        monkeypatch.setenv("KP_BLOCK_CLASS", ORDERS[order])
        plan = eng.Plan(eng.get_device(0), GP, MAX_BLOCK)
        try:
            plan.set_counts(Mk, Uk)
            rt, _re, nlv = plan.run(groups)
            leaves = [[int(x) for x in plan.leaves(lane)] for lane in range(len(pens))]
        finally:
            plan.close()
        for lane, (score, _rm, _ru, names, _arr) in enumerate(want):
            assert bits_equal(rt[lane], np.float32(score)), (order, lane)
            assert int(nlv[lane]) == len(names), (order, lane)
            assert [PE.num2pattern(x) for x in leaves[lane]] == names, (order, lane)
        got[order] = (rt, nlv, leaves)
    assert bits_equal(got["class"][0], got["plain"][0])
    assert np.array_equal(got["class"][1], got["plain"][1])
    assert got["class"][2] == got["plain"][2]
