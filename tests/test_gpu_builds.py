"""Every build of the sweep the dispatcher can launch, against the CPU oracle.

kp_pass.h picks among the builds of kp_dp_kernel<CT, NL, HZ, MIX>: 32- or 64-bit counts, 1 to 8
lanes per workgroup, with or without a second (alpha, beta) set for the last lanes, with or
without the k-mer code.  They differ in their log, their pair-list decode, their gather shape,
their LDS table sizes and in where the first second-set lane (js) falls, so each is run here on
its own: one pass over NNMNN at the default block (151,875 cells, 675-cell blocks: levels wider
than 512 / NL cells and narrow top levels, so the thread-per-cell, lane-split and pair-split
paths all run; 7 high levels, each with blocks, so the builds with and without the k-mer code
both launch).  Bar: every cell of every lane and every root bit for bit (any NaN equals any
NaN).  Every case asserts, from the plan's info, the host's cut and the launch count, that the
build it names is the one that ran.
"""
import numpy as np
import pytest

from tests import build_cases as BC
from tests.fixtures import bits_equal

pytestmark = pytest.mark.gpu

GP = "NNMNN"
ITYPES = {"uint32": np.uint32, "uint64": np.uint64}
# The 64-bit table's sparse tail.  With every k-mer at 1e7 counts the pseudo counts vanish in
# float32: the oracle's arrays for alpha 0.5 and alpha 2.0 are then equal in all 151,875 cells of
# every fold (measured on the host), and no test could tell that a mixed workgroup had ignored
# its second (alpha, beta) set.  So one k-mer in eight of the 64-bit tables is scaled down to
# 1..1e4 counts (as whole-genome tables hold rare k-mers beside common ones); the total stays
# above 2^32 (4.9e9) and the two alphas' arrays differ in 300 to 15,000 cells per fold.  The
# roots (~5e8, one float32 ulp = 32) still agree between the alphas to 0-2 ulp, which is why
# the product-path case below compares cells too, not only roots.
SPARSE = 0.125


@pytest.fixture(scope="module")
def eng():
    from kmerpapa_amd import engine
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine


# ---- counts and oracle passes, built once per module run ----
_tables = {}


def _table(gp, itype, empty=False):
    """Seeded 3-fold counts of ``gp`` (as test_gpu_parity.test_1lane_sweep_vs_oracle builds
    them: scale 2e4 for uint32, 1e7 for uint64, the latter with the SPARSE tail; ``empty``:
    10 % of the k-mers without counts)."""
    key = (gp, np.dtype(itype).name, empty)
    if key not in _tables:
        from kmerpapa_amd import engine
        from kmerpapa_amd.CV_tools import fold_tables
        from kmerpapa_amd.pattern_utils import generality, matches
        rng = np.random.RandomState(len(gp))
        scale = 1e7 if itype == np.uint64 else 2e4
        ctx = {}
        for k in matches(gp):
            bg = int(rng.poisson(scale * rng.lognormal(0, 0.5)))
            if itype == np.uint64 and rng.rand() < SPARSE:
                bg = int(bg * 10.0 ** -rng.uniform(3, 7))
            ctx[k] = (int(rng.binomial(bg, 0.01 * rng.lognormal(0, 0.4))), bg)
            if empty and rng.rand() < 0.1:
                ctx[k] = (0, 0)
        if itype == np.uint64:
            assert sum(m + u for m, u in ctx.values()) > 2 ** 32
        if empty:
            assert sum(v == (0, 0) for v in ctx.values()) > 10
        contexts, Mf, Uf = fold_tables(ctx, BC.NF, np.random.RandomState(3), itype)
        Mk, Uk = engine.counts_in_kmer_order(gp, contexts, Mf, Uf, generality(gp), itype)
        tot_m = Mf.sum(axis=0).astype(np.uint64)
        tot_u = Uf.sum(axis=0).astype(np.uint64)
        mtr = tot_m.sum() - tot_m
        utr = tot_u.sum() - tot_u
        _tables[key] = dict(gp=gp, ctx=ctx, contexts=contexts, Mf=Mf, Uf=Uf, Mk=Mk, Uk=Uk, my=mtr / (mtr + utr),
                            bits=64 if itype == np.uint64 else 32, refs={})
    return _tables[key]


def _betas(case, alpha):
    return (alpha * (1.0 - case["my"])) / case["my"]


def _beta_of(case):
    return lambda alpha, f: float(_betas(case, alpha)[f])


def _ref(case, alpha, pen):
    """oracle.cv_pass of one (alpha, penalty) over every fold: (score [npat, nf], root_train,
    root_test), computed once per (table, alpha, penalty) and never written to."""
    key = (alpha, pen)
    if key not in case["refs"]:
        from oracle import oracle as O
        r = O.cv_pass(case["gp"], case["contexts"], case["Mf"], case["Uf"], alpha, _betas(case, alpha), pen, case["bits"])
        for a in (r["score"], r["root_train"], r["root_test"]):
            a.setflags(write=False)
        case["refs"][key] = (r["score"], r["root_train"], r["root_test"])
    return case["refs"][key]


def _lanes(groups):
    """(fold, alpha, penalty) of every lane, group-major."""
    return [(f, a, pen) for f, a, _b, pens in groups for pen in pens]


def _run(eng, monkeypatch, case, groups, width, cut, exact=None):
    """One pass of ``groups`` at KP_LANES_PER_WG = ``width``.  Asserts that the plan holds
    ``width`` lanes per workgroup, that the host cuts the groups into ``cut`` and that the pass
    made one launch per high level (so one class of workgroups: the build of ``width`` lanes,
    mixed if ``cut`` says so, with and without the k-mer code).  Returns every lane's score
    array and the roots."""
    monkeypatch.setenv("KP_LANES_PER_WG", str(width))
    if exact is not None:
        monkeypatch.setenv("KP_EXACT_LOGS", str(exact))
    plan = eng.Plan(eng.get_device(0), case["gp"], 0)
    try:
        plan.set_counts(case["Mk"], case["Uk"])
        assert plan.info["lanes_per_workgroup"] == width
        assert plan.info["npat"] == 151875 and plan.info["block"] == 675 and plan.info["nblocks"] == 225
        assert plan.info["high_levels"] == 7
        assert eng.device_groups(groups, width) == cut
        rt, re, nlv = plan.run(groups)
        assert plan.stats()["dp_launches"] == plan.info["high_levels"]
        scores = [plan.dump_lane(lane)[0] for lane in range(len(rt))]
    finally:
        plan.close()
    return scores, rt, re, nlv


def _check_vs_oracle(case, groups, scores, rt, re):
    lanes = _lanes(groups)
    assert len(lanes) == len(scores) == len(rt) == len(re)
    for lane, (f, alpha, pen) in enumerate(lanes):
        score, root_train, root_test = _ref(case, alpha, pen)
        assert bits_equal(scores[lane], score[:, f]), (lane, f, alpha, pen)
        assert bits_equal(rt[lane], root_train[f]), (lane, f, alpha, pen)
        assert bits_equal(re[lane], root_test[f]), (lane, f, alpha, pen)


def _check_reference_tells_lanes_apart(case, groups, cut):
    """The reference-only conditions: within every device group the oracle's arrays of any two
    lanes differ in some cell (a swapped penalty or alpha cannot pass), and where both alphas
    run penalty PENS[0] of a fold, their arrays differ (an ignored second set cannot pass)."""
    lanes = _lanes(groups)
    for lane0, n, _mixed in cut:
        cols = [_ref(case, a, pen)[0][:, f] for f, a, pen in lanes[lane0:lane0 + n]]
        for i in range(n):
            for j in range(i + 1, n):
                assert not bits_equal(cols[i], cols[j]), (lanes[lane0 + i], lanes[lane0 + j])
    alphas = sorted({a for _f, a, _p in lanes})
    if len(alphas) == 2:
        for f in sorted({f for f, _a, _p in lanes}):
            assert (f, alphas[0], BC.PENS[0]) in lanes and (f, alphas[1], BC.PENS[0]) in lanes
            assert not bits_equal(_ref(case, alphas[0], BC.PENS[0])[0][:, f], _ref(case, alphas[1], BC.PENS[0])[0][:, f])


# ---- (a) single alpha: CT x NL ----
@pytest.mark.parametrize("width", range(1, 9))
@pytest.mark.parametrize("itype", sorted(ITYPES))
def test_single_alpha_builds_vs_oracle(eng, monkeypatch, itype, width):
    """kp_dp_kernel<CT, NL, *, false> for both count widths and NL = 1..8: three fold groups
    of NL penalties, one full workgroup each."""
    case = _table(GP, ITYPES[itype])
    groups = BC.single_groups(width, _beta_of(case))
    cut = [(q * width, width, 0) for q in range(BC.NF)]
    _check_reference_tells_lanes_apart(case, groups, cut)
    scores, rt, re, _ = _run(eng, monkeypatch, case, groups, width, cut)
    _check_vs_oracle(case, groups, scores, rt, re)


# ---- (b) mixed: CT x NL x js ----
MIXED = [(w, n1, n2) for w in range(2, 9) for n1, n2 in BC.mixed_splits(w)]


@pytest.mark.parametrize("width,n1,n2", MIXED, ids=[f"{w}-{n1}+{n2}" for w, n1, n2 in MIXED])
@pytest.mark.parametrize("itype", sorted(ITYPES))
def test_mixed_builds_vs_oracle(eng, monkeypatch, itype, width, n1, n2):
    """kp_dp_kernel<CT, NL, *, true> for both count widths and NL = 2..8, the second (alpha,
    beta) set starting at lane 1 and at lane NL - 1: per fold n1 penalties of alpha 0.5 and n2
    of alpha 2.0, cut into one mixed workgroup; every lane against the oracle run with that
    lane's own alpha."""
    case = _table(GP, ITYPES[itype])
    groups = BC.mixed_groups(n1, n2, _beta_of(case))
    cut = [(q * width, width, n2) for q in range(BC.NF)]
    _check_reference_tells_lanes_apart(case, groups, cut)
    scores, rt, re, _ = _run(eng, monkeypatch, case, groups, width, cut)
    _check_vs_oracle(case, groups, scores, rt, re)


# ---- (c) NaN encodings through a mixed group ----
@pytest.mark.parametrize("width,n1,n2", [(4, 2, 2), (5, 3, 2)], ids=["4-2+2", "5-3+2"])
@pytest.mark.parametrize("itype", sorted(ITYPES))
def test_mixed_builds_nan_cells_vs_oracle(eng, monkeypatch, itype, width, n1, n2):
    """alpha 0 beside alpha 0.5 in one workgroup, with 10 % of the k-mers empty: the alpha 0
    lanes hold p = 0/0 cells, the alpha 0.5 lanes none; every cell, NaNs included."""
    case = _table(GP, ITYPES[itype], empty=True)
    groups = BC.mixed_groups(n1, n2, _beta_of(case), alphas=(0.0, 0.5))
    cut = [(q * width, width, n2) for q in range(BC.NF)]
    for f, alpha, pen in _lanes(groups):
        col = _ref(case, alpha, pen)[0][:, f]
        assert bool(np.isnan(col).any()) == (alpha == 0.0), (f, alpha, pen)
    scores, rt, re, _ = _run(eng, monkeypatch, case, groups, width, cut)
    _check_vs_oracle(case, groups, scores, rt, re)
    for lane, (f, alpha, pen) in enumerate(_lanes(groups)):
        assert np.array_equal(np.isnan(scores[lane]), np.isnan(_ref(case, alpha, pen)[0][:, f]))


# ---- (d) KP_EXACT_LOGS=1 ----
@pytest.mark.parametrize("kind", ["mixed-4-1+3", "single-3"])
def test_exact_logs_builds_vs_oracle_and_default_path(eng, monkeypatch, kind):
    """64-bit counts with every cell's single term from the C library's logs: a mixed 4-lane
    workgroup (1 + 3) and a single-alpha 3-lane one equal the oracle and the default path."""
    case = _table(GP, np.uint64)
    if kind == "single-3":
        width, groups = 3, BC.single_groups(3, _beta_of(case))
        cut = [(q * 3, 3, 0) for q in range(BC.NF)]
    else:
        width, groups = 4, BC.mixed_groups(1, 3, _beta_of(case))
        cut = [(q * 4, 4, 3) for q in range(BC.NF)]
    fast = _run(eng, monkeypatch, case, groups, width, cut, exact=0)
    exact = _run(eng, monkeypatch, case, groups, width, cut, exact=1)
    _check_vs_oracle(case, groups, *exact[:3])
    _check_vs_oracle(case, groups, *fast[:3])
    for lane, (a, b) in enumerate(zip(exact[0], fast[0])):
        assert bits_equal(a, b), lane
    assert bits_equal(exact[1], fast[1]) and bits_equal(exact[2], fast[2])


# ---- (e) backtrack and kp_fit_leaves on mixed 64-bit fit lanes ----
def test_mixed_u64_fit_lanes_backtrack_vs_oracle(eng, monkeypatch):
    """All-data counts only, two groups of fold -1 (alpha 0.5 and 2.0, two penalties each) cut
    into one mixed 4-lane workgroup: each lane's root score, leaf count and partition (names
    and order, through kp_fit_leaves) equal oracle.fit's with that lane's alpha."""
    from kmerpapa_amd.pattern_utils import PatternEnumeration, generality
    from oracle import oracle as O
    case = _table(GP, np.uint64)
    contexts = list(case["ctx"])
    M = np.array([case["ctx"][k][0] for k in contexts], np.uint64)
    U = np.array([case["ctx"][k][1] for k in contexts], np.uint64)
    Mk, Uk = eng.counts_in_kmer_order(GP, contexts, M, U, generality(GP), np.uint64)
    nm, nu = int(M.sum()), int(U.sum())
    assert nm + nu > 2 ** 32
    my = nm / (nm + nu)
    beta = {a: (a * (1.0 - my)) / my for a in (BC.ALPHA1, BC.ALPHA2)}
    groups = BC.mixed_groups(2, 2, lambda a, f: beta[a], folds=[-1])
    if eng.shard_width(GP, np.uint64) != 4:
        monkeypatch.setenv("KP_LANES_PER_WG", "4")
    assert eng.shard_width(GP, np.uint64) == 4
    assert eng.device_groups(groups, 4) == [(0, 4, 2)]
    plan = eng.Plan(eng.get_device(0), GP, 0)
    try:
        plan.set_counts(Mk, Uk)
        assert plan.info["lanes_per_workgroup"] == 4 and plan.nf == 1
        rt, _re, nlv = plan.run(groups)
        assert plan.stats()["dp_launches"] == plan.info["high_levels"] == 7
        PE = PatternEnumeration(GP)
        cols = []
        for lane, (_f, alpha, pen) in enumerate(_lanes(groups)):
            score, _rm, _ru, names, arr = O.fit(GP, contexts, M, U, alpha, beta[alpha], pen, 64)
            assert bits_equal(rt[lane], np.float32(score)), (lane, alpha, pen)
            assert int(nlv[lane]) == len(names), (lane, alpha, pen)
            assert [PE.num2pattern(int(x)) for x in plan.leaves(lane)] == names, (lane, alpha, pen)
            # (more than the roots: at these counts the two alphas' root scores agree in float32)
            assert bits_equal(plan.dump_lane(lane)[0], arr["score"]), (lane, alpha, pen)
            cols.append(arr["score"])
        # (reference only: the four lanes' arrays differ pairwise, so a lane that took another
        # lane's alpha or penalty cannot pass)
        for i in range(4):
            for j in range(i + 1, 4):
                assert not bits_equal(cols[i], cols[j]), (i, j)
    finally:
        plan.close()


# ---- (f) the product path: whole-genome-sized counts, two alphas, the 5-penalty grid ----
def test_product_path_u64_grid_vs_oracle(eng, monkeypatch):
    """Counts above 2^32 - 1 through the drop-in CV driver on NNNMN (4 lanes per workgroup with
    nothing set): every fold's 10 lanes run as [4] [1 + 3 mixed] [2], so the 64-bit mixed 4-lane
    build runs.  Every (alpha, penalty, fold) train and test root equals the oracle's, and the
    best point is the one a plain selection over the oracle's roots gives."""
    from kmerpapa_amd.algorithms import bottum_up_array_penalty_plus_pseudo_CV as cvm
    from kmerpapa_amd.shard import fold_order
    gp, seed = "NNNMN", 3
    monkeypatch.delenv("KP_LANES_PER_WG", raising=False)
    assert eng.shard_width(gp, np.uint64) == 4
    case = _table(gp, np.uint64)  # (its fold split: fold_tables with RandomState(3), as cv_roots(seed=3) draws it)
    ctx = case["ctx"]
    nmut, nunmut = sum(v[0] for v in ctx.values()), sum(v[1] for v in ctx.values())
    itype = cvm._itype(nmut, nunmut)
    assert itype == np.uint64
    alphas, pens = BC.GRID_ALPHAS, BC.GRID_PENS
    # the passes: a fold's 10 lanes are cut into [4] [1 + 3 mixed] [2] ...
    groups = BC.grid_groups(_beta_of(case), fold_order(BC.NF))
    for pas in eng.plan_passes(groups, 10, width=4)[0]:
        assert eng.device_groups(pas, 4) == [(0, 4, 0), (4, 4, 3), (8, 2, 0)]
    # ... and run_groups packs each piece into a pass of its own (engine.pass_cap)
    want_passes = eng.plan_passes(groups, eng.pass_cap(groups, 1000, 4), 4)[0]
    want_cuts = [eng.device_groups(pas, 4) for pas in want_passes]
    assert sorted(want_cuts) == sorted([[(0, 4, 0)], [(0, 4, 3)], [(0, 2, 0)]] * BC.NF)
    log = []
    monkeypatch.setattr(eng, "PASS_LOG", log)
    res = cvm.cv_roots(gp, ctx, alphas, pens, BC.NF, seed, 1, itype, devices=[0])
    plan = eng.get_plan(0, gp)
    assert plan.itype == np.uint64 and plan.info["lanes_per_workgroup"] == 4
    assert [rec[1] for rec in log] == [sum(len(g[3]) for g in pas) for pas in want_passes]
    assert all(rec[5]["dp_launches"] == plan.info["high_levels"] for rec in log)
    monkeypatch.setattr(eng, "PASS_LOG", None)
    for a_i, alpha in enumerate(alphas):
        assert np.array_equal(res["betas"][0, a_i], _betas(case, alpha))
        for p_i, pen in enumerate(pens):
            _score, root_train, root_test = _ref(case, alpha, pen)
            assert bits_equal(res["train"][0, a_i, p_i], root_train), (alpha, pen)
            assert bits_equal(res["test"][0, a_i, p_i], root_test), (alpha, pen)
    # the selection (CV :165-177): float64 sum over the folds, strict "<", alpha-major
    best, best_loss = (None, None), 1e100
    for alpha in alphas:
        for pen in pens:
            acc = 0.0
            for v in _ref(case, alpha, pen)[2]:
                acc += float(v)
            if acc < best_loss:
                best, best_loss = (alpha, pen), acc

    class A:
        nfolds = BC.NF
        iterations = 1
        verbosity = 0
        CVfile = None
    A.seed = seed
    monkeypatch.setenv("KMERPAPA_DEVICES", "0")
    got = cvm.pattern_partition_bottom_up(gp, ctx, alphas, A, nmut, nunmut, pens)
    assert (got[0], got[1]) == best and got[2] == best_loss
    eng.release_all()


def test_product_path_u64_passes_every_cell_vs_oracle(eng, monkeypatch):
    """The same grid's passes as engine.run_groups makes them (each fold's [4] [1 + 3 mixed] [2]
    pieces, a pass each), run on a plan of NNNMN with nothing set: every cell of every lane.
    (The roots the driver returns cannot tell the two alphas apart at these counts; the cells
    can.)"""
    from kmerpapa_amd.shard import fold_order
    gp = "NNNMN"
    monkeypatch.delenv("KP_LANES_PER_WG", raising=False)
    case = _table(gp, np.uint64)
    groups = BC.grid_groups(_beta_of(case), fold_order(BC.NF))
    passes = eng.plan_passes(groups, eng.pass_cap(groups, 1000, 4), 4)[0]
    for f in range(BC.NF):  # (reference only: the mixed piece's two alphas differ at its penalties)
        for pen in BC.GRID_PENS:
            assert not bits_equal(_ref(case, 0.5, pen)[0][:, f], _ref(case, 2.0, pen)[0][:, f]), (f, pen)
    plan = eng.Plan(eng.get_device(0), gp, 0)
    try:
        plan.set_counts(case["Mk"], case["Uk"])
        assert plan.info["lanes_per_workgroup"] == 4 and plan.info["block"] == 3375
        mixed = 0
        for pas in passes:
            cut = eng.device_groups(pas, 4)
            assert len(cut) == 1
            mixed += cut[0] == (0, 4, 3)
            rt, re, _ = plan.run(pas)
            assert plan.stats()["dp_launches"] == plan.info["high_levels"]
            _check_vs_oracle(case, pas, [plan.dump_lane(lane)[0] for lane in range(len(rt))], rt, re)
        assert mixed == BC.NF
    finally:
        plan.close()
