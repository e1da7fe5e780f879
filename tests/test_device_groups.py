"""How kp_pass cuts a pass's groups into workgroups (host code, kp_device_groups; no GPU):
full workgroups first for a group wider than one, and consecutive groups of the same fold
cut together into mixed workgroups (at most two alphas each) when that needs fewer
workgroups -- what engine.fold_pieces relies on for the 11-mer's 7-penalty grid."""
import pytest

from kmerpapa_amd import engine
from tests import build_cases


def _dg(sizes, folds=None, alphas=None, width=5):
    folds = folds or [0] * len(sizes)
    alphas = alphas or [float(i + 1) for i in range(len(sizes))]
    groups = [(f, a, 0.5 * a, [1.0 + j for j in range(n)]) for f, a, n in zip(folds, alphas, sizes)]
    return engine.device_groups(groups, width)


def test_wide_group_full_workgroups_first(monkeypatch):
    assert _dg([7]) == [(0, 5, 0), (5, 2, 0)]
    assert _dg([8], width=3) == [(0, 3, 0), (3, 3, 0), (6, 2, 0)]
    monkeypatch.setenv("KP_WIDE_SPLIT", "0")  # the near-equal split (A/B knob)
    assert _dg([7]) == [(0, 4, 0), (4, 3, 0)]


def test_same_fold_groups_become_mixed_workgroups():
    assert _dg([2, 3]) == [(0, 5, 3)]
    assert _dg([4, 1]) == [(0, 5, 1)]
    assert _dg([3, 4, 3]) == [(0, 5, 2), (5, 5, 3)]
    # a piece of the 11-mer grid: the last 2 penalties of one alpha, the first 3 of the next
    assert _dg([2, 3], alphas=[1.0, 2.0]) == [(0, 5, 3)]


def test_no_mixing_when_it_saves_nothing_or_needs_three_alphas():
    assert _dg([5, 2]) == [(0, 5, 0), (5, 2, 0)]          # 2 workgroups either way
    assert _dg([4, 2]) == [(0, 4, 0), (4, 2, 0)]
    assert _dg([2, 2, 1]) == [(0, 2, 0), (2, 2, 0), (4, 1, 0)]  # one workgroup would hold 3 alphas
    assert _dg([2, 3], folds=[0, 1]) == [(0, 2, 0), (2, 3, 0)]  # different folds never mix


def test_same_alpha_pieces_join_without_a_second_set():
    # two pieces of ONE (alpha, fold) group (e.g. a split group's lanes) join unmixed
    assert _dg([2, 3], alphas=[1.0, 1.0]) == [(0, 5, 0)]


def test_fold_pieces_run_as_one_workgroup_each():
    """Every 5-lane piece engine.plan_passes cuts from the 11-mer grid is one workgroup."""
    alphas, pens = [0.5, 1.0, 2.0, 3.0, 5.0, 7.0, 10.0], [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    groups = [(f, a, 0.01 * a, list(pens)) for a in alphas for f in range(2)]
    passes, _ = engine.plan_passes(groups, 7, 5)
    mixed = 0
    for p in passes:
        dg = engine.device_groups(p, 5)
        assert len(dg) == 1 and dg[0][1] == sum(len(g[3]) for g in p)
        mixed += dg[0][2] > 0
    assert mixed == 10


# ---- the cuts tests/test_gpu_builds.py relies on to name the build each of its cases runs ----

def _beta(alpha, fold):
    return 100.0 * alpha + fold  # (a placeholder: only equal / unequal matters to the cut)


@pytest.mark.parametrize("width", range(1, 9))
def test_build_matrix_single_alpha_cut(width):
    """Three fold groups of ``width`` penalties: one unmixed workgroup of that width each."""
    groups = build_cases.single_groups(width, _beta)
    assert engine.device_groups(groups, width) == [(q * width, width, 0) for q in range(build_cases.NF)]


@pytest.mark.parametrize("width", range(2, 9))
def test_build_matrix_mixed_cut(width):
    """Per fold n1 lanes of one alpha and n2 of the next, n1 + n2 = width: one mixed workgroup
    per fold whose last n2 lanes take the second set, for js = n1 at both ends of its range."""
    splits = build_cases.mixed_splits(width)
    assert splits == ([(1, 1)] if width == 2 else [(1, width - 1), (width - 1, 1)])
    for n1, n2 in splits:
        groups = build_cases.mixed_groups(n1, n2, _beta)
        assert engine.device_groups(groups, width) == [(q * width, width, n2) for q in range(build_cases.NF)]
        # at a workgroup one lane narrower (a silent width fallback) nothing is mixed
        assert all(m == 0 for _, _, m in engine.device_groups(groups, width - 1))


def test_grid_fold_pass_width4_cut():
    """The default product path of whole-genome counts (64-bit: 4 lanes per workgroup) on the
    usual 2 alpha x 5 penalty grid: a fold's 10 lanes, as engine.plan_passes lays them out, are
    cut into [4] [1 + 3 mixed] [2]; and the passes run_groups itself makes (engine.pass_cap: 5
    lanes) are those three pieces, one workgroup each."""
    from kmerpapa_amd.shard import fold_order
    groups = build_cases.grid_groups(_beta, fold_order(build_cases.NF))
    passes, order = engine.plan_passes(groups, 10, 4)
    assert sorted(order) == list(range(30))
    assert len(passes) == build_cases.NF
    for f, pas in enumerate(passes):
        assert {g[0] for g in pas} == {f}
        assert engine.device_groups(pas, 4) == [(0, 4, 0), (4, 4, 3), (8, 2, 0)]
    passes, order = engine.plan_passes(groups, engine.pass_cap(groups, 1000, 4), 4)
    assert sorted(order) == list(range(30))
    assert [len({g[0] for g in pas}) for pas in passes] == [1] * (3 * build_cases.NF)
    assert sorted(engine.device_groups(pas, 4) for pas in passes) == sorted([[(0, 4, 0)], [(0, 4, 3)], [(0, 2, 0)]]
                                                                            * build_cases.NF)


def test_build_matrix_lattices_keep_their_widths(monkeypatch):
    """NNMNN (the matrix's lattice) holds every workgroup width asked for, 1 to 8, at both
    count widths; NNNMN's larger tables cap it at 5 (32-bit) and 4 (64-bit: the product-path
    case's width, with nothing set)."""
    import numpy as np
    assert engine.shard_width("NNNMN", np.uint64) == 4
    for w in range(1, 9):
        monkeypatch.setenv("KP_LANES_PER_WG", str(w))
        assert engine.shard_width("NNMNN", np.uint32) == w
        assert engine.shard_width("NNMNN", np.uint64) == w
        assert engine.shard_width("NNNMN", np.uint32) == min(w, 5)
        assert engine.shard_width("NNNMN", np.uint64) == min(w, 4)


def test_fit_fold_groups_mix_like_any_other_fold():
    """Two groups of fold -1 (all data: the fit) are cut together like any other fold's."""
    groups = build_cases.mixed_groups(2, 2, _beta, folds=[-1])
    assert engine.device_groups(groups, 4) == [(0, 4, 2)]
    assert engine.device_groups(groups, 5) == [(0, 4, 2)]
    assert engine.device_groups(groups, 3) == [(0, 2, 0), (2, 2, 0)]  # 2 workgroups either way
    # fold -1 beside fold 0: different folds, never mixed
    two = build_cases.mixed_groups(2, 2, _beta, folds=[-1])[:1] + build_cases.mixed_groups(2, 2, _beta, folds=[0])[1:]
    assert engine.device_groups(two, 4) == [(0, 2, 0), (2, 2, 0)]


def test_bad_arguments():
    with pytest.raises(engine.KPError):
        engine.device_groups([(0, 1.0, 1.0, [1.0])], 0)
