"""The greedy top-down partition without a GPU: the plain-Python restatement
(tests/greedy_ref.py) and the host run of the kernels' per-node code (kp_greedy_host) against
the reference's recorded values (tests/golden/greedy*.json, make_golden_greedy.py) and
against each other on seeded random cases."""
import numpy as np
import pytest

from kmerpapa_amd import engine
from kmerpapa_amd.CV_tools import make_all_folds
from tests import greedy_cases as C
from tests import greedy_ref as R
from tests.fixtures import context_table, golden_json, golden_npz

FIT = golden_json("greedy_fit.json")
GRID = golden_json("greedy_grid.json")


def _gm():
    from kmerpapa_amd.algorithms import greedy_penalty_plus_pseudo
    return greedy_penalty_plus_pseudo


_tables = {}


def _table(k):
    if k not in _tables:
        ctx, gp, n_mut, n_unmut = context_table(k)
        _tables[k] = (gp, _gm().kmer_table_of(gp, ctx), n_mut, n_unmut)
    return _tables[k]


def _host_run(gp, M, U, lanes, nf=0):
    return engine.greedy_host(gp, M, U, lanes, nf)[:3]


@pytest.mark.parametrize("k", [5, 7])
def test_golden_fits(k):
    """greedy_partition's loss (bit for bit), names and totals: greedy_ref and kp_greedy_host."""
    gp, table, n_mut, n_unmut = _table(k)
    rec = FIT[str(k)]
    assert rec["gen_pat"] == gp
    for fit in rec["fits"]:
        want = (C.bits(float.fromhex(fit["loss_hex"])), fit["names"])
        loss, Mt, Ut, names = R.fit(gp, table[:, 0], table[:, 1], fit["alpha"], fit["penalty"])
        assert (Mt, Ut) == (fit["M"], fit["U"]) == (n_mut, n_unmut)
        assert (C.bits(loss), names) == want, f"greedy_ref differs at {fit['alpha']}, {fit['penalty']}"
        beta = R.get_betas(fit["alpha"], Mt, Ut)
        hl, _, nl, leaves = engine.greedy_host(gp, table[:, 0], table[:, 1],
                                               [(-1, -1, fit["alpha"], beta, fit["penalty"])])
        got = [engine.word_pattern(w, len(gp)) for w in leaves[0]]
        assert (C.bits(hl[0]), got) == want, f"kp_greedy_host differs at {fit['alpha']}, {fit['penalty']}"
        assert int(nl[0]) == len(fit["names"])
    assert rec["fits"][1]["penalty"] == 0.0 and len(rec["fits"][1]["names"]) > len(rec["fits"][0]["names"])
    assert rec["fits"][2]["names"] == [gp]  # c = 1e9: the root stays whole


@pytest.mark.parametrize("run", range(4))
def test_golden_grid(run):
    """GridSearchCV's loglik values and best point: greedy_ref over make_all_folds' tables,
    and the drop-in module with kp_greedy_host in place of the GPU call."""
    rec = GRID["runs"][run]
    gp, table, _, _ = _table(5)
    alphas, pens = GRID["alphas"], GRID["penalties"]
    want = [[C.bits(float.fromhex(x)) for x in row] for row in rec["loglik_hex"]]
    folds = make_all_folds(table, rec["nfolds"], rec["nit"], np.random.RandomState(rec["seed"]))
    ref = [[C.bits(R.loglik(gp, table, folds, a, c)) for c in pens] for a in alphas]
    assert ref == want
    ctx = context_table(5)[0]
    cv = _gm().GridSearchCV(gp, ctx, pens, alphas, rec["nfolds"], rec["nit"], rec["seed"])
    points = [(a, c) for a in alphas for c in pens]
    cv._grid = dict(zip(points, cv.logliks(points, run=_host_run)))
    assert [[C.bits(cv.loglik(a, c)) for c in pens] for a in alphas] == want
    best = cv.get_best_a_c()
    assert [best[0], best[1], C.bits(best[2])] == rec["best"][:2] + [C.bits(float.fromhex(rec["best"][2]))]


def test_host_equals_ref_on_random_cases():
    """kp_greedy_host against greedy_ref: loss bits, partition and its order, leaf counts and
    chain sums on 200 seeded cases (N / two- / three-letter mixes of 2-6 positions, all-zero
    and uniform tables, totals past 2^32, alpha = 0 with empty k-mers, c = 0 and c = 1e9)."""
    kinds = set()
    for i, (gp, nf, M, U, lanes) in enumerate(C.cases()):
        loss, chain, nl, leaves = engine.greedy_host(gp, M, U, list(lanes), nf)
        assert C.observed(gp, loss, chain, nl, leaves) == C.expected(gp, nf, M, U, lanes, i), (i, gp, nf, lanes)
        kinds.add((int(M.sum()) == 0, int(M.sum() + U.sum()) > 1 << 32))
    assert len(C.cases()) == 200 and kinds == {(True, False), (False, False), (False, True)}


def test_uniform_table_first_candidate_wins():
    """Every k-mer alike: the four 1 + 3 splits of N (A|B, C|D, G|H, T|V) have one value at
    every position, below the 2 + 2 splits'; the scan keeps the first of those twelve equal
    candidates, A|B at position 0, and likewise further down."""
    gp = "NNN"
    M = np.full(64, 3, np.uint64)
    U = np.full(64, 100, np.uint64)
    beta = R.get_betas(1.0, 192, 6400)
    _, _, _, leaves = engine.greedy_host(gp, M, U, [(-1, -1, 1.0, beta, 0.0)])
    names = [engine.word_pattern(w, 3) for w in leaves[0]]
    assert names == R.lane(gp, M, U, -1, 1.0, beta, 0.0)[1] == ["AAA", "AAB", "ABN", "BNN"]


def test_argument_errors():
    one = np.ones(4, np.uint64)
    lane = [(-1, -1, 1.0, 1.0, 1.0)]
    with pytest.raises(engine.KPError) as e:
        engine.greedy_host("N" * 17, one, one, lane)
    assert e.value.code == -1 and "16 positions" in str(e.value)
    with pytest.raises(engine.KPError) as e:
        engine.greedy_host("N", one * np.uint64(1 << 52), one, lane)
    assert e.value.code == -1 and "2^53" in str(e.value)
    with pytest.raises(engine.KPError):
        engine.greedy_host("NN", one, one, lane)  # 4 rows for 16 k-mers
    with pytest.raises(engine.KPError):
        engine.greedy_host("N", one, one, [(0, -1, 1.0, 1.0, 1.0)])  # a fold lane without fold tables


def test_pattern_words_round_trip():
    for pat in ["ACGT", "NMRWSYKVHDB", "N" * 16]:
        assert engine.word_pattern(engine.pattern_word(pat), len(pat)) == pat
    assert engine.pattern_word("AC") == 1 | 2 << 4


def test_interleaved_fold_split_is_make_all_folds():
    """The greedy CV's colours are the [n, 2] table flattened (M, U interleaved, matches
    order), redrawn per repeat: the module's tables are the reference's make_all_folds
    (pinned in folds.npz) and each fold is one native kp_fold_sample of those colours."""
    kt = np.array([[1, 100, 200], [10, 1000, 2000]])
    want = golden_npz("folds.npz")["make_all_folds"]
    assert np.array_equal(make_all_folds(kt, 10, 2, np.random.RandomState(0)), want)
    gp, table, _, _ = _table(5)
    ctx = context_table(5)[0]
    cv = _gm().CrossValidation(gp, ctx, nfolds=3, nit=2, seed=1)
    prng = np.random.RandomState(1)
    for rep in range(2):
        col = table.reshape(-1).copy()
        per = int(col.sum()) // 3
        for f in range(2):
            s = engine.fold_sample(col, per, prng)
            assert np.array_equal(cv.fold_kmer_table[rep, f], s.reshape(table.shape))
            col -= s
        assert np.array_equal(cv.fold_kmer_table[rep, 2], col.reshape(table.shape))
    assert cv.fold_kmer_table.sum(axis=1).tolist() == [table.tolist()] * 2


def test_module_has_the_reference_names():
    gm = _gm()
    for name in ("train_loss", "test_logLik", "greedy_partition", "CrossValidation", "GridSearchCV"):
        assert hasattr(gm, name)
    assert hasattr(gm.CrossValidation, "loglik") and hasattr(gm.GridSearchCV, "get_best_a_c")
    assert C.bits(gm.train_loss(3.0, 100.0, 0.5, 7.0, 2.0)) == C.bits(R.train_loss(3, 100, 0.5, 7.0, 2.0))
    assert C.bits(gm.test_logLik(3.0, 100.0, 1.0, 9.0, 0.5, 7.0)) == C.bits(R.test_loglik(3, 100, 1, 9, 0.5, 7.0))


def test_cli_still_rejects_greedy_without_input_and_bayesopt(tmp_path, capsys):
    from kmerpapa_amd import cli
    assert cli.main(["--greedyCV"]) == 2
    pos = tmp_path / "p.txt"
    pos.write_text("AAA 1\n")
    assert cli.main(["-p", str(pos), "-b", str(pos), "--BayesOpt"]) == 2
    assert "not part of this MI355X build" in capsys.readouterr().err
