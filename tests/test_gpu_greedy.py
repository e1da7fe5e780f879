"""The greedy top-down partition on the GPU (kp_greedy) against the host run of the same
per-node code (kp_greedy_host), the plain-Python restatement (tests/greedy_ref.py) and the
reference's recorded values (tests/golden/greedy*.json).  Bar: loss and chain sums bit for
bit, identical partitions (names and order) and leaf counts, CLI text byte-identical."""
import numpy as np
import pytest

from tests import greedy_cases as C
from tests import greedy_ref as R
from tests.fixtures import context_table, golden_json, write_count_files

pytestmark = pytest.mark.gpu

FIT = golden_json("greedy_fit.json")
GRID = golden_json("greedy_grid.json")
CLI = golden_json("greedy_cli.json")


@pytest.fixture(scope="module")
def dev():
    from kmerpapa_amd import engine
    engine.load()
    assert engine.device_count() >= 1, "no GPU visible to the HIP runtime"
    return engine.get_device(engine.visible_devices()[0])


def _gpu(dev, gp, M, U, lanes, nf):
    loss, chain, nl = dev.greedy(gp, M, U, list(lanes), nf)
    return C.observed(gp, loss, chain, nl, [dev.greedy_leaves(i) for i in range(len(lanes))])


def _host(gp, M, U, lanes, nf):
    from kmerpapa_amd import engine
    loss, chain, nl, leaves = engine.greedy_host(gp, M, U, list(lanes), nf)
    return C.observed(gp, loss, chain, nl, leaves)


@pytest.mark.parametrize("part", range(4))
def test_random_cases_equal_host_and_ref(dev, part, monkeypatch):
    """The 200 seeded cases of the CPU suite (50 per part) with 64 k-mers per histogram chunk,
    so that nodes of more than 64 k-mers are merged from several waves' partial histograms:
    every case against kp_greedy_host, every fourth also against greedy_ref."""
    monkeypatch.setenv("KP_GREEDY_CHUNK", "64")
    for i, (gp, nf, M, U, lanes) in enumerate(C.cases()):
        if i % 4 != part:
            continue
        got = _gpu(dev, gp, M, U, lanes, nf)
        assert got == _host(gp, M, U, lanes, nf), (i, gp, nf, lanes)
        if (i // 4) % 4 == 0:
            assert got == C.expected(gp, nf, M, U, lanes, i), (i, gp, nf, lanes)


def _table4096(nf):
    rng = np.random.RandomState(77)
    bg = rng.randint(1, 30000, size=(4096, nf))
    M = rng.binomial(bg, rng.uniform(0.001, 0.05, size=(4096, 1))).astype(np.uint64)
    return M, bg.astype(np.uint64)


def _lanes40(M, U, nf):
    """Fit lanes and CV lanes mixed: lane i on fold i % (nf + 1) - 1, 8 chains."""
    lanes = []
    pens = [0.0, 2.0, 5.0, 9.0, 1e9]
    for i in range(40):
        fold = i % (nf + 1) - 1
        alpha = [0.5, 2.0, 10.0][i % 3]
        trM, trU = int(M.sum()), int(U.sum())
        if fold >= 0:
            trM -= int(M[:, fold].sum())
            trU -= int(U[:, fold].sum())
        lanes.append((fold, i % 8 if fold >= 0 else -1, alpha, R.get_betas(alpha, trM, trU), pens[i % 5]))
    return lanes


def test_40_lanes_in_several_batches_and_many_chunks(dev, monkeypatch):
    """40 mixed lanes on a 4,096-k-mer table, chunk 64 (the root spans 64 chunks), under a
    memory budget of 8 MiB that holds about ten lanes' trees at a time; the same call with
    the device's own budget runs as one batch and gives the same bits."""
    gp, nf = "NNNNNN", 3
    M, U = _table4096(nf)
    lanes = _lanes40(M, U, nf)
    want = _host(gp, M, U, lanes, nf)
    monkeypatch.setenv("KP_GREEDY_CHUNK", "64")
    monkeypatch.setenv("KP_GREEDY_MEM", str(8 << 20))
    assert _gpu(dev, gp, M, U, lanes, nf) == want
    assert dev.greedy_batches() > 1
    monkeypatch.delenv("KP_GREEDY_MEM")
    assert _gpu(dev, gp, M, U, lanes, nf) == want
    assert dev.greedy_batches() == 1
    assert max(want[2]) > 2048 and min(want[2]) == 1  # c = 0 and c = 1e9 lanes are among them


def test_one_lane(dev, monkeypatch):
    """A single CV lane with a chain, chunk 64 and the default chunk: host, ref and GPU agree."""
    gp, nf = "NNNNNN", 3
    M, U = _table4096(nf)
    lanes = [_lanes40(M, U, nf)[2]]
    want = C.expected(gp, nf, M, U, tuple(lanes), "one_lane")
    assert _host(gp, M, U, lanes, nf) == want
    assert _gpu(dev, gp, M, U, lanes, nf) == want
    monkeypatch.setenv("KP_GREEDY_CHUNK", "64")
    assert _gpu(dev, gp, M, U, lanes, nf) == want


def test_budget_too_small_is_nomem(dev, monkeypatch):
    from kmerpapa_amd import engine
    M, U = _table4096(3)
    monkeypatch.setenv("KP_GREEDY_MEM", str(1 << 19))
    with pytest.raises(engine.KPError) as e:
        dev.greedy("NNNNNN", M, U, _lanes40(M, U, 3)[:2], 3)
    assert e.value.code == -2 and "do not fit" in str(e.value)


@pytest.mark.parametrize("k", [5, 7])
def test_golden_fits(dev, k):
    """greedy_partition of the drop-in module: loss bit for bit, names, totals.  The 7-mer
    fit at c = 0 (NNNMNNN, 8,192 k-mers, 5,382 leaves) is the mid-size case at the default chunk."""
    from kmerpapa_amd.algorithms import greedy_penalty_plus_pseudo as gm
    ctx, gp, n_mut, n_unmut = context_table(k)
    assert FIT[str(k)]["gen_pat"] == gp
    for fit in FIT[str(k)]["fits"]:
        loss, M, U, names = gm.greedy_partition(gp, ctx, fit["alpha"], None, fit["penalty"], None)
        assert C.bits(loss) == C.bits(float.fromhex(fit["loss_hex"])), (fit["alpha"], fit["penalty"])
        assert names == fit["names"]
        assert (int(M), int(U)) == (fit["M"], fit["U"]) == (n_mut, n_unmut)


@pytest.mark.parametrize("run", range(4))
def test_golden_grid(dev, run):
    from kmerpapa_amd.algorithms import greedy_penalty_plus_pseudo as gm
    rec = GRID["runs"][run]
    ctx, gp, _, _ = context_table(5)
    alphas, pens = GRID["alphas"], GRID["penalties"]
    cv = gm.GridSearchCV(gp, ctx, pens, alphas, rec["nfolds"], rec["nit"], rec["seed"])
    got = [[C.bits(cv.loglik(a, c)) for c in pens] for a in alphas]
    assert got == [[C.bits(float.fromhex(x)) for x in row] for row in rec["loglik_hex"]]
    best = cv.get_best_a_c()
    assert [best[0], best[1], C.bits(best[2])] == rec["best"][:2] + [C.bits(float.fromhex(rec["best"][2]))]
    # a point outside the grid runs as a job of its own
    one = gm.CrossValidation(gp, ctx, rec["nfolds"], rec["nit"], rec["seed"])
    assert C.bits(one.loglik(alphas[1], pens[0])) == got[1][0]


@pytest.mark.parametrize("run", ["greedy", "greedyCV", "greedy_smaller_k"])
def test_cli_text(dev, run, tmp_path, capsys):
    """--greedy, --greedyCV and --greedy --test_smaller_k through the CLI: stdout table and
    stderr byte-identical to the reference's."""
    from kmerpapa_amd import cli
    g = CLI[run]
    pos, bg = write_count_files(5, str(tmp_path))
    argv = [pos if a.endswith("mutated_5mers.txt") else bg if a.endswith("background_5mers.txt") else a
            for a in g["argv"]]
    out = tmp_path / "o.txt"
    capsys.readouterr()
    rc = cli.main(argv + ["-o", str(out)])
    assert rc == g["rc"]
    assert out.read_text() == g["output"]
    assert capsys.readouterr().err == g["stderr"]


def test_all_kmers_with_greedy_is_the_references_assertion(dev, tmp_path):
    from kmerpapa_amd import cli
    pos, bg = write_count_files(5, str(tmp_path))
    with pytest.raises(AssertionError, match="greedy option cannot be used"):
        cli.main(["-p", pos, "-b", bg, "--greedy", "--score", "all_kmers", "-a", "0.5", "2", "--nfolds", "2",
                  "-o", str(tmp_path / "o.txt")])
