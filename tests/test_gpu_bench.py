"""bench.py as a command on the GPU: a run without --full times exactly --steps steps and
skips the legs beside the headline figure, and --dump-outputs writes what the last timed
step computed -- checked bit for bit against the CPU oracle on a 5-mer lattice (151,875
cells: the oracle takes milliseconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.fixtures import bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GP = "NNMNN"


def test_plain_run_dumps_last_step(tmp_path):
    import bench
    from oracle import oracle as O
    out = tmp_path / "dump"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--pattern", GP, "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 1  # the JSON line is stdout's only content
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "cell-scores/s" and line["higher_is_better"] is True
    units = 2 * line["config"]["units_per_step"]
    assert abs(line["value"] * line["ms_per_step"] * 2 / 1e3 - units) <= 1e-9 * units
    assert line["cv_full_grid"] is None and line["cpu_baseline"] is None and "scaling_by_gpus" not in line

    d = {n: np.load(out / f"{n}.npy") for n in ("root_train", "root_test", "n_leaves", "cell_index", "cell_scores",
                                                 "lane_params")}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in d)
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    lanes = line["config"]["lanes_per_step"]
    assert d["root_train"].shape == d["root_test"].shape == d["n_leaves"].shape == (lanes,)
    assert d["cell_scores"].shape == (lanes, bench.DUMP_CELLS) and d["lane_params"].shape == (lanes, 4)
    cells = d["cell_index"].astype(np.int64)
    assert cells.min() >= 0 and cells.max() < O.npat(GP)

    prep = bench.prepare(GP)
    beta = {(g[1], g[0]): g[2] for g in prep["groups"]}
    for lane, (fold, alpha, b, c) in enumerate(d["lane_params"]):
        fold = int(fold)
        assert beta[(alpha, fold)] == b
        ref = O.cv_pass(GP, prep["contexts"], prep["Mf"], prep["Uf"], alpha,
                        [beta[(alpha, f)] for f in range(prep["nfolds"])], c, 32)
        assert bits_equal(d["root_train"][lane], ref["root_train"][fold])
        assert bits_equal(d["root_test"][lane], ref["root_test"][fold])
        assert bits_equal(d["cell_scores"][lane], ref["score"][cells, fold])
        assert d["n_leaves"][lane] >= 1
