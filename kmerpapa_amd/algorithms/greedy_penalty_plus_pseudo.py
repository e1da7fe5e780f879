"""The greedy top-down heuristic -- drop-in for the reference's
``kmerpapa.algorithms.greedy_penalty_plus_pseudo`` (v0.2.4; ``--greedy`` / ``--greedyCV``).

There is no lattice here: a pattern is split at the (position, pair) whose two halves have
the smallest summed loss, as long as that beats the pattern's own loss, and the halves are
split again (greedy_res_kmer_table_ord, ref :159-196).  Only the k-mer count table and one
tree per (alpha, penalty, fold) are needed, so this is the path for general patterns whose
lattice does not fit a GPU.  The trees of the whole grid and all folds of one repeat grow
together on the first visible GPU (``kp_greedy``, csrc/kp_greedy.h) in float64 with the C
library's log, in the reference's operation and scan order: losses, partitions and test
log-likelihoods are bit-identical to the reference's.  There is no CPU path.

The fold split is the reference's ``CV_tools.make_all_folds`` over the ``[n, 2]`` table
flattened (M and U interleaved, ``matches`` order), drawn by the native sampler.
``BaysianOptimizationCV`` is not provided: ``gp_minimize`` is unseeded in the reference.
"""
import math

import numpy as np

from .. import engine
from ..CV_tools import make_all_folds
from ..pattern_utils import generality, matches
from ..score_utils import get_betas


def train_loss(trainM, trainU, alphas, betas, penalty):
    """Loss of one pattern (ref :18-25; host helper kept for the reference's API -- the
    partition evaluates it on the GPU)."""
    p = (trainM + alphas) / (trainM + trainU + alphas + betas)
    s = penalty
    if trainM > 0:
        s += -2.0 * trainM * math.log(p)
    if trainU > 0:
        s += -2.0 * trainU * math.log(1 - p)
    return s


def test_logLik(trainM, trainU, testM, testU, alphas, betas):
    """-2 log-likelihood of test counts under the training rate (ref :28-35; host helper)."""
    p = (trainM + alphas) / (trainM + trainU + alphas + betas)
    s = 0.0
    if testM > 0:
        s += -2.0 * testM * math.log(p)
    if testU > 0:
        s += -2.0 * testU * math.log(1 - p)
    return s


def kmer_table_of(genpat, contextD):
    """``[n_kmers, 2]`` uint64 (M, U) rows in ``matches(genpat)`` order (ref :282-287) from a
    dict or an io_utils.KmerCounts table (which must hold every k-mer of ``genpat``)."""
    npat = generality(genpat)
    table = np.zeros((npat, 2), dtype=np.uint64)
    if hasattr(contextD, "letters"):
        if len(contextD) != npat:
            raise KeyError("the count table must hold every k-mer of the general pattern (zero-filled)")
        idx = engine.kmer_order(genpat, contextD)
        table[idx, 0] = contextD.M
        table[idx, 1] = contextD.U
    else:
        for i, context in enumerate(matches(genpat)):
            n_mut, n_unmut = contextD[context]
            table[i, 0] = n_mut
            table[i, 1] = n_unmut
    return table


def _device():
    devices = engine.visible_devices()  # no CPU path: raises without the library / a GPU
    if not devices:
        raise engine.KPError(-3, "the greedy partition runs on the GPU: no GPU is visible to the HIP runtime "
                                 f"({engine.LIB_PATH})")
    return engine.get_device(devices[0])


def greedy_partition(genpat, contextD, alpha, beta, penalty, args):
    """Greedy partition of all data (ref :279-293).  ``beta`` is ignored as in the reference:
    it is recomputed from the table totals.  Returns ``(loss, M_total, U_total, names)``."""
    table = kmer_table_of(genpat, contextD)
    MU = table.sum(axis=0)
    beta = get_betas(alpha, MU[0], MU[1])
    dev = _device()
    loss, _, _ = dev.greedy(genpat, table[:, 0], table[:, 1], [(-1, -1, alpha, beta, penalty)])
    k = len(genpat)
    papa = [engine.word_pattern(w, k) for w in dev.greedy_leaves(0)]
    return float(loss[0]), MU[0], MU[1], papa


class CrossValidation:
    """Repeated k-fold cross-validation of the greedy partition (ref :296-336)."""

    def __init__(self, genpat, contextD, nfolds=2, nit=1, seed=None, verbosity=1):
        self.nfolds = nfolds
        self.nit = nit
        self.seed = seed
        self.genpat = genpat
        self.npat = generality(genpat)
        self.kmer_table = kmer_table_of(genpat, contextD)
        prng = np.random.RandomState(seed)
        self.fold_kmer_table = make_all_folds(self.kmer_table, nfolds, nit, prng)
        self.genpat_ord = np.array([ord(x) for x in self.genpat])

    def logliks(self, points, run=None):
        """:meth:`loglik` of every ``(alpha, penalty)`` of ``points``: per repeat one GPU job
        whose lanes are points x folds; a point's folds form one chain, so its test terms
        are added fold by fold, leaf by leaf from 0.0 as the reference's ``test_ll`` (:325-333).
        ``run(genpat, M, U, lanes, nf)`` replaces the GPU call (tests run the host restatement)."""
        run = run or _device().greedy
        ll_lists = [[] for _ in points]
        for repeat in range(self.nit):
            folds = self.fold_kmer_table[repeat]  # [nfolds, n, 2]
            M = np.ascontiguousarray(folds[:, :, 0].T)
            U = np.ascontiguousarray(folds[:, :, 1].T)
            train_M = M.sum() - M.sum(axis=0)
            train_U = U.sum() - U.sum(axis=0)
            lanes = []
            for pi, (alpha, penalty) in enumerate(points):
                for fold in range(self.nfolds):
                    beta = get_betas(alpha, train_M[fold], train_U[fold])
                    lanes.append((fold, pi, alpha, beta, penalty))
            chain = run(self.genpat, M, U, lanes, self.nfolds)[1]
            for pi in range(len(points)):
                ll_lists[pi].append(float(chain[pi]))
        return [sum(ll_list) / len(ll_list) for ll_list in ll_lists]

    def loglik(self, alpha, penalty):
        """Mean over the repeats of the summed test -2 log-likelihood of all folds (ref :315-336)."""
        return self.logliks([(alpha, penalty)])[0]


class GridSearchCV(CrossValidation):
    """Grid search over pseudo counts and penalties (ref :338-353); the whole grid is one GPU
    job per repeat, evaluated on first use."""

    def __init__(self, genpat, contextD, penalties, pseudo_counts, nfolds=2, nit=1, seed=None, verbosity=1):
        super().__init__(genpat, contextD, nfolds=nfolds, nit=nit, seed=seed)
        self.penalties = penalties
        self.pseudo_counts = pseudo_counts
        self._grid = None

    def loglik(self, alpha, penalty):
        if self._grid is None:
            points = [(a, c) for a in self.pseudo_counts for c in self.penalties]
            self._grid = dict(zip(points, self.logliks(points)))
        if (alpha, penalty) in self._grid:
            return self._grid[(alpha, penalty)]
        return super().loglik(alpha, penalty)

    def get_best_a_c(self):
        best_combo = (None, None)
        best_ll = 1e100
        for a in self.pseudo_counts:
            for c in self.penalties:
                ll = self.loglik(a, c)
                if ll < best_ll:
                    best_ll = ll
                    best_combo = (a, c)
        return best_combo + (best_ll,)
