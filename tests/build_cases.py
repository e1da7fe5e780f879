"""Shapes of the sweep-build matrix (tests/test_gpu_builds.py), shared with the host-side
cut tests (tests/test_device_groups.py): which user groups make kp_pass launch which build of
kp_dp_kernel<CT, NL, HZ, MIX>.  No GPU and no counts here: betas are passed in."""

NF = 3
PENS = [1.0, 2.0, 3.0, 5.0, 7.0, 9.0, 12.0, 16.0]
ALPHA1, ALPHA2 = 0.5, 2.0
# the product-path case: the usual 5-penalty grid with two alphas
GRID_ALPHAS = [0.5, 2.0]
GRID_PENS = [1, 2, 3, 5, 7]


def mixed_splits(width):
    """(n1, n2): lanes of the first and of the second (alpha, beta) set of a mixed workgroup
    of ``width`` lanes; js = n1 at both ends of its range (one split at width 2)."""
    return sorted({(width - 1, 1), (1, width - 1)})


def single_groups(width, beta_of, folds=range(NF), alpha=ALPHA1):
    """One full workgroup per fold: ``width`` penalties of one alpha.  ``beta_of(alpha, fold)``."""
    return [(f, alpha, beta_of(alpha, f), PENS[:width]) for f in folds]


def mixed_groups(n1, n2, beta_of, folds=range(NF), alphas=(ALPHA1, ALPHA2)):
    """Per fold two consecutive groups, ``n1`` penalties of the first alpha and ``n2`` of the
    second, both from the head of PENS: kp_pass cuts each fold's n1 + n2 lanes into one mixed
    workgroup, and the lanes (alpha1, PENS[0]) and (alpha2, PENS[0]) both exist."""
    out = []
    for f in folds:
        out.append((f, alphas[0], beta_of(alphas[0], f), PENS[:n1]))
        out.append((f, alphas[1], beta_of(alphas[1], f), PENS[:n2]))
    return out


def grid_groups(beta_of, folds):
    """The CV driver's groups of the 2 alpha x 5 penalty grid (alpha-major, the folds in the
    order given)."""
    return [(f, a, beta_of(a, f), list(GRID_PENS)) for a in GRID_ALPHAS for f in folds]
