"""What the numpy model of ``factors.glmpca`` reaches on smoke()'s tree, measured on the CPU without the device, and the scores
the GPU test (tests/test_gpu_factors_quality.py) shares with the measurement.  A helper: nothing here is collected.

The protocol (``python tools/factors_calibration.py``, which writes the constants below): the node means (60 x 300), size
factors, pseudotimes and branches of ``test_gpu_trends._simulation()`` are read from tests/golden/ptree_smoke_tree.npz; for each
of 24 seeds a 3 000 x 300 matrix of numpy's negative binomial (tests/ptree_quality.py's ``numpy_counts``: alpha = 0.2,
beta = 2), the model loop (tests/factors_model.py, numpy's own sums) with the package's defaults from the package's "pca" start
computed by numpy (``pca_start``).  Recorded, as (mean, standard deviation with ddof 1) over the seeds:

  (a) the rms over the cells and the genes with counts of the fitted minus the true log-mean at unit size;
  (b) the mean over the cells of the true tree distance to the 14 nearest neighbours in score space;
  (c) the same for ``ptree_quality.numpy_scores`` at equal k: the principal components of log1p(x / s).

The tree distance of two cells is the length of the path between them along smoke()'s tree in time steps: the difference of
their pseudotimes on one branch or on the root and a child, and through the fork (the root's last node) otherwise."""
import numpy as np

N_NEIGHBORS = 14
FORK = 19                        # the pseudotime of the root branch's last node: A has 20 steps

# written by tools/factors_calibration.py (DESIGN section 35 has the whole table) ---- begin
K, PENALTY, MAX_ROUNDS = 10, 50.0, 30
LOG_MEAN_RMS = (0.1904, 0.0027)
NEIGHBOUR_DISTANCE = (3.8127, 0.0520)
PCA_NEIGHBOUR_DISTANCE = (4.6465, 0.0711)
# ---- end
# the model's margin below PCA at its 5 sd low end, as regress's calibration has it
MARGIN = PCA_NEIGHBOUR_DISTANCE[0] - (NEIGHBOUR_DISTANCE[0] + 5.0 * NEIGHBOUR_DISTANCE[1])


def tree_distance_to(pt, br, i, neighbours):
    """(len(neighbours),) true tree distances from cell i."""
    pt = np.asarray(pt, dtype=np.float64)
    same = (br[neighbours] == br[i]) | (br[neighbours] == "A") | (br[i] == "A")
    return np.where(same, np.abs(pt[neighbours] - pt[i]), (pt[neighbours] - FORK) + (pt[i] - FORK))


def neighbour_distance(indices, pt, br):
    """(b): the mean over the cells of the mean true tree distance to the neighbours ``indices`` (N, n)."""
    br = np.asarray(br).astype("U1")
    return float(np.mean([tree_distance_to(pt, br, i, np.asarray(indices[i], dtype=np.int64)).mean() for i in range(len(pt))]))


def nearest(scores, n=N_NEIGHBORS):
    """(N, n) indices of the n nearest other cells in Euclidean distance, by numpy."""
    Y = np.asarray(scores, dtype=np.float64)
    sq = np.sum(Y * Y, axis=1)
    d2 = sq[:, None] + sq[None, :] - 2.0 * (Y @ Y.T)
    np.fill_diagonal(d2, np.inf)
    return np.argsort(d2, axis=1, kind="stable")[:, :n]


def log_mean_rms(linear_predictor, true_means, keep):
    """(a): the rms of linear_predictor - log(true means at unit size) over the cells and the genes ``keep``."""
    return float(np.sqrt(np.mean((linear_predictor[:, keep] - np.log(true_means[:, keep])) ** 2)))


def pca_start(x, sc, k):
    """``factors.glmpca``'s "pca" start by numpy: the scores and loadings of the first k principal components of
    log1p(x / s), each scaled by the square root of the singular value."""
    z = np.log1p(x / sc[:, None])
    z = z - z.mean(axis=0)
    u, s, vt = np.linalg.svd(z, full_matrices=False)
    root = np.sqrt(s[:k])
    return u[:, :k] * root[None, :], vt[:k].T * root[None, :]
