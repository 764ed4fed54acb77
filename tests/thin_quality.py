"""What the numpy models of THIN-1 and of ``factors.glmpca`` say of ``thin.rank_curve``, measured on the CPU without the device,
and the protocol the GPU test (tests/test_gpu_thin_heldout.py) shares with the measurement.  A helper: nothing here is collected.

The protocol (``python tools/thin_calibration.py``, which writes the constants below): for each of 24 seeds a 600 x 200 matrix
from a log-bilinear truth of rank 3 (tests/test_factors_model.py's ``_bilinear`` at level 1: normal scores, loadings of standard
deviation 0.3, means around 3), under the Poisson law (alpha = 0, beta = 1) and under smoke()'s (alpha = 0.2, beta = 2); the
model's split at 1/2 (tests/thin_model.py, seed = the draw's); for k = 1 .. 6 the model loop (tests/factors_model.py, numpy's own
sums) on the train part with half the size factors, from the "pca" start computed by numpy, with the package's defaults; the
held-out Q is the model's ``cell_equations`` of the test part at the fit.  Recorded per law: the share of seeds whose held-out
maximum is at k = 3, and (mean, standard deviation with ddof 1) of Q(3) - Q(1) and of Q(6) - Q(3)."""
import numpy as np

N, G, RANK, LEVEL = 600, 200, 3, 1.0
KS = (1, 2, 3, 4, 5, 6)
LAWS = {"poisson": (0.0, 1.0), "smoke": (0.2, 2.0)}

# written by tools/thin_calibration.py (DESIGN section 37 has the whole table) ---- begin
SEEDS = 24
PEAK_AT_RANK = {"poisson": 1.0000, "smoke": 0.9167}
GAIN_3_OVER_1 = {"poisson": (15909.8, 1624.0), "smoke": (4157.5, 520.5)}
GAIN_6_OVER_3 = {"poisson": (-14.1, 6.6), "smoke": (-0.7, 0.7)}
# ---- end


def draw(seed, law):
    """(X int64 (N, G), sc) of seed ``seed`` under ``law``."""
    import test_factors_model
    alpha, beta = LAWS[law]
    X, sc, _, _ = test_factors_model._bilinear(np.random.default_rng(1000 + seed), N, G, RANK, LEVEL, alpha, beta)
    return np.asarray(X, dtype=np.int64), sc


def model_heldout(f, test, sc_test, alpha, beta):
    """The model's held-out Q of the fit ``f``: what ``thin.heldout`` asks of the device."""
    import factors_model as M
    loadings = np.concatenate([f.intercept[:, None], f.loadings], axis=1)
    coef = np.concatenate([np.ones((f.scores.shape[0], 1)), f.scores], axis=1)
    return float(M.cell_equations(test, sc_test, loadings, coef, alpha, beta, ordered=False).eq.q.sum())


def model_curve(seed, law, ks=KS):
    """(len(ks),) held-out Q by the models alone."""
    import factors_model as M
    import factors_quality
    import thin_model as T
    alpha, beta = LAWS[law]
    X, sc = draw(seed, law)
    train = T.interval(X, 0, T.GRID // 2, seed=seed, sliced=True)
    test = X - train
    out = []
    for k in ks:
        scores, loadings = factors_quality.pca_start(train, 0.5 * sc, k)
        f = M.glmpca(train, 0.5 * sc, scores, alpha, beta, loadings=loadings, ordered=False, transposed=True)
        out.append(model_heldout(f, test, 0.5 * sc, alpha, beta))
    return np.array(out)
