"""-m gpu: ``thin.heldout`` is ``factors.cell_equations``' Q called by hand, to the bit, and ``thin.rank_curve`` on a drawn log-bilinear
matrix of rank 3 (tests/thin_quality.py holds the protocol and the constants; tools/thin_calibration.py writes them from the numpy
models of THIN-1 and of the glmpca loop over 24 seeds, without the device):

  (a) Q(3) - Q(1) of the device's held-out curve lies above the models' mean - 5 sd: the true rank is seen;
  (b) Q(6) - Q(3) lies below the models' mean + 5 sd: ranks past the truth gain nothing held out;
  (c) under the Poisson law, where the two parts of a count are independent and the models' maximum is at the true rank in all
      24 seeds, ``best`` is 3.

Under smoke()'s law (alpha = 0.2, beta = 2) the two parts of an entry share its gamma rate.  The models' curve still rises to
the true rank (Q(3) - Q(1) = 4157 with sd 521) but is flat past it, Q(6) - Q(3) = -0.7 with sd 0.7, since the penalty holds the
factors past the third near 0; its maximum is at 3 in 22 of 24 seeds and at 6, by less than 1, in the other two.  (a) and (b)
are asserted under both laws, (c) under the Poisson law alone."""
import numpy as np
import pytest

import thin_quality as Q

pytestmark = pytest.mark.gpu


def _device(law):
    import torch
    X, sc = Q.draw(0, law)
    return torch.as_tensor(X.astype(np.int32)).cuda(), sc


def test_the_constants_are_calibrated():
    assert Q.SEEDS == 24 and Q.PEAK_AT_RANK["poisson"] == 1.0
    for law in Q.LAWS:
        assert Q.GAIN_3_OVER_1[law][0] - 5.0 * Q.GAIN_3_OVER_1[law][1] > 0 and Q.GAIN_6_OVER_3[law][1] > 0


def test_heldout_is_cell_equations_q_to_the_bit():
    from prosstt_amd import factors, thin
    X, sc = _device("smoke")
    alpha, beta = Q.LAWS["smoke"]
    s = thin.split(X, 0.5, seed=0)
    sc_train, sc_test = s.sizes(sc)
    f = factors.glmpca(s.train, sc_train, 2, alpha=alpha, beta=beta, max_rounds=2)
    got = thin.heldout(f, s.test, sc_test)
    loadings = np.concatenate([f.intercept[:, None], f.loadings], axis=1)
    coef = np.concatenate([np.ones((Q.N, 1)), f.scores], axis=1)
    by_hand = factors.cell_equations(s.test, sc_test, loadings, coef, alpha, beta).q
    assert got.per_cell.shape == (Q.N,) and got.per_cell.tobytes() == np.asarray(by_hand, dtype=np.float64).tobytes()
    assert got.total == float(np.asarray(by_hand).sum())
    # the parts are the model's, so the curve below is drawn on the matrices the calibration thinned
    import thin_model as T
    assert np.array_equal(s.train.cpu().numpy(), T.interval(Q.draw(0, "smoke")[0], 0, 32768, seed=0, sliced=True))


@pytest.mark.parametrize("law", list(Q.LAWS))
def test_the_rank_curve_sees_the_true_rank(law):
    from prosstt_amd import thin
    X, sc = _device(law)
    alpha, beta = Q.LAWS[law]
    curve = thin.rank_curve(X, sc, (1, 3, 6), alpha=alpha, beta=beta, fraction=0.5, seed=0)
    q1, q3, q6 = curve.heldout
    rise, past = Q.GAIN_3_OVER_1[law], Q.GAIN_6_OVER_3[law]
    print("%s: held-out Q(3) - Q(1) = %.1f (models %.1f, sd %.1f), Q(6) - Q(3) = %.1f (models %.1f, sd %.1f), best k = %d; on the "
          "train part Q(3) - Q(1) = %.1f, Q(6) - Q(3) = %.1f"
          % (law, q3 - q1, *rise, q6 - q3, *past, curve.best, curve.train[1] - curve.train[0], curve.train[2] - curve.train[1]))
    assert curve.ks == (1, 3, 6) and curve.best in curve.ks
    assert q3 - q1 > rise[0] - 5.0 * rise[1]
    assert q6 - q3 < past[0] + 5.0 * past[1]
    if law == "poisson":
        assert curve.best == Q.RANK
