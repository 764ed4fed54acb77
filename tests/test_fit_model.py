"""The numpy model of the fit (tests/fit_model.py) against mpmath, ``fit.maximize`` on the model against scipy's L-BFGS-B,
and the likelihood ratios of a fit to draws from the model itself.  No GPU."""
import functools

import numpy as np
import pytest

import fit_model as M
from prosstt_amd import fit

XS = [0, 1, 2, 12, 13, 14, 37, 1000, 33047, 2 ** 31 - 1]
RS = 10.0 ** np.arange(-8.0, 12.01, 0.5)              # 41 values of r over 1e-8 .. 1e12
THETAS = 10.0 ** np.arange(-6.0, 6.01, 1.0)           # 13 values of theta over 1e-6 .. 1e6


def test_lgd_against_mpmath():
    """lgamma(r + x) - lgamma(r) on the grid, relative to itself (the value is 0 at r = x = 1).  Measured: 9.9e-16."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    worst = 0.0
    for x in XS[1:]:
        got = M.lgd(RS, np.full(RS.shape, x))
        for r, g in zip(RS.tolist(), got.tolist()):
            want = mp.loggamma(mp.mpf(r) + x) - mp.loggamma(mp.mpf(r))
            err = abs(mp.mpf(g) - want)
            worst = max(worst, float(err / abs(want)) if want != 0 else float(err))
    print("lgd against mpmath: worst relative error %.3g" % worst)
    assert worst <= 2.0 ** -40 / 400


def test_term_against_mpmath():
    """Every term on the grid r x x x theta, once at the quasi-Poisson end (a = 0, theta = b - 1, mu = r theta) and once at
    b = 1 (a = 1 / r, mu = r theta, so that theta = a mu and r moves over its grid there too):
    |model - mpmath| <= 2^-40 (|lgd| + r L1 + x |log theta - L1|).  Measured: 0.0014 of that cap."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    worst = 0.0
    for x in XS:
        for theta in THETAS.tolist():
            for textbook in (False, True):
                a = 1.0 / RS if textbook else np.zeros(RS.shape)
                bm1 = 0.0 if textbook else theta
                mu = RS * theta
                value, magnitude = M.term(mu, np.full(RS.shape, x), a, bm1)
                for m, a_, v, s in zip(mu.tolist(), a.tolist(), value.tolist(), magnitude.tolist()):
                    th = mp.mpf(a_) * mp.mpf(m) + mp.mpf(bm1)
                    r = mp.mpf(m) / th
                    l1 = mp.log1p(th)
                    want = (mp.loggamma(r + x) - mp.loggamma(r)) - r * l1 + x * (mp.log(th) - l1)
                    cap = 2.0 ** -40 * s
                    assert cap > 0
                    worst = max(worst, float(abs(mp.mpf(v) - want)) / cap)
    print("term against mpmath: worst error / cap %.3g" % worst)
    assert worst <= 1.0


def test_log_factorial_and_the_split_at_twelve():
    import math
    xs = np.array([0, 1, 2, 3, 12, 13, 14, 170, 33047, 2 ** 31 - 1])
    want = np.array([math.lgamma(int(x) + 1.0) for x in xs])
    np.testing.assert_allclose(M.log_factorial(xs), want, rtol=4e-15, atol=0)
    # the two forms of lgd meet: the product form taken past its range equals the Stirling form
    r = np.array([1e-8, 0.3, 1.0, 7.5, 15.9, 16.0, 123.0, 1e6, 1e12])
    product = np.log(np.prod([r + j for j in range(12)], axis=0)) + np.log(r + 12)
    np.testing.assert_allclose(M.lgd(r, np.full(r.shape, 13)), product, rtol=4e-15)


# ------------------------------------------------------------------------------------------------ optimiser vs scipy

def _draws(rng, N, G, K, a, b, mean_mu=0.5, mean_sigma=1.2):
    labels = rng.integers(0, K, size=N)
    sc = rng.lognormal(0.0, 0.35, size=N)
    means = rng.lognormal(mean_mu, mean_sigma, size=(K, G))
    mu = sc[:, None] * means[labels]
    theta = a * mu + (b - 1.0)
    X = rng.negative_binomial(mu / theta, 1.0 / (1.0 + theta))
    return X, sc, labels, means


@pytest.mark.parametrize("free,a,b", [(("alpha", "beta"), 0.2, 2.0), (("alpha",), 0.3, 1.0)])
def test_maximize_reaches_scipys_likelihood(free, a, b):
    """The shortfall of maximize's likelihood below L-BFGS-B's on the same function, 16 genes.  Measured with this seed:
    at most 9.1e-13 (both parameters free) and 1.8e-11 (alpha alone), the size of the rounding of a sum of 3 000 terms;
    OPTIMISER_BOUND is ten times the larger."""
    optimize = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(2024)
    X, sc, labels, means = _draws(rng, 3000, 16, 6, a, b)
    got = M.count_model(X, sc, labels, means, free=free)
    assert got.converged.all() and not got.at_bound.any()
    _, base, _, _ = M.loglik(X, sc, labels, means, np.full(16, 0.1), np.full(16, 2.0))
    shortfall = []
    for g in range(16):
        def negative(p, g=g):
            alpha = np.exp(p[0])
            beta = 1.0 + np.exp(p[1]) if len(free) == 2 else 1.0
            return -M.loglik(X[:, [g]], sc, labels, means[:, [g]], [alpha], [beta])[0][0, 0]
        start = [np.log(0.1), 0.0][:len(free)]
        best = min((optimize.minimize(negative, s, method="L-BFGS-B", bounds=[(-12.0, 4.0)] * len(free),
                                      options=dict(ftol=1e-15, gtol=1e-10)) for s in (start, [np.log(a), 0.0][:len(free)])),
                   key=lambda res: res.fun)
        shortfall.append((-best.fun - base[g]) - got.loglik[g])
    worst = max(shortfall)
    print("maximize against L-BFGS-B, free = %r: worst shortfall %.3g" % (free, worst))
    assert M.OPTIMISER_BOUND <= 1e-3
    assert worst <= M.OPTIMISER_BOUND


# ------------------------------------------------------------------------------------------------- likelihood ratio

@functools.lru_cache(maxsize=None)
def _likelihood_ratios():
    rng = np.random.default_rng(5)
    X, sc, labels, means = _draws(rng, 3000, 300, 60, 0.2, 2.0)
    got = M.count_model(X, sc, labels, means)
    ll, base, _, _ = M.loglik(X, sc, labels, means, np.full(300, 0.2), np.full(300, 2.0))
    return 2.0 * (got.loglik - (ll[0] - base)), got


def test_likelihood_ratio_against_the_truth_is_chi_square():
    """2 (l_hat - l_truth) of 300 genes drawn from the model with their true means: chi-square with 2 degrees of freedom.
    Measured: mean 1.84, 3.0 % above 5.99, 15 to 18 rounds."""
    lr, got = _likelihood_ratios()
    print("likelihood ratio: mean %.4f, max %.3f, min %.3g, above 5.99: %.3f, rounds %d - %d"
          % (lr.mean(), lr.max(), lr.min(), (lr > 5.99).mean(), got.rounds.min(), got.rounds.max()))
    assert got.converged.all() and not got.at_bound.any() and not got.bad.any()
    assert lr.min() >= -1e-6
    assert lr.max() <= 30.0                            # P(chi2_2 > 30) = 3e-7
    assert abs(lr.mean() - 2.0) <= 5.0 * 2.0 / np.sqrt(300)


def test_standard_errors_match_the_spread_of_the_estimates():
    """Over genes that share the truth, the standard deviation of log alpha_hat is what the Hessians say on average (the
    genes differ in their means, so only the order of magnitude is bound: within a factor 1.5)."""
    _, got = _likelihood_ratios()
    spread_u = np.std(np.log(got.alpha), ddof=1)
    spread_v = np.std(np.log(got.beta - 1.0), ddof=1)
    said_u = np.sqrt(np.mean(got.se_log_alpha ** 2))
    said_v = np.sqrt(np.mean(got.se_log_beta_minus_1 ** 2))
    print("spread of log alpha %.4f (standard errors say %.4f), of log(beta - 1) %.4f (%.4f)" % (spread_u, said_u, spread_v, said_v))
    assert np.all(np.isfinite(got.hessian)) and np.all(got.hessian[:, 0] < 0) and np.all(got.hessian[:, 2] < 0)
    assert 1 / 1.5 <= spread_u / said_u <= 1.5 and 1 / 1.5 <= spread_v / said_v <= 1.5
    hp = fit.hyperparameters(got)
    assert hp.n_genes == 300 and hp.log_alpha_std == pytest.approx(spread_u) and hp.log_beta_minus_1_std == pytest.approx(spread_v)
