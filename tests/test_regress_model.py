"""tests/regress_model.py, the numpy model that the device pass of prosstt_amd/regress.py is tested against, pinned without a
GPU: its fit against scipy's maximum of the exact negative-binomial likelihood at beta = 1, against the closed form of a
one-hot design at alpha = 0 and beta = 1, its score and information against central differences of its Q, and its sums against
rational arithmetic where every term is an integer."""
from fractions import Fraction

import numpy as np
import pytest

import regress_model as M

from prosstt_amd import regress


def _problem(seed, N=240, G=24, p=3, a=0.3):
    """Covariates per cell (K = N, labels 0 .. N - 1), negative-binomial counts with dispersion ``a`` at beta = 1."""
    rng = np.random.default_rng(seed)
    D = np.column_stack([np.ones(N)] + [rng.normal(0.0, 0.6, size=N) for _ in range(p - 1)])
    truth = np.column_stack([rng.normal(1.5, 0.5, size=G)] + [rng.normal(0.0, 0.4, size=G) for _ in range(p - 1)])
    sc = rng.lognormal(0.0, 0.3, size=N)
    mu = sc[:, None] * np.exp(D @ truth.T)
    X = rng.negative_binomial(1.0 / a, 1.0 / (1.0 + a * mu)) if a > 0 else rng.poisson(mu)
    return X.astype(np.int64), sc, np.arange(N), D, truth


def test_the_fit_is_scipys_maximum_of_the_exact_negative_binomial_likelihood_at_beta_one():
    import scipy.optimize
    import scipy.stats
    a = 0.3
    X, sc, labels, D, _ = _problem(5, a=a)
    got = M.regression(X, sc, labels, D, a, 1.0, tol=1e-13, max_rounds=50)
    assert got.converged.all() and not got.separated.any() and not got.no_counts.any()
    assert got.rounds.max() <= 12
    for g in range(X.shape[1]):
        def negative(c, g=g):
            mu = sc * np.exp(D @ c)
            return -scipy.stats.nbinom.logpmf(X[:, g], 1.0 / a, 1.0 / (1.0 + a * mu)).sum()
        best = scipy.optimize.minimize(negative, got.coef[g] + 0.05, method="BFGS", options={"gtol": 1e-9})
        np.testing.assert_allclose(got.coef[g], best.x, rtol=0, atol=2e-6)
        assert negative(got.coef[g]) <= best.fun + 1e-9


def test_a_one_hot_design_at_alpha_zero_and_beta_one_has_the_closed_form():
    rng = np.random.default_rng(11)
    N, G, K = 300, 17, 5
    labels = rng.integers(-1, K, size=N)
    sc = rng.lognormal(0.0, 0.4, size=N)
    X = rng.poisson(sc[:, None] * rng.lognormal(1.0, 0.7, size=(K, G))[np.maximum(labels, 0)])
    got = M.regression(X, sc, labels, regress.group_design(K), 0.0, 1.0, tol=1e-14, max_rounds=50)
    assert got.converged.all()
    want = np.stack([X[labels == k].sum(axis=0) / sc[labels == k].sum() for k in range(K)], axis=1)        # (G, K)
    # the stopping rule bounds the change of Q, not of the coefficients: a step of size e changes Q by I e^2 / 2, so a gene
    # may stop within sqrt(2 tol (|Q| + 1) / I) of the maximiser -- 2e-6 here (tol 1e-14, |Q| about 1e4, I about 50)
    np.testing.assert_allclose(np.exp(got.coef), want, rtol=1e-5)
    np.testing.assert_allclose(got.fitted(), want.T, rtol=1e-5)
    # the information is diagonal: sum of mu per group, and the covariance its inverse
    counts = np.stack([X[labels == k].sum(axis=0) for k in range(K)], axis=1).astype(np.float64)
    np.testing.assert_allclose(np.diagonal(got.cov, axis1=1, axis2=2), 1.0 / counts, rtol=1e-5)


@pytest.mark.parametrize("a,b", [(0.3, 1.0), (0.2, 2.0), (0.0, 1.0), (0.0, 3.0)])
def test_the_score_is_the_gradient_of_q_and_the_information_its_expected_hessian(a, b):
    X, sc, labels, D, truth = _problem(3, N=60, G=6, p=3, a=max(a, 0.1))
    coef = truth + 0.1
    at = M.normal_equations(X, sc, labels, D, coef, a, b)
    assert at.status == 0 and np.array_equal(at.ne.used, np.full(6, 60))
    h = 1e-5
    p = D.shape[1]
    for j in range(p):
        e = np.zeros(p)
        e[j] = h
        up = M.normal_equations(X, sc, labels, D, coef + e, a, b).ne
        down = M.normal_equations(X, sc, labels, D, coef - e, a, b).ne
        np.testing.assert_allclose((up.q - down.q) / (2 * h), at.ne.score[:, j], rtol=2e-6, atol=1e-6)
    # x = mu makes the Hessian its own expectation (it is linear in x): coefficients 0 and integer size factors
    size = np.random.default_rng(8).integers(1, 9, size=60).astype(np.float64)
    Xm = np.repeat(size[:, None], 6, axis=1).astype(np.int64)
    zero = np.zeros((6, p))
    at = M.normal_equations(Xm, size, labels, D, zero, a, b).ne
    assert np.abs(at.score).max() <= 1e-12
    for j in range(p):
        e = np.zeros(p)
        e[j] = h
        up = M.normal_equations(Xm, size, labels, D, zero + e, a, b).ne
        down = M.normal_equations(Xm, size, labels, D, zero - e, a, b).ne
        np.testing.assert_allclose(-(up.score - down.score) / (2 * h), at.information[:, j, :], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("meat", [False, True])
def test_the_exact_case_against_rational_arithmetic(meat):
    """coef = 0, s = 1, alpha = 0, beta = 1, design entries in {0, +-1, +-2}, counts below 64: mu = d = w = 1 and u = x - 1,
    every product and sum an integer, whatever the order (700 rows: two blocks of rows)."""
    rng = np.random.default_rng(21)
    N, G, K, p = 700, 5, 9, 4
    X = rng.integers(0, 64, size=(N, G))
    D = rng.integers(-2, 3, size=(K, p)).astype(np.float64)
    labels = rng.integers(-1, K, size=N)
    assert regress.row_blocks(N, G)[1] > 1
    got = M.normal_equations(X, np.ones(N), labels, D, np.zeros((G, p)), 0.0, 1.0, meat)
    assert got.status == 0
    for g in range(G):
        for j in range(p):
            want = sum(Fraction(int(D[labels[i], j])) * (int(X[i, g]) - 1) for i in range(N) if labels[i] >= 0)
            assert Fraction(got.ne.score[g, j]) == want
            for k in range(p):
                want = sum(Fraction(int(D[labels[i], j] * D[labels[i], k])) * ((int(X[i, g]) - 1) ** 2 if meat else 1)
                           for i in range(N) if labels[i] >= 0)
                assert Fraction(got.ne.information[g, j, k]) == want
    assert np.array_equal(got.ne.used, np.full(G, int((labels >= 0).sum())))


def test_the_model_names_the_status_bits():
    X, sc, labels, D, truth = _problem(4, N=40, G=4, p=2)
    clean = M.normal_equations(X, sc, labels, D, truth, 0.2, 2.0)
    assert clean.status == 0
    bad = X.copy()
    bad[3, 1] = -1
    assert M.normal_equations(bad, sc, labels, D, truth, 0.2, 2.0).status == regress.NEGATIVE
    lab = labels.copy()
    lab[5] = 40
    assert M.normal_equations(X, sc, lab, D, truth, 0.2, 2.0).status == regress.LABEL
    s = sc.copy()
    s[7] = 0.0
    assert M.normal_equations(X, s, labels, D, truth, 0.2, 2.0).status == regress.SIZE
    assert M.normal_equations(X, sc, labels, D, truth, 0.2, 0.5).status == regress.PARAMETER
    c = truth.copy()
    c[0, 0] = np.nan
    assert M.normal_equations(X, sc, labels, D, c, 0.2, 2.0).status == regress.COEFFICIENT
    c = truth.copy()
    c[2, 0] = 800.0
    assert M.normal_equations(X, sc, labels, D, c, 0.2, 2.0).status == regress.ETA
