"""tests/mapping_model.py pinned without the package: the scores against rational arithmetic, the tie rule of the argmax, the
log-sum-exps against math.fsum and scipy, the Poisson score against scipy's log-pmf (differences between nodes, where the
constant of the cell cancels), and the centring of the panel, which changes no argmax and no posterior.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import mapping_model as mm


def _case(N=5, G=7, R=4, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.poisson(4.0, size=(N, G)).astype(np.int32)
    P = rng.standard_normal((R, G)).astype(np.float32)
    s = rng.lognormal(0.0, 0.5, N)
    m = rng.standard_normal(R) * 10
    c = rng.standard_normal(R)
    return X, s, P, m, c


def test_scores_against_rational_arithmetic():
    X, s, P, m, c = _case()
    S = mm.scores(X, s, P, m, c)
    b = mm.bound(X, s, P, m, c, 256)
    assert S.shape == (5, 4)
    for i in range(5):
        for r in range(4):
            exact = sum(Fraction(int(X[i, g])) * Fraction(float(P[r, g])) for g in range(7)) \
                - Fraction(float(s[i])) * Fraction(float(m[r])) + Fraction(float(c[r]))
            # the model's own error: the binary64 roundings, a fraction of the bound it is the reference of
            assert abs(Fraction(float(S[i, r])) - exact) <= Fraction(float(b[i, r])) / 1000, (i, r)
    # on dyadic inputs every step is exact
    Xd = (X % 8).astype(np.int32)
    Pd = (np.round(P * 4) / 8).astype(np.float32)
    sd, md, cd = np.round(s * 4) / 4, np.round(m), np.round(c * 8) / 8
    Sd = mm.scores(Xd, sd, Pd, md, cd)
    for i in range(5):
        for r in range(4):
            exact = sum(Fraction(int(Xd[i, g])) * Fraction(float(Pd[r, g])) for g in range(7)) \
                - Fraction(float(sd[i])) * Fraction(float(md[r])) + Fraction(float(cd[r]))
            assert Fraction(float(Sd[i, r])) == exact


def test_the_argmax_takes_the_lower_node_of_a_tie_and_never_a_nan():
    nan = float("nan")
    S = np.array([[1.0, 3.0, 3.0, 2.0], [nan, -5.0, nan, -5.0], [nan, nan, nan, nan], [2.0, 2.0, 2.0, 2.0],
                  [-np.inf, -np.inf, 0.0, nan], [0.0, -0.0, 0.0, -1.0]])
    assert mm.best(S).tolist() == [1, 1, 0, 0, 2, 0]
    assert mm.best(S).dtype == np.int32


def test_lse_against_fsum_and_scipy():
    from scipy.special import logsumexp
    rng = np.random.default_rng(8)
    S = rng.standard_normal((9, 33)) * 50 - 700            # exp(S) underflows without the shift
    got = mm.lse(S)
    np.testing.assert_allclose(got, logsumexp(S, axis=1), rtol=1e-14)
    for i in range(9):
        top = max(S[i])
        assert got[i] == math.log(math.fsum(math.exp(v - top) for v in S[i])) + top
    offsets = np.array([0, 1, 1, 20, 33])
    bl = mm.branch_lse(S, offsets)
    assert bl.shape == (9, 4) and np.all(np.isneginf(bl[:, 1]))
    assert np.array_equal(bl[:, 0], S[:, 0])                # a branch of one node
    np.testing.assert_allclose(bl[:, 3], logsumexp(S[:, 20:], axis=1), rtol=1e-14)
    np.testing.assert_allclose(logsumexp(bl, axis=1), got, rtol=1e-14)


def test_the_score_is_the_poisson_log_likelihood_up_to_a_constant_of_the_cell():
    from scipy.stats import poisson
    rng = np.random.default_rng(5)
    R, G, N = 6, 40, 8
    means = rng.gamma(2.0, 2.0, size=(R, G))
    s = rng.lognormal(0.0, 0.5, N)
    X = rng.poisson(s[:, None] * means[rng.integers(0, R, N)]).astype(np.int32)
    panel, exposure = mm.poisson_panel(means)
    S = mm.scores(X, s, panel, exposure)
    ll = np.array([[poisson.logpmf(X[i], s[i] * means[r]).sum() for r in range(R)] for i in range(N)])
    # differences between nodes: the constant of the cell cancels; what is left is the float32 rounding of the panel
    A = np.abs(X).astype(np.float64) @ np.abs(panel).astype(np.float64).T
    tol = 2.0 ** -24 * (A + A[:, :1]) + 1e-9
    assert np.all(np.abs((S - S[:, :1]) - (ll - ll[:, :1])) <= tol)
    assert np.array_equal(mm.best(S), np.argmax(ll, axis=1))


def test_centring_changes_no_argmax_and_no_posterior():
    rng = np.random.default_rng(6)
    R, G, N = 7, 30, 12
    means = rng.gamma(2.0, 2.0, size=(R, G))
    means[2, 5] = 0.0                                       # floored
    s = rng.lognormal(0.0, 0.5, N)
    X = rng.poisson(3.0, size=(N, G)).astype(np.int32)
    panel, exposure = mm.poisson_panel(means)
    assert panel.dtype == np.float32 and abs(float(np.sum(panel.astype(np.float64), axis=0).max())) < 1e-4
    assert abs(exposure.sum()) < 1e-9
    mfl = np.maximum(means, 1e-7)
    raw = mm.scores(X, s, np.log(mfl), mfl.sum(axis=1))     # not centred, the logs in binary64
    S = mm.scores(X, s, panel, exposure)
    assert np.array_equal(mm.best(S), mm.best(raw))
    post, post_raw = np.exp(S - mm.lse(S)[:, None]), np.exp(raw - mm.lse(raw)[:, None])
    np.testing.assert_allclose(post, post_raw, rtol=1e-4, atol=1e-12)
    # weights: a weight of zero removes a gene
    w = np.ones(G)
    w[3] = 0.0
    pw, ew = mm.poisson_panel(means, w)
    assert np.all(pw[:, 3] == 0)
    keep = np.arange(G) != 3
    p2, e2 = mm.poisson_panel(means[:, keep])
    assert np.array_equal(pw[:, keep], p2) and np.allclose(ew, e2, rtol=0, atol=1e-12)
    # nothing below 2^-100 in magnitude but zero
    flat, _ = mm.poisson_panel(np.full((3, 4), 2.5))
    assert np.all(flat == 0)


def test_the_argmax_rule_accepts_what_the_bound_allows_and_nothing_else():
    S = np.array([[0.0, 1.0, 0.5], [0.0, 1.0, 0.9999]])
    b = np.full((2, 3), 1e-3)
    assert mm.margins(S, b).tolist() == [True, False]
    assert mm.check_argmax(S, b, [1, 2]) == 0.5
    # (a clear best node that is missed also breaks the first half of the rule, which is checked first)
    for wrong in ([2, 1], [1, 0]):
        with pytest.raises(AssertionError, match="below the model's best"):
            mm.check_argmax(S, b, wrong)


def test_node_table_and_tree_distance():
    top, time = [["A", "B"], ["A", "C"]], {"A": 3, "B": 2, "C": 4}
    offsets, code, when = mm.node_table(top, time, ["A", "B", "C"], "A")
    assert offsets.tolist() == [0, 3, 5, 9]
    assert code.tolist() == [0, 0, 0, 1, 1, 2, 2, 2, 2]
    assert when.tolist() == [0, 1, 2, 3, 4, 3, 4, 5, 6]
    d = mm.tree_distance(top, time, ["A", "B", "C"], "A", [0, 2, 3, 4, 8], [2, 3, 5, 8, 8])
    assert d.tolist() == [2, 1, 2, 6, 0]
