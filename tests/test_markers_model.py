"""The numpy model of the marker-gene step (tests/markers_model.py) against scipy: Welch's t-test from per-group sums, the
over-estimated variance, Benjamini-Hochberg, and a planted-marker case.  No GPU, and nothing of the package."""
import numpy as np
import pytest
import scipy.stats

import markers_model as mm

G = 50
PLANTED = 7                     # a gene that is 0 in every cell: vn1 + vn2 = 0


def _case(N, K, seed=0):
    """(A binary64 (N, G), labels, X): Poisson counts with gene means in [3, 30] (so that log1p(x / s) has a variance well
    above 1e-3 in every group: about 1 / mean, 0.03 at the least), size factors in [0.5, 2], interleaved labels, a
    small shift of the mean in group 0, and the planted constant gene."""
    rng = np.random.default_rng(1000 * N + K + seed)
    labels = rng.permutation(np.arange(N) % K)
    mean = rng.uniform(3.0, 30.0, size=G)
    s = rng.uniform(0.5, 2.0, size=N)
    lam = mean[None, :] * s[:, None] * np.where(labels == 0, 1.2, 1.0)[:, None]
    X = rng.poisson(lam)
    X[:, PLANTED] = 0
    return mm.dense(X, s), labels, X


@pytest.mark.parametrize("N", [40, 300])
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("rows_per_block", [7, 1000])
def test_welch_against_scipy(N, K, rows_per_block):
    A, labels, X = _case(N, K)
    S1, S2, n = mm.sums(A, labels, rows_per_block)
    nz = np.stack([(X[labels == k] > 0).sum(0) for k in range(K)])
    st = mm.statistics(S1, S2, nz, n)
    for k in range(K):
        own, rest = A[labels == k], A[labels != k]
        # the variance from the sums: the roundings of S2, of S1^2 / n, and of the subtraction and division
        for v, part, s2, cells in ((st["v1"][k], own, S2[k], len(own)), (st["v2"][k], rest, S2.sum(0) - S2[k], len(rest))):
            bound = cells * 2.0 ** -51 * s2 / (cells - 1)
            assert np.all(np.abs(v - np.var(part, axis=0, ddof=1)) <= bound)
        want = scipy.stats.ttest_ind(own, rest, equal_var=False, axis=0)
        ok = (st["v1"][k] > 1e-3) & (st["v2"][k] > 1e-3)
        assert set(np.flatnonzero(~ok)) <= {PLANTED}            # every other gene is compared
        np.testing.assert_allclose(st["t"][k][ok], want.statistic[ok], rtol=1e-9, atol=0)
        np.testing.assert_allclose(st["df"][k][ok], want.df[ok], rtol=1e-9, atol=0)
        np.testing.assert_allclose(st["pvals"][k][ok], want.pvalue[ok], rtol=1e-9, atol=0)
        # the constant gene: scipy divides 0 by 0; the definition says t = 0, p = 1
        assert st["t"][k][PLANTED] == 0 and st["pvals"][k][PLANTED] == 1
        np.testing.assert_array_equal(st["pts"][k], (X[labels == k] > 0).mean(0))
        np.testing.assert_array_equal(st["pts_rest"][k], (X[labels != k] > 0).mean(0))
        m1, m2 = own.mean(0), rest.mean(0)
        np.testing.assert_allclose(st["logfoldchanges"][k], np.log2((np.expm1(m1) + 1e-9) / (np.expm1(m2) + 1e-9)), rtol=1e-10,
                                   atol=1e-12)


def test_a_reference_group():
    A, labels, X = _case(300, 4)
    S1, S2, n = mm.sums(A, labels, 64)
    nz = np.stack([(X[labels == k] > 0).sum(0) for k in range(4)])
    st = mm.statistics(S1, S2, nz, n, reference=2)
    ok = np.arange(G) != PLANTED
    for k in (0, 1, 3):
        want = scipy.stats.ttest_ind(A[labels == k], A[labels == 2], equal_var=False, axis=0)
        np.testing.assert_allclose(st["t"][k][ok], want.statistic[ok], rtol=1e-9, atol=0)
        np.testing.assert_allclose(st["pvals"][k][ok], want.pvalue[ok], rtol=1e-9, atol=0)
    assert not st["t"][2].any()                                 # the reference against itself


@pytest.mark.parametrize("N,K", [(40, 2), (300, 4)])
def test_overestimated_variance(N, K):
    """vn2 = v2 / n1: the statistic is Welch's with n2 := n1; df keeps n2 - 1 in its second term."""
    A, labels, X = _case(N, K)
    S1, S2, n = mm.sums(A, labels, 64)
    st = mm.statistics(S1, S2, np.zeros_like(S1), n, method="t-test_overestim_var")
    ok = np.arange(G) != PLANTED
    for k in range(K):
        own, rest = A[labels == k], A[labels != k]
        n1, n2 = len(own), len(rest)
        v1, v2 = np.var(own, axis=0, ddof=1), np.var(rest, axis=0, ddof=1)
        want = scipy.stats.ttest_ind_from_stats(own.mean(0), np.sqrt(v1), n1, rest.mean(0), np.sqrt(v2), n1, equal_var=False)
        np.testing.assert_allclose(st["t"][k][ok], want.statistic[ok], rtol=1e-9, atol=0)
        vn1, vn2 = v1 / n1, v2 / n1
        with np.errstate(invalid="ignore"):
            df = (vn1 + vn2) ** 2 / (vn1 ** 2 / (n1 - 1) + vn2 ** 2 / (n2 - 1))
        np.testing.assert_allclose(st["df"][k][ok], df[ok], rtol=1e-9, atol=0)
        np.testing.assert_allclose(st["pvals"][k][ok], 2 * scipy.stats.t.sf(np.abs(want.statistic), df)[ok], rtol=1e-9, atol=0)


def test_benjamini_hochberg():
    rng = np.random.default_rng(5)
    for p in (rng.uniform(size=50), rng.uniform(size=50) ** 6, np.r_[rng.uniform(size=20), np.ones(5), np.zeros(3), [0.2] * 4],
              np.array([0.3])):
        np.testing.assert_allclose(mm.bh(p), scipy.stats.false_discovery_control(p, method="bh"), rtol=1e-15, atol=0)
    assert np.all(mm.bh([0.01, 0.04, 0.03, 0.5]) == np.array([0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5]))


def test_fewer_than_two_cells():
    S = np.ones((2, 3))
    with pytest.raises(ValueError):
        mm.statistics(S, S, S, [1, 5])
    with pytest.raises(ValueError):
        mm.statistics(S, S, S, [5, 1])


def planted_case(seed=11, N=240, genes=60, K=3):
    """(X, s, labels): Poisson counts with genes 0 .. 9 drawn with ten times the mean in group 1."""
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.arange(N) % K)
    mean = rng.uniform(1.0, 4.0, size=genes)
    s = rng.uniform(0.5, 2.0, size=N)
    lam = mean[None, :] * s[:, None] * np.ones((N, genes))
    lam[np.ix_(labels == 1, np.arange(10))] *= 10.0
    return rng.poisson(lam).astype(np.int32), s, labels


def test_planted_markers_come_first():
    X, s, labels = planted_case()
    S1, S2, n = mm.sums(mm.dense(X, s), labels, 64)
    nz = np.stack([(X[labels == k] > 0).sum(0) for k in range(3)])
    st = mm.statistics(S1, S2, nz, n)
    names = mm.rank(st["t"])
    assert set(names[1][:10]) == set(range(10))
    assert np.all(st["pvals_adj"][1][:10] < 1e-20) and np.all(st["logfoldchanges"][1][:10] > 2.5)
    assert np.all(np.diff(st["t"][1][names[1]]) <= 0)
