"""The checking model of the highly-variable-gene selection (tests/hvg_model.py) against what it must equal by
construction: its loess returns quadratic data unchanged, is numpy's weighted polyfit at the target and handles ties in x;
the integer route of the clipped sums equals the np.minimum route; the bins are pandas' own.  No GPU."""
import numpy as np
import pytest

import hvg_model as M


def test_loess_returns_quadratic_data():
    rng = np.random.default_rng(0)
    x = np.sort(rng.uniform(-2.0, 1.0, size=200))
    y = 0.7 - 1.3 * x + 0.4 * x * x
    # a consistent system: the residual is 0, the error that of lstsq on a design of condition ~ 1 / h^2 <= 1e3
    np.testing.assert_allclose(M.loess(x, y, 0.3), y, rtol=0, atol=1e-11)
    np.testing.assert_allclose(M.loess(x, y, 1.0), y, rtol=0, atol=1e-11)


@pytest.mark.parametrize("span", [0.1, 0.3, 0.75])
def test_loess_is_the_weighted_polyfit_at_the_target(span):
    rng = np.random.default_rng(1)
    x = rng.normal(size=150)
    y = np.sin(x) + rng.normal(0.0, 0.2, size=150)
    got = M.loess(x, y, span)
    q = min(150, max(3, int(np.floor(span * 150 + 1e-5))))
    for i in (0, 17, 149, int(np.argmin(x)), int(np.argmax(x))):
        d = np.abs(x - x[i])
        h = np.sort(d)[q - 1]
        w = np.where(d < h, (1.0 - (d / h) ** 3) ** 3, 0.0)
        keep = w > 0
        want = np.polyfit(x[keep] - x[i], y[keep], 2, w=np.sqrt(w[keep]))[-1]
        np.testing.assert_allclose(got[i], want, rtol=1e-10, atol=1e-12)


def test_loess_with_ties_in_x():
    x = np.repeat([0.0, 1.0, 3.0], 5)
    y = np.arange(15, dtype=np.float64) ** 1.5
    # q = 4 < 5 equal x: h = 0 everywhere, the mean of y at the ties
    np.testing.assert_allclose(M.loess(x, y, 0.3), np.repeat([y[:5].mean(), y[5:10].mean(), y[10:].mean()], 5), rtol=1e-14)
    # q = 7: at x0 = 0 the two nearest others lie AT h = 1 and weigh nothing: one distinct x, a rank-1 system
    # q = 12: at x0 = 0 h = 3, so x = 0 and x = 1 weigh: two distinct x, a rank-2 system whose every solution has the same
    # intercept, the mean of y at x0
    for span in (0.5, 0.8):
        np.testing.assert_allclose(M.loess(x, y, span)[:5], np.full(5, y[:5].mean()), rtol=1e-12)


def test_loess_on_tie_heavy_means_is_finite_and_between_the_data():
    for kind in ("ties", "flat"):
        x, y = M.tie_heavy(kind)
        fit = M.loess(x, y)
        assert np.all(np.isfinite(fit)) and fit.min() >= y.min() - 0.5 and fit.max() <= y.max() + 0.5
        for v in np.unique(x):                         # equal x, equal fit
            assert np.ptp(fit[x == v]) <= 1e-12


@pytest.mark.parametrize("which", ["small", "wide"])
def test_integer_route_equals_the_minimum_route(which):
    X, _, n_top, _ = M.inputs(which)
    X = X.copy()
    X[3, 5] = 10 ** 4                                  # an entry that is clipped for certain
    n = X.shape[0]
    mean, var = M.count_moments(X)
    reg_std, clip = M.seurat_v3_fit(mean, var, n)
    thr = np.floor(clip).astype(np.int64)
    X64 = X.astype(np.int64)
    over = X64 > thr[None, :]
    assert over.any() and not over.all()
    kept = np.where(over, 0, X64)
    n_over = over.sum(axis=0)
    sum_c = kept.sum(axis=0) + n_over * clip
    sq_c = (kept * kept).sum(axis=0) + n_over * clip ** 2
    want_sum, want_sq = M.clipped_moments(X, clip)
    # either route sums n non-negative binary64 terms: within n 2^-53 of exact each
    np.testing.assert_allclose(sum_c, want_sum, rtol=n * 2.0 ** -52)
    np.testing.assert_allclose(sq_c, want_sq, rtol=n * 2.0 ** -52)
    vn = M.variances_norm(n, mean, var, reg_std, sum_c, sq_c)
    assert np.array_equal(M.top(vn, n_top), M.seurat_v3(X, n_top)["mask"])


def test_top_breaks_ties_by_index_and_puts_nan_last():
    score = np.array([1.0, np.nan, 3.0, 3.0, 1.0, np.nan])
    assert M.top(score, 1).tolist() == [False, False, True, False, False, False]
    assert M.top(score, 3).tolist() == [True, False, True, True, False, False]
    assert M.top(score, 5).tolist() == [True, True, True, True, True, False]


def test_seurat_bins_one_gene_bin_and_zero_variance():
    # 4 bins over m = log1p(mean); the last bin holds one gene; gene 0 has no variance
    mean = np.array([1.0, 1.1, 1.2, 2.0, 2.1, 2.2, 9.0])
    var = np.array([0.0, 2.0, 3.0, 1.0, 4.0, 2.5, 5.0])
    n = 10
    s1 = mean * n
    s2 = var * (n - 1) + s1 * mean
    got = M.seurat(s1, s2, n, n_top=3, n_bins=4)
    d = got["dispersions"]
    assert np.isnan(d[0]) and np.isnan(got["dispersions_norm"][0])
    np.testing.assert_allclose(d[1:], np.log(var[1:] / mean[1:]), rtol=1e-12)
    np.testing.assert_allclose(got["dispersions_norm"][6], 1.0, rtol=1e-12)            # (d - 0) / d
    first = d[1:3]
    np.testing.assert_allclose(got["dispersions_norm"][1:3], (first - first.mean()) / first.std(ddof=1), rtol=1e-12)
