"""The host side of prosstt_amd/hvg.py against the model (tests/hvg_model.py) and its refusals: the loess within
LOESS_TOL, the two flavours from sums formed with numpy, ``concat`` of the chunked sums, and every argument check that is
made before anything reaches a device.  No GPU."""
import numpy as np
import pytest

import hvg_model as M

torch = pytest.importorskip("torch")

from prosstt_amd import hvg, summary      # noqa: E402


def _summary(X):
    X64 = X.astype(np.int64)
    exact = X64.astype(object)                         # Python ints: a sum of squares can pass 64 bits
    return summary.CountSummary(X64.sum(axis=0), [int(v) for v in (exact * exact).sum(axis=0)], (X == 0).sum(axis=0),
                                X64.sum(axis=1), (X == 0).sum(axis=1))


def _clipped(X, thresholds):
    X64 = X.astype(np.int64)
    over = X64 > np.asarray(thresholds)[None, :]
    kept = np.where(over, 0, X64)
    kept_exact = kept.astype(object)                   # Python ints: a sum of squares can pass 64 bits
    return hvg.ClippedSums(X.shape[0], over.sum(axis=0), kept.sum(axis=0), [int(v) for v in (kept_exact * kept_exact).sum(axis=0)])


def _moments(X, sc):
    Y = M.normalized(X, sc)
    return hvg.NormalizedMoments(X.shape[0], Y.sum(axis=0), (Y * Y).sum(axis=0))


@pytest.mark.parametrize("which", ["small", "wide", "ties", "flat"])
def test_loess_fit_is_the_models_within_the_tolerance(which):
    if which in ("ties", "flat"):
        x, y = M.tie_heavy(which)
    else:
        mean, var = M.count_moments(M.inputs(which)[0])
        x, y = np.log10(mean), np.log10(var)
    got, want = hvg.loess_fit(x, y), M.loess(x, y)
    worst = M.within_loess_tol(got, want)
    print("loess_fit against the model, %s: %.3g" % (which, worst))
    assert worst <= M.LOESS_TOL


def test_loess_fit_small_and_singular_systems():
    x = np.repeat([0.0, 1.0, 3.0], 5)
    y = np.arange(15, dtype=np.float64) ** 1.5
    for span in (0.3, 0.5, 0.8, 1.0):
        np.testing.assert_allclose(hvg.loess_fit(x, y, span), M.loess(x, y, span), rtol=M.LOESS_TOL, atol=M.LOESS_TOL)
    for n in (1, 2, 3, 4):
        x, y = np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64) ** 2
        np.testing.assert_allclose(hvg.loess_fit(x, y), M.loess(x, y), rtol=M.LOESS_TOL, atol=M.LOESS_TOL)
    assert hvg.loess_fit([], []).shape == (0,)
    with pytest.raises(ValueError):
        hvg.loess_fit([1.0, 2.0], [1.0])
    with pytest.raises(ValueError):
        hvg.loess_fit([1.0, 2.0], [1.0, 2.0], span=0.0)


@pytest.mark.parametrize("which", ["small", "wide"])
def test_seurat_v3_from_numpy_sums_is_the_models(which):
    X, planted, n_top, _ = M.inputs(which)
    X = X.copy()
    X[:, 7] = 4                                        # a constant gene: reg_std 1, score 0
    want = M.seurat_v3(X, n_top)
    assert M.gap(want["variances_norm"], want["mask"]) > 1000 * M.LOESS_TOL
    cs = _summary(X)
    fit = hvg.seurat_v3_fit(cs)
    assert isinstance(fit, hvg.SeuratV3Fit) and fit.thresholds.dtype == np.int64 and fit.reg_std[7] == 1.0
    # reg_std = sqrt(10^fit): a relative error of ln(10) / 2 times the fit's absolute one
    np.testing.assert_allclose(fit.reg_std, want["reg_std"], rtol=1.2 * M.LOESS_TOL * max(1.0, np.abs(np.log10(want["var"][want["var"] > 0])).max()))
    np.testing.assert_array_equal(fit.thresholds, np.floor(fit.clip).astype(np.int64))
    hv = hvg.seurat_v3(cs, fit, _clipped(X, fit.thresholds), n_top)
    np.testing.assert_allclose(hv.means, want["mean"], rtol=1e-13)
    np.testing.assert_allclose(hv.variances, want["var"], rtol=1e-11)
    np.testing.assert_allclose(hv.variances_norm, want["variances_norm"], rtol=1e-9)
    assert hv.variances_norm[7] == 0.0
    np.testing.assert_array_equal(hv.highly_variable, want["mask"])
    np.testing.assert_array_equal(hv.genes, np.flatnonzero(want["mask"]))
    assert hv.flavor == "seurat_v3" and hv.dispersions is None and hv.dispersions_norm is None
    order = hv.genes[np.argsort(hv.rank[hv.genes])]
    assert np.array_equal(np.sort(hv.rank[hv.genes]), np.arange(n_top)) and np.all(np.isnan(hv.rank[~hv.highly_variable]))
    assert np.all(np.diff(hv.variances_norm[order]) <= 0)
    assert hv.highly_variable[planted].sum() >= len(planted) // 2


@pytest.mark.parametrize("which", ["small", "wide"])
def test_seurat_from_numpy_sums_is_the_models(which):
    X, planted, n_top, sc = M.inputs(which)
    X = X.copy()
    X[:, 7] = 0                                        # an absent gene: mean 1e-12, dispersion NaN
    nm = _moments(X, sc)
    want = M.seurat(nm.s1, nm.s2, nm.n_cells, n_top)
    hv = hvg.seurat(nm, n_top)
    np.testing.assert_allclose(hv.dispersions, want["dispersions"], rtol=1e-13, equal_nan=True)
    np.testing.assert_allclose(hv.dispersions_norm, want["dispersions_norm"], rtol=1e-11, atol=1e-12, equal_nan=True)
    assert np.isnan(hv.dispersions_norm[7]) and not hv.highly_variable[7]
    np.testing.assert_array_equal(hv.highly_variable, want["mask"])
    assert hv.flavor == "seurat" and hv.variances_norm is None and hv.highly_variable.sum() == n_top
    # the four cutoffs instead of a number
    for cut in (dict(), dict(min_mean=0.5, max_mean=2.0, min_disp=0.0, max_disp=2.0), dict(n_bins=7)):
        want = M.seurat(nm.s1, nm.s2, nm.n_cells, None, **cut)
        got = hvg.seurat(nm, None, **cut)
        np.testing.assert_array_equal(got.highly_variable, want["mask"])
        assert 0 < got.highly_variable.sum() < X.shape[1]
        assert np.array_equal(np.sort(got.rank[got.genes]), np.arange(len(got.genes)))


def test_seurat_with_equal_means_and_with_one_gene():
    # every mean equal: pd.cut widens the range by 0.1 % on either side, and so does the product
    n = 10
    for mean, var in ((np.full(4, 2.0), np.array([1.0, 2.0, 3.0, 0.0])), (np.array([0.5]), np.array([2.0]))):
        s1 = mean * n
        nm = hvg.NormalizedMoments(n, s1, var * (n - 1) + s1 * mean)
        want = M.seurat(nm.s1, nm.s2, n, 1, n_bins=5)
        got = hvg.seurat(nm, 1, n_bins=5)
        np.testing.assert_allclose(got.dispersions_norm, want["dispersions_norm"], rtol=1e-12, equal_nan=True)
        np.testing.assert_array_equal(got.highly_variable, want["mask"])


def test_top_goes_to_the_lower_index_on_ties_and_nan_is_last():
    score = np.array([1.0, np.nan, 3.0, 3.0, 1.0, np.nan])
    for n_top in range(1, 7):
        mask, genes, rank = hvg._top(score, n_top)
        np.testing.assert_array_equal(mask, M.top(score, n_top))
        assert genes.tolist() == np.flatnonzero(mask).tolist()
    assert hvg._top(score, 3)[2].tolist()[2:4] == [0.0, 1.0]


def test_concat_adds_the_parts():
    X, _, n_top, sc = M.inputs("small")
    X = X.copy()
    X[:40, :3] = 2 ** 31 - 2                           # sums of squares beyond 64 bits
    cs = _summary(X)
    fit = hvg.seurat_v3_fit(cs)
    thr = fit.thresholds.copy()
    thr[:3] = 2 ** 31 - 1, 2 ** 31 - 1, 5              # keeps the large entries of two of the three genes
    whole = _clipped(X, thr)
    parts = [_clipped(X[lo:hi], thr) for lo, hi in ((0, 1), (1, 200), (200, 500))]
    cat = hvg.ClippedSums.concat(parts)
    assert cat.n_cells == 500 and list(cat.sumsq_le) == list(whole.sumsq_le) and max(whole.sumsq_le) > 1 << 64
    np.testing.assert_array_equal(cat.n_over, whole.n_over)
    np.testing.assert_array_equal(cat.sum_le, whole.sum_le)
    assert cat.n_over[2] == 40 and cat.n_over[0] == 0
    np.testing.assert_array_equal(hvg.seurat_v3(cs, fit, cat, n_top).highly_variable,
                                  hvg.seurat_v3(cs, fit, whole, n_top).highly_variable)
    nm = [_moments(X[lo:hi], sc[lo:hi]) for lo, hi in ((0, 100), (100, 500))]
    both = hvg.NormalizedMoments.concat(nm)
    assert both.n_cells == 500
    np.testing.assert_array_equal(both.s1, nm[0].s1 + nm[1].s1)
    np.testing.assert_array_equal(both.s2, nm[0].s2 + nm[1].s2)
    for cls in (hvg.ClippedSums, hvg.NormalizedMoments):
        with pytest.raises(ValueError):
            cls.concat([])
    with pytest.raises(TypeError):
        hvg.ClippedSums.concat(nm)
    with pytest.raises(ValueError):
        hvg.NormalizedMoments.concat([nm[0], hvg.NormalizedMoments(5, np.zeros(3), np.zeros(3))])
    with pytest.raises(ValueError):
        hvg.ClippedSums(5, np.zeros(3), np.zeros(2), [0, 0, 0])


def test_host_functions_refuse_bad_arguments():
    X, _, n_top, sc = M.inputs("small")
    cs = _summary(X)
    fit = hvg.seurat_v3_fit(cs)
    clipped = _clipped(X, fit.thresholds)
    nm = _moments(X, sc)
    for bad in (0, X.shape[1] + 1, 2.5, True, None):
        with pytest.raises(ValueError):
            hvg.seurat_v3(cs, fit, clipped, bad)
    for bad in (0, X.shape[1] + 1, 2.5, True):
        with pytest.raises(ValueError):
            hvg.seurat(nm, bad)
    with pytest.raises(ValueError):
        hvg.seurat(nm, 5, n_bins=0)
    with pytest.raises(TypeError):
        hvg.seurat(clipped, 5)
    with pytest.raises(TypeError):
        hvg.seurat_v3_fit(nm)
    with pytest.raises(TypeError):
        hvg.seurat_v3(cs, (fit.reg_std, fit.clip, fit.thresholds), clipped, 5)
    with pytest.raises(TypeError):
        hvg.seurat_v3(cs, fit, nm, 5)
    with pytest.raises(ValueError):
        hvg.seurat_v3(cs, fit, _clipped(X[:100], fit.thresholds), 5)          # other cells
    with pytest.raises(ValueError):
        hvg.seurat_v3_fit(_summary(X[:1]))                                    # one cell has no variance
    with pytest.raises(ValueError):
        hvg.seurat(hvg.NormalizedMoments(1, nm.s1, nm.s2), 5)


def test_thresholds_and_gene_selections_are_checked_on_the_host():
    assert hvg._thresholds([0, 5, 2 ** 31 - 1], 3).dtype == np.int32
    for bad in ([0, -1, 3], [0, 1, 2 ** 31], [0, 1]):
        with pytest.raises(ValueError):
            hvg._thresholds(bad, 3)
    with pytest.raises(TypeError):
        hvg._thresholds([0.5, 1.0, 2.0], 3)
    assert hvg._gene_indices(np.array([True, False, True, True]), 4).tolist() == [0, 2, 3]
    assert hvg._gene_indices([3, 0, 0], 4).tolist() == [3, 0, 0]
    assert hvg._gene_indices(torch.tensor([2, 1]), 4).dtype == np.int32
    for bad in ([4], [-1], [], np.zeros(4, dtype=bool), np.ones(3, dtype=bool), [[0, 1]]):
        with pytest.raises(ValueError):
            hvg._gene_indices(bad, 4)
    with pytest.raises(TypeError):
        hvg._gene_indices([0.0, 1.0], 4)


def test_entry_points_refuse_what_is_not_a_device_count_matrix():
    X, _, n_top, sc = M.inputs("small")
    T = torch.as_tensor(X)
    thr = np.zeros(X.shape[1], dtype=np.int64)
    calls = (lambda a: hvg.highly_variable_genes(a, n_top_genes=n_top),
             lambda a: hvg.highly_variable_genes(a, sc, n_top, "seurat"),
             lambda a: hvg.clipped_sums(a, thr), lambda a: hvg.normalized_moments(a, sc),
             lambda a: hvg.select_genes(a, [0, 1]))
    for call in calls:
        with pytest.raises(TypeError):
            call(X)                                    # a host array: there is no CPU path
        with pytest.raises(TypeError):
            call(T.to(torch.int64))
        with pytest.raises(ValueError):
            call(T)                                    # a CPU tensor
        with pytest.raises(ValueError):
            call(T[0])                                 # one dimension
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T, flavor="cell_ranger")
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T[:1], n_top_genes=5)                       # fewer than two cells
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T, n_top_genes=0)
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T, n_top_genes=X.shape[1] + 1)
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T, n_top_genes=None)                        # cutoffs are the seurat flavour's
    with pytest.raises(ValueError, match="size_factors"):
        hvg.highly_variable_genes(T, None, n_top, "seurat")
    with pytest.raises(ValueError):
        hvg.highly_variable_genes(T, sc[:-1], n_top, "seurat")
