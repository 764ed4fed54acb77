"""-m gpu: prosstt_amd/hvg.py and libprosstt_amd_hvg.so against exact host references: the clipped sums equal numpy's
integers on ragged shapes, strided and unaligned views, and values that carry the 128-bit sum of squares; the normalised
moments equal math.fsum of the same float32 products; the gathered columns equal numpy's; and whole calls of both flavours
select the model's genes (tests/hvg_model.py), stage by stage."""
import ctypes
import functools
import math

import numpy as np
import pytest

import hvg_model as M

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------------ clipped sums

def _clipped_reference(X, thr):
    """Exact (n_over, sum_le, sumsq_le) of an int matrix (numpy, no Python-int loop over entries): the sum of squares
    through x = h * 2^16 + l, each partial sum below 2^45 for N < 2^13."""
    X = np.asarray(X, dtype=np.int64)
    over = X > np.asarray(thr, dtype=np.int64)[None, :]
    kept = np.where(over, 0, X)
    h, lo = kept >> 16, kept & 0xFFFF
    a, b, c = (h * h).sum(axis=0), (h * lo).sum(axis=0), (lo * lo).sum(axis=0)
    return over.sum(axis=0), kept.sum(axis=0), [(int(x) << 32) + (int(y) << 17) + int(z) for x, y, z in zip(a, b, c)]


def _thresholds(rng, X):
    """One threshold per gene, by turns: 0, a value of the column, that value - 1, 2^31 - 1, a random value."""
    N, G = X.shape
    present = X[rng.integers(0, N, size=G), np.arange(G)].astype(np.int64)
    kinds = np.stack([np.zeros(G, dtype=np.int64), present, np.maximum(present - 1, 0), np.full(G, INT_MAX),
                      rng.integers(0, min(max(2, int(X.max()) + 2), INT_MAX + 1), size=G)])
    return kinds[rng.permutation(G) % 5, np.arange(G)]


NS = [1, 2, 63, 64, 65, 1000, 4097]
GS = [1, 3, 4, 5, 1023, 1024, 1025, 5003]
PADS = [0, 1, 3, 64]
KINDS = ["zeros", "nb", "big"]
CASES = [(NS[i % 7], GS[(3 * i + i // 7) % 8], PADS[(i // 2) % 4], KINDS[i % 3], (i // 5) % 2) for i in range(40)]


def _view(N, G, pad, kind, shift, rng):
    """(host matrix, device view of it): G columns from column ``shift`` of a tensor of row stride G + pad."""
    import torch
    shift = shift if pad > 0 else 0                   # a base that is not 16-byte aligned needs room in the row
    width = G + pad
    if kind == "zeros":
        W = np.zeros((N, width), dtype=np.int32)
    elif kind == "nb":
        W = rng.negative_binomial(0.5, 0.4, size=(N, width)).astype(np.int32)
    else:
        W = (INT_MAX - rng.integers(0, 3, size=(N, width))).astype(np.int32)
        W[rng.random((N, width)) < 0.1] = 0
    D = torch.as_tensor(W).cuda()
    view = D[:, shift:shift + G]
    assert view.stride() == ((width, 1) if N > 1 else view.stride())
    return W[:, shift:shift + G], view


@pytest.mark.parametrize("N,G,pad,kind,shift", CASES)
def test_clipped_sums_shapes_strides_values_and_thresholds(N, G, pad, kind, shift):
    from prosstt_amd import hvg
    rng = np.random.default_rng(N * 100003 + G * 7 + pad)
    X, view = _view(N, G, pad, kind, shift, rng)
    thr = _thresholds(rng, X)
    got = hvg.clipped_sums(view, thr)
    assert (got.n_cells, got.n_genes) == (N, G)
    n_over, sum_le, sumsq_le = _clipped_reference(X, thr)
    np.testing.assert_array_equal(got.n_over, n_over)
    np.testing.assert_array_equal(got.sum_le, sum_le)
    assert list(got.sumsq_le) == sumsq_le
    if kind == "big" and N >= 63 and G >= 1023:
        assert max(sumsq_le) >= 1 << 64               # the carry into the high word was exercised


def test_clipped_sums_add_up_to_count_summary_and_concat():
    import torch
    from prosstt_amd import hvg
    from prosstt_amd.summary import count_summary
    rng = np.random.default_rng(3)
    X = rng.negative_binomial(0.5, 0.1, size=(333, 1030)).astype(np.int32)
    D = torch.as_tensor(X).cuda()
    s = count_summary(D)
    everything = hvg.clipped_sums(D, np.full(1030, INT_MAX))
    np.testing.assert_array_equal(everything.sum_le, s.gene_sum)
    assert list(everything.sumsq_le) == list(s.gene_sumsq) and not everything.n_over.any()
    nothing = hvg.clipped_sums(D, np.zeros(1030, dtype=np.int64))
    np.testing.assert_array_equal(nothing.n_over, 333 - s.gene_zeros)
    assert not nothing.sum_le.any()
    thr = _thresholds(rng, X)
    parts = hvg.ClippedSums.concat([hvg.clipped_sums(D[lo:hi], thr) for lo, hi in ((0, 1), (1, 200), (200, 333))])
    whole = hvg.clipped_sums(D, thr)
    np.testing.assert_array_equal(parts.n_over, whole.n_over)
    np.testing.assert_array_equal(parts.sum_le, whole.sum_le)
    assert list(parts.sumsq_le) == list(whole.sumsq_le) and parts.n_cells == 333


def _raw(name, *args):
    from prosstt_amd import _native
    _native.check(getattr(_native.load("hvg"), name)(*args), "hvg")


def _workspace(N, G):
    import torch
    from prosstt_amd import _native
    need = ctypes.c_uint64(0)
    _native.check(_native.load("hvg").prosstt_amd_hvg_workspace_bytes(N, G, ctypes.byref(need)), "hvg")
    return torch.empty(int(need.value), dtype=torch.uint8, device="cuda")


def test_clipped_sums_refusals_and_status_bits():
    import torch
    from prosstt_amd import hvg, device
    from prosstt_amd.device import _ptr
    X = torch.ones((6, 10), dtype=torch.int32, device="cuda")
    thr = np.full(10, 3)
    bad = X.clone()
    bad[3, 7] = -1
    with pytest.raises(ValueError, match=device.NEGATIVE_ENTRY):
        hvg.clipped_sums(bad, thr)
    assert hvg.clipped_sums(X, thr).sum_le.tolist() == [6] * 10          # nothing left behind by the refused call
    negative = thr.copy()
    negative[4] = -1
    with pytest.raises(ValueError):
        hvg.clipped_sums(X, negative)
    with pytest.raises(ValueError):
        hvg.clipped_sums(X, thr[:9])
    with pytest.raises(ValueError):
        hvg.clipped_sums(X[:, ::2], thr[:5])
    with pytest.raises(ValueError):
        hvg.clipped_sums(X[:0], thr)
    # the library's own answer to a negative threshold: bit 1 of the status word, and only that bit
    ws = _workspace(6, 10)
    out = torch.zeros(40, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = torch.as_tensor(negative.astype(np.int32)).cuda()
    _raw("prosstt_amd_hvg_clipped_sums", None, _ptr(X), 6, 10, 10, _ptr(t), _ptr(ws), ws.numel(), _ptr(out[:10]),
         _ptr(out[10:20]), _ptr(out[20:]), _ptr(status))
    assert int(status.item()) == hvg.RANGE


# ------------------------------------------------------------------------------------------------ normalised moments

def _fsum_columns(Y):
    return np.array([math.fsum(col) for col in Y.T.tolist()])


@pytest.mark.parametrize("N,G,pad,shift", [(1, 5, 0, 0), (65, 1025, 3, 1), (1000, 1023, 0, 0), (4097, 5, 1, 1), (300, 1024, 64, 0)])
def test_normalized_moments_against_fsum(N, G, pad, shift):
    import torch
    from prosstt_amd import hvg
    rng = np.random.default_rng(N + G)
    X, view = _view(N, G, pad, "nb", shift, rng)
    X = X.copy()
    X[rng.integers(0, N, size=3), rng.integers(0, G, size=3)] = 2 ** 24 + 1 + rng.integers(0, 1000, size=3)
    view.copy_(torch.as_tensor(X))
    sc = rng.lognormal(0.0, 0.7, size=N)
    got = hvg.normalized_moments(view, sc)
    Y = M.normalized(X, sc)                            # numpy reproduces float32(x) * inv to the bit; Y * Y is exact
    # any order of summing N non-negative binary64 terms is within (N - 1) 2^-53 of exact
    np.testing.assert_allclose(got.s1, _fsum_columns(Y), rtol=N * 2.0 ** -52)
    np.testing.assert_allclose(got.s2, _fsum_columns(Y * Y), rtol=N * 2.0 ** -52)
    assert got.n_cells == N


def test_normalized_moments_with_unit_size_factors_are_the_integers():
    import torch
    from prosstt_amd import hvg
    from prosstt_amd.summary import count_summary
    rng = np.random.default_rng(11)
    X = rng.negative_binomial(0.5, 0.01, size=(1500, 1100)).astype(np.int32)     # counts < 2^24, sums of squares < 2^53
    D = torch.as_tensor(X).cuda()
    got = hvg.normalized_moments(D, np.ones(1500))
    s = count_summary(D)
    assert max(s.gene_sumsq) < 1 << 53
    np.testing.assert_array_equal(got.s1, s.gene_sum.astype(np.float64))
    np.testing.assert_array_equal(got.s2, np.array([float(v) for v in s.gene_sumsq]))


def test_normalized_moments_same_bits_again_on_a_second_stream_and_presented():
    import torch
    from prosstt_amd import hvg, device
    rng = np.random.default_rng(12)
    X = rng.negative_binomial(0.5, 0.1, size=(2100, 1030)).astype(np.int32)
    sc = rng.lognormal(0.0, 0.7, size=2100)
    D = torch.as_tensor(X).cuda()
    first = hvg.normalized_moments(D, sc)
    again = hvg.normalized_moments(D, sc)
    with torch.cuda.stream(torch.cuda.Stream()):
        other = hvg.normalized_moments(D, sc)
    for b in (again, other):
        assert first.s1.tobytes() == b.s1.tobytes() and first.s2.tobytes() == b.s2.tobytes()
    bad = D.clone()
    bad[5, 5] = -3
    with pytest.raises(ValueError, match=device.NEGATIVE_ENTRY):
        hvg.normalized_moments(bad, sc)
    parts = hvg.NormalizedMoments.concat([hvg.normalized_moments(D[:700], sc[:700]), hvg.normalized_moments(D[700:], sc[700:])])
    np.testing.assert_allclose(parts.s1, first.s1, rtol=2100 * 2.0 ** -52)
    np.testing.assert_allclose(parts.s2, first.s2, rtol=2100 * 2.0 ** -52)


# ---------------------------------------------------------------------------------------------------- gather columns

@functools.lru_cache(maxsize=None)
def _gather_matrix():
    import torch
    rng = np.random.default_rng(21)
    W = rng.integers(0, INT_MAX, size=(67, 1103), dtype=np.int64).astype(np.int32)
    D = torch.as_tensor(W).cuda()
    return W[:, 1:1101], D[:, 1:1101]                  # 1100 genes, row stride 1103, a base off 16 bytes


def _selection(kind, n_sel, rng, G=1100):
    if kind == "sorted":
        return np.sort(rng.choice(G, size=n_sel, replace=False))
    if kind == "permutation":
        return rng.permutation(G)[:n_sel]
    return rng.integers(0, max(1, n_sel // 3), size=n_sel)            # repeats


@pytest.mark.parametrize("kind", ["sorted", "permutation", "repeats"])
@pytest.mark.parametrize("n_sel", [1, 3, 4, 5, 255, 256, 257, 1025])
def test_select_genes_is_numpys_columns(kind, n_sel):
    from prosstt_amd import hvg
    X, view = _gather_matrix()
    idx = _selection(kind, n_sel, np.random.default_rng(n_sel))
    got = hvg.select_genes(view, idx)
    assert got.shape == (67, n_sel) and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), X[:, idx])
    if kind == "sorted":
        mask = np.zeros(1100, dtype=bool)
        mask[idx] = True
        np.testing.assert_array_equal(hvg.select_genes(view, mask).cpu().numpy(), X[:, idx])


def test_select_genes_all_columns_many_rows_and_presented():
    import torch
    from prosstt_amd import hvg, device
    X, view = _gather_matrix()
    np.testing.assert_array_equal(hvg.select_genes(view, np.ones(1100, dtype=bool)).cpu().numpy(), X)
    rng = np.random.default_rng(22)
    tall = rng.integers(0, 1000, size=(4097, 37)).astype(np.int32)
    D = torch.as_tensor(tall).cuda()
    np.testing.assert_array_equal(hvg.select_genes(D, [36, 0, 5]).cpu().numpy(), tall[:, [36, 0, 5]])
    perm = rng.permutation(4097)
    got = hvg.select_genes(device.PresentedCounts(D, perm), [36, 0, 5])
    assert isinstance(got, device.PresentedCounts) and np.array_equal(got.cell_of_row, perm)
    np.testing.assert_array_equal(got.counts.cpu().numpy(), tall[:, [36, 0, 5]])
    for bad in ([37], [-1], [], np.zeros(37, dtype=bool)):
        with pytest.raises(ValueError):
            hvg.select_genes(D, bad)


def test_gather_columns_wider_output_rows_and_a_column_outside_the_matrix():
    import torch
    from prosstt_amd import hvg
    from prosstt_amd.device import _ptr
    X, view = _gather_matrix()
    cols = np.array([5, 1099, 1100, 0, -1, 7, 2 ** 31 - 1, 5], dtype=np.int32)
    valid = (cols >= 0) & (cols < 1100)
    Y = torch.full((67, 11), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    c = torch.as_tensor(cols).cuda()
    _raw("prosstt_amd_hvg_gather_columns", None, _ptr(view), 67, 1100, 1103, _ptr(c), 8, _ptr(Y), 11, _ptr(status))
    got = Y.cpu().numpy()
    assert int(status.item()) == hvg.RANGE
    np.testing.assert_array_equal(got[:, :8][:, valid], X[:, cols[valid]])
    assert not got[:, :8][:, ~valid].any()             # 0 in place of a column outside the matrix
    assert (got[:, 8:] == -7).all()                    # ldy > n_sel: the rest of the row is not touched
    status.zero_()
    _raw("prosstt_amd_hvg_gather_columns", None, _ptr(view), 67, 1100, 1103, _ptr(c[:2]), 2, _ptr(Y), 11, _ptr(status))
    assert int(status.item()) == 0                     # status is only ever set


# ------------------------------------------------------------------------------------------------------- whole calls

@functools.lru_cache(maxsize=None)
def _case(which):
    """The inputs of a whole call and the model's results on them, computed once."""
    X, planted, n_top, sc = M.inputs(which)
    v3 = M.seurat_v3(X, n_top)
    Y = M.normalized(X, sc)
    se = M.seurat(Y.sum(axis=0), (Y * Y).sum(axis=0), X.shape[0], n_top)
    return X, planted, n_top, sc, v3, se


@pytest.mark.parametrize("which", ["small", "wide"])
def test_seurat_v3_selects_the_models_genes_stage_by_stage(which):
    import torch
    from prosstt_amd import hvg
    from prosstt_amd.summary import count_summary
    X, planted, n_top, sc, want, _ = _case(which)
    N = X.shape[0]
    assert M.gap(want["variances_norm"], want["mask"]) > 1000 * M.LOESS_TOL
    D = torch.as_tensor(X).cuda()
    # stage 1: the moments from the exact sums
    cs = count_summary(D)
    fit = hvg.seurat_v3_fit(cs, device=D.device)
    # stage 2: the loess, its weighted sums on the device
    v = want["var"] > 0
    fitted = hvg.loess_fit(np.log10(want["mean"][v]), np.log10(want["var"][v]), device=D.device)
    worst = M.within_loess_tol(fitted, 2.0 * np.log10(want["reg_std"][v]))
    print("loess_fit on the device against the model, %s: %.3g" % (which, worst))
    assert worst <= M.LOESS_TOL
    np.testing.assert_array_equal(fit.thresholds, np.floor(want["clip"]).astype(np.int64))
    # stage 3: the clipped sums for these thresholds, exactly
    clipped = hvg.clipped_sums(D, fit.thresholds)
    n_over, sum_le, sumsq_le = _clipped_reference(X, fit.thresholds)
    np.testing.assert_array_equal(clipped.n_over, n_over)
    np.testing.assert_array_equal(clipped.sum_le, sum_le)
    assert list(clipped.sumsq_le) == sumsq_le
    # stage 4: the model fed with the device's sums gives the mask of the model alone, and the product's
    sum_c = clipped.sum_le + clipped.n_over * want["clip"]
    sq_c = np.array([float(s) for s in clipped.sumsq_le]) + clipped.n_over * want["clip"] ** 2
    fed = M.variances_norm(N, want["mean"], want["var"], want["reg_std"], sum_c, sq_c)
    np.testing.assert_array_equal(M.top(fed, n_top), want["mask"])
    hv = hvg.highly_variable_genes(D, n_top_genes=n_top)
    np.testing.assert_array_equal(hv.highly_variable, want["mask"])
    np.testing.assert_array_equal(hv.genes, np.flatnonzero(want["mask"]))
    np.testing.assert_allclose(hv.variances_norm, want["variances_norm"], rtol=1e-9)
    np.testing.assert_allclose(hv.means, want["mean"], rtol=1e-14)
    assert hv.flavor == "seurat_v3" and hv.highly_variable[planted].sum() >= len(planted) // 2


@pytest.mark.parametrize("which", ["small", "wide"])
def test_seurat_selects_the_models_genes_stage_by_stage(which):
    import torch
    from prosstt_amd import hvg
    X, planted, n_top, sc, _, want = _case(which)
    N = X.shape[0]
    score = np.where(np.isnan(want["dispersions_norm"]), -np.inf, want["dispersions_norm"])
    assert M.gap(score, want["mask"]) > 1000 * M.LOESS_TOL
    D = torch.as_tensor(X).cuda()
    nm = hvg.normalized_moments(D, sc)
    Y = M.normalized(X, sc)
    np.testing.assert_allclose(nm.s1, Y.sum(axis=0), rtol=N * 2.0 ** -52)
    np.testing.assert_allclose(nm.s2, (Y * Y).sum(axis=0), rtol=N * 2.0 ** -52)
    fed = M.seurat(nm.s1, nm.s2, N, n_top)
    np.testing.assert_array_equal(fed["mask"], want["mask"])
    hv = hvg.highly_variable_genes(D, sc, n_top, "seurat")
    np.testing.assert_array_equal(hv.highly_variable, want["mask"])
    np.testing.assert_allclose(hv.dispersions_norm, fed["dispersions_norm"], rtol=1e-11, atol=1e-12, equal_nan=True)
    cut = hvg.highly_variable_genes(D, sc, None, "seurat", min_disp=0.25)
    np.testing.assert_array_equal(cut.highly_variable, M.seurat(nm.s1, nm.s2, N, None, min_disp=0.25)["mask"])
    assert hv.flavor == "seurat" and 0 < cut.highly_variable.sum() < X.shape[1]


def test_single_cell_outliers_are_clipped():
    import torch
    from prosstt_amd import hvg
    X, planted, n_top, _ = M.inputs("small")
    X = X.copy()
    rng = np.random.default_rng(31)
    quiet = np.setdiff1d(np.arange(X.shape[1]), planted)[:6]
    X[rng.integers(0, X.shape[0], size=6), quiet] = 10 ** 4               # one cell each
    clipped, unclipped = M.seurat_v3(X, n_top), M.seurat_v3(X, n_top, clip=False)
    # without the clip one cell's 10^4 counts carry a gene into the selection; with it none of the six is selected
    assert unclipped["mask"][quiet].sum() >= 3 and not clipped["mask"][quiet].any()
    assert not np.array_equal(clipped["mask"], unclipped["mask"])
    assert M.gap(clipped["variances_norm"], clipped["mask"]) > 1000 * M.LOESS_TOL
    D = torch.as_tensor(X).cuda()
    hv = hvg.highly_variable_genes(D, n_top_genes=n_top)
    np.testing.assert_array_equal(hv.highly_variable, clipped["mask"])
    over = hvg.clipped_sums(D, np.floor(clipped["clip"]).astype(np.int64)).n_over
    assert (over[quiet] >= 1).all()                    # the outliers were above their genes' thresholds


def test_presented_counts_give_the_plan_order_result():
    import torch
    from prosstt_amd import hvg, device
    X, _, n_top, sc, v3, se = _case("wide")
    perm = np.random.default_rng(41).permutation(X.shape[0])
    presented = device.PresentedCounts(torch.as_tensor(X[perm]).cuda(), perm)      # row i is cell perm[i]
    a = hvg.highly_variable_genes(presented, n_top_genes=n_top)
    np.testing.assert_array_equal(a.highly_variable, v3["mask"])
    b = hvg.highly_variable_genes(presented, sc, n_top, "seurat")
    np.testing.assert_array_equal(b.highly_variable, se["mask"])
    plain = hvg.highly_variable_genes(torch.as_tensor(X).cuda(), n_top_genes=n_top)
    assert a.variances_norm.tobytes() == plain.variances_norm.tobytes()             # exact sums: no order in them


def test_pca_of_the_selected_genes_has_the_bits_of_the_sliced_matrix():
    import torch
    from prosstt_amd import hvg, embed
    X, _, n_top, sc, v3, _ = _case("small")
    D = torch.as_tensor(X).cuda()
    idx = np.flatnonzero(v3["mask"])
    a = embed.pca(hvg.select_genes(D, idx), sc, n_components=5)
    b = embed.pca(D[:, torch.as_tensor(idx).cuda()].contiguous(), sc, n_components=5)
    for f in a._fields:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
