"""-m gpu: rows whose offsets do not fit in 32 bits.  Every library that reads a matrix in place takes a row stride and
promises 64-bit offsets; here each reads a small matrix whose rows lie 2^24 + 4 (16-byte loads) or 2^24 + 3 (4-byte loads,
the base one element off) elements apart, so that rows from 64 on start beyond byte 2^32 and rows 128 to 160 beyond element
2^31, and knn a panel with rows 2^20 + 4 or 2^20 + 3 floats apart (rows from 2048 on beyond element 2^31).

One device buffer of 19 GiB, allocated once: 8 GiB of guard, then the view's base.  A truncated offset (a byte offset kept
in 32 bits, signed or unsigned, or an element index kept in a signed 32 bits: at most 8 GiB either way) still lands inside
the buffer, on another row's entries or on the fill, 0xFF before every case: -1 counts, which every count library reports
as NEGATIVE, and NaN coordinates.  So an offset bug is a failed assertion, never a fault.

For each count library and both strides: (a) the far result has the bytes of the same call on a near view of the same
alignment class (the same host matrix, row stride G + 3 with the base on 16 bytes, or G + 4 with the base one element off;
blocking depends on (N, G) alone); (b) the near result meets the library's own criterion against its model, imported from
the library's GPU test module.  The bounds of embed's products and moments and of hvg's normalised moments are written
inline in those modules, so they are written again here, as they stand there.  knn is compared bit for bit with
knn_model.model.

The address arithmetic that reads the matrix, as audited in the sources (every product with ld, N or G; all are 64-bit):

  stats     count_summary_kernel   X + (row + k) * ld, rp[g]: row int64_t, ld int64_t, g = strip * 1024 + ... int64_t
                                   s.rows[strip * N + rr + tid]: int64_t; slabs at (size_t)blockIdx.y * (size_t)G
  embed     embed_moments_kernel   X + r * ld: r int64_t from (int64_t)blockIdx.y * rows_per_block
            embed_matmul_kernel    X + (row_ok ? r : 0) * ld: r = (int64_t)blockIdx.x * kRowsMM + ...; out[row * LP + ..]
                                   int64_t row; slab + (size_t)blockIdx.y * (size_t)N * LP
            load_cols2 (rmatmul)   X + (i + s) * ld + gw: i, ld, gw int64_t
  hvg       hvg_clipped_kernel     X + r * ld: int64_t; slabs at (size_t)blockIdx.y * (size_t)G + g
            hvg_moments_kernel     X + r * ld: int64_t; s1slab[k * G + g]: int64_t k, G, g
            hvg_gather_kernel      src[(r + k) * ld], dst[(r + k) * ldy]: r int64_t, k int
  markers   sum_rows               X + r[u] * ld, X + r * ld: int64_t r widened from the int32 row list
  ranks     ranks_emit_kernel      X + row * ld: row = (int64_t)rows[q0 + r + u]
  fit       fit_loglik_kernel      X + r0 * ld + g, xtile + (int64_t)(rt + tr) * ld, xcol[(int64_t)r * ld]: r0 int64_t,
                                   rt, tr, r int cast before the product; mcol[(int64_t)k * ldm]
  autocorr  sums and smooth        A.X + r * A.ld, A.X + r[u] * A.ld: r int64_t (row_of), A.ld int64_t
  knn       load8                  P + row * ld: row, ld int64_t; slab + (qt * 64 + 4 ty) * np + ..: qt int64_t;
                                   index[i * k + r]: i int64_t
  all       the wrappers           ld = X.stride(0), passed as c_int64 (every ld of prosstt_amd/_native.py is i64)

No 32-bit product was found in the audit, and none by the run."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GIB = 1 << 30
GUARD = 8 * GIB
TOTAL = 19 * GIB
N, G = 161, 1029                  # rows 128 .. 160 start beyond element 2^31; one whole strip of 1024 genes and a remainder
# path: (far row stride, near row stride, column shift)
PATHS = {"vector": ((1 << 24) + 4, G + 3, 0), "scalar": ((1 << 24) + 3, G + 4, 1)}
KNN = dict(N=2200, d=33, k=17, chunk=700)
KNN_PATHS = {"vector": ((1 << 20) + 4, 0), "scalar": ((1 << 20) + 3, 1)}
FILL = 12345                      # the padding of the near tensor: a read past the view shows in every sum


@pytest.fixture(scope="module")
def arena():
    """The 19 GiB device buffer as uint8; freed at teardown."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 24 * GIB:
        pytest.skip("%.1f GiB of device memory are free, the far-offset buffer needs 24" % (free / GIB))
    holder = [torch.empty(TOTAL, dtype=torch.uint8, device="cuda")]
    assert holder[0].data_ptr() % 16 == 0
    yield holder[0]
    holder.clear()
    del holder
    torch.cuda.empty_cache()


def _far(arena, host, stride, shift):
    """``host`` (rows, cols) written into the poisoned arena behind the guard: the view with rows ``stride`` elements apart
    whose first element lies ``shift`` elements behind the base."""
    import torch
    arena.fill_(0xFF)
    rows, cols = host.shape
    dtype = torch.int32 if host.dtype == np.int32 else torch.float32
    flat = arena[GUARD:].view(dtype)
    assert flat.data_ptr() % 16 == 0 and (rows - 1) * stride + cols + shift <= flat.numel()
    view = torch.as_strided(flat, (rows, cols), (stride, 1), flat.storage_offset() + shift)
    view.copy_(torch.from_numpy(np.array(host)).cuda())          # (a copy: the shared arrays are read-only)
    assert view.stride() == (stride, 1) and view.data_ptr() == flat.data_ptr() + 4 * shift
    assert (rows - 1) * stride * 4 >= 1 << 33 and (rows - 1) * stride >= 1 << 31          # bytes and elements past 32 bits
    return view


def _near(host, stride, shift):
    import torch
    rows, cols = host.shape
    wide = torch.full((rows, stride), FILL, dtype=torch.int32, device="cuda")
    wide[:, shift:shift + cols] = torch.from_numpy(np.array(host)).cuda()
    view = wide[:, shift:shift + cols]
    assert view.data_ptr() % 16 == 4 * shift and view.stride() == (stride, 1)
    return view


@functools.lru_cache(maxsize=None)
def _inputs():
    """The host matrix (test_gpu_fit._matrix's "big" values: INT_MAX among them), size factors, labels of three and of seven
    groups with cells of every group among rows 128 to 160 and a few cells left out, and fit's means and candidates."""
    import test_gpu_fit as tf
    rng = np.random.default_rng(161 * 1029)
    X = np.ascontiguousarray(tf._matrix(N, G, 0, "big", 0, rng)[0])
    assert X.shape == (N, G) and X.dtype == np.int32 and X.max() == tf.INT_MAX and X.min() == 0
    s = rng.lognormal(0.0, 0.7, size=N)
    labels = {K: (np.arange(N) * 5 + 1) % K for K in (3, 7)}
    for K, lab in labels.items():
        lab[[3, 70, 129]] = -1
        assert set(lab[128:]) == set(range(K)) | {-1}
    sc, _, means, alpha, beta = tf._inputs(N, G, 7, 9, rng)
    X.setflags(write=False)
    return dict(X=X, s=s, labels=labels, fit=(sc, labels[7], means, alpha, beta))


@pytest.fixture(params=sorted(PATHS))
def views(request, arena):
    """(far view, near view) of the shared matrix for one alignment class."""
    far_stride, near_stride, shift = PATHS[request.param]
    X = _inputs()["X"]
    far = _far(arena, X, far_stride, shift)
    near = _near(X, near_stride, shift)
    assert (far.data_ptr() % 16 == 0 and far_stride % 4 == 0 and near_stride % 4 == 0) == (request.param == "vector")
    assert (far.data_ptr() % 16 == 4 and far_stride % 2 == 1 and near_stride % 2 == 1) == (request.param == "scalar")
    return far, near


def _same_bytes(far, near, what):
    from test_gpu_stale_memory import _flatten
    a, b = _flatten(far), _flatten(near)
    assert sorted(a) == sorted(b) and len(a) > 0, what
    for path in a:
        assert a[path] == b[path], "%s: %s of the far view differs from the near view's" % (what, path)


_cache = {}


def _a32(near):
    """The device's own float32 entries of the matrix (test_gpu_markers._a32's selection panels), as a host array."""
    import torch
    from prosstt_amd import embed
    if "a32" not in _cache:
        op = embed.LogNormalized(near, _inputs()["s"])
        out = torch.empty(N, G, dtype=torch.float32, device="cuda")
        for g0 in range(0, G, 128):
            w = min(128, G - g0)
            P = torch.zeros(G, w, dtype=torch.float32, device="cuda")
            P[g0 + torch.arange(w, device="cuda"), torch.arange(w, device="cuda")] = 1.0
            out[:, g0:g0 + w] = op.matmul(P)
        _cache["a32"] = out.cpu().numpy()
    return _cache["a32"]


# ------------------------------------------------------------------------------------------------------ count matrices

def test_count_summary(views):
    import test_gpu_count_summary as tc
    from prosstt_amd import summary
    far, near = views
    got = summary.count_summary(near)
    tc._assert_exact(got, tc._host_reference(_inputs()["X"]))
    _same_bytes(summary.count_summary(far), got, "count_summary")


def test_log_normalized_moments_and_products(views):
    import torch
    import test_gpu_embed as te
    from prosstt_amd import embed
    far, near = views
    X, s = _inputs()["X"], _inputs()["s"]
    rng = np.random.default_rng(33)
    W = rng.standard_normal((G, 33)).astype(np.float32)
    Q = rng.standard_normal((N, 33)).astype(np.float32)
    Wd, Qd = torch.as_tensor(W).cuda(), torch.as_tensor(Q).cuda()
    results = []
    for view in (near, far):
        op = embed.LogNormalized(view, s)
        results.append((op.matmul(Wd), op.rmatmul(Qd), op.gene_moments()))
    Y, Z, (S1, S2) = results[0]
    A = np.log1p(X.astype(np.int64) / s[:, None])
    te._assert_product(Y.cpu().numpy(), A, W, "matmul")
    te._assert_product(Z.cpu().numpy(), A.T, Q, "rmatmul")
    R1, R2 = A.sum(axis=0), (A * A).sum(axis=0)
    assert np.all(np.abs(S1 - R1) <= 2.0 ** -19 * R1) and np.all(np.abs(S2 - R2) <= 2.0 ** -18 * R2)     # test_gpu_embed's
    _same_bytes(results[1], results[0], "LogNormalized")


def test_hvg_clipped_sums(views):
    import test_gpu_hvg as th
    from prosstt_amd import hvg
    far, near = views
    X = _inputs()["X"]
    thr = th._thresholds(np.random.default_rng(7), X)
    got = hvg.clipped_sums(near, thr)
    n_over, sum_le, sumsq_le = th._clipped_reference(X, thr)
    np.testing.assert_array_equal(got.n_over, n_over)
    np.testing.assert_array_equal(got.sum_le, sum_le)
    assert list(got.sumsq_le) == sumsq_le and max(sumsq_le) >= 1 << 64
    _same_bytes(hvg.clipped_sums(far, thr), got, "clipped_sums")


def test_hvg_normalized_moments(views):
    import hvg_model
    import test_gpu_hvg as th
    from prosstt_amd import hvg
    far, near = views
    X, s = _inputs()["X"], _inputs()["s"]
    got = hvg.normalized_moments(near, s)
    Y = hvg_model.normalized(X, s)
    np.testing.assert_allclose(got.s1, th._fsum_columns(Y), rtol=N * 2.0 ** -52)                      # test_gpu_hvg's
    np.testing.assert_allclose(got.s2, th._fsum_columns(Y * Y), rtol=N * 2.0 ** -52)
    _same_bytes(hvg.normalized_moments(far, s), got, "normalized_moments")


def test_hvg_select_genes(views):
    import test_gpu_hvg as th
    from prosstt_amd import hvg
    far, near = views
    X = _inputs()["X"]
    for kind, n_sel in (("permutation", 257), ("repeats", 1025), ("sorted", 5)):
        idx = th._selection(kind, n_sel, np.random.default_rng(n_sel), G)
        got = hvg.select_genes(near, idx)
        np.testing.assert_array_equal(got.cpu().numpy(), X[:, idx])
        _same_bytes(hvg.select_genes(far, idx), got, "select_genes " + kind)


def test_markers_group_moments(views):
    import markers_model as mm
    import test_gpu_markers as tm
    from prosstt_amd import markers
    far, near = views
    X, s, labels = _inputs()["X"], _inputs()["s"], _inputs()["labels"][3]
    nz, cs = tm._integers(X, labels, 3)
    for rpb in (0, 64):
        got = markers.group_moments(near, s, labels, rows_per_block=rpb)
        assert np.array_equal(got.nonzero, nz) and np.array_equal(got.count_sum, cs)
        S1, S2, _ = mm.sums(_a32(near), labels, rpb or mm.default_rows_per_block(int((labels >= 0).sum()), G), 3)
        assert tm._same_bits(got.s1, S1) and tm._same_bits(got.s2, S2), rpb
        _same_bytes(markers.group_moments(far, s, labels, rows_per_block=rpb), got, "group_moments")


def test_ranks_rank_sums(views):
    import ranks_model as rm
    import test_gpu_ranks as tr
    from prosstt_amd import ranks
    far, near = views
    s, labels = _inputs()["s"], _inputs()["labels"][3]
    if "ranks" not in _cache:
        _cache["ranks"] = rm.rank_sums(_a32(near), labels, 3, reference=None)
    got = ranks.rank_sums(near, s, labels)
    tr._check(got, _cache["ranks"], 3)
    _same_bytes(ranks.rank_sums(far, s, labels), got, "rank_sums")
    _same_bytes(ranks.rank_sums(far, s, labels, genes_per_pass=1024), got, "rank_sums in two passes")


def test_fit_loglik(views):
    import fit_model
    import test_gpu_fit as tf
    from prosstt_amd import fit
    far, near = views
    args = _inputs()["fit"]
    if "fit" not in _cache:
        _cache["fit"] = fit_model.loglik(_inputs()["X"], *args)
    got = fit.loglik(near, *args)
    r_ll, r_base = tf._ratios(got, _cache["fit"])
    print("fit ratio on the near view: ll %.3g base %.3g" % (r_ll, r_base))
    assert r_ll <= tf.EPS and r_base <= tf.EPS and _cache["fit"][2].sum() > 0
    _same_bytes(fit.loglik(far, *args), got, "loglik")


def test_autocorr_graph_sums_and_smooth(views):
    import autocorr_model as am
    import test_gpu_autocorr as ta
    from prosstt_amd import autocorr
    far, near = views
    s = _inputs()["s"]
    csr = ta._hand_graph(N)                                       # a hub of all other cells, an empty row, a self-loop
    g = ta._as_graph(csr)
    got = autocorr.graph_sums(near, s, g)
    ta._check(got, am.sums(_a32(near), *csr, got.mean, am.default_rows_per_block(N)), "the near view")
    _same_bytes(autocorr.graph_sums(far, s, g), got, "graph_sums")
    for tile in ta.TILES:
        tiled = autocorr.graph_sums(near, s, g, rows_per_block=64, gene_tile=tile, mean=got.mean)
        ta._check(tiled, am.sums(_a32(near), *csr, got.mean, 64), tile)
        _same_bytes(autocorr.graph_sums(far, s, g, rows_per_block=64, gene_tile=tile, mean=got.mean), tiled, "graph_sums, tiled")
        for normalize in (True, False):
            if ("smooth", normalize) not in _cache:
                _cache["smooth", normalize] = am.smooth(_a32(near), *csr, normalize)
            panel = autocorr.smooth(near, s, g, normalize=normalize, gene_tile=tile)
            assert ta._bits32(panel.cpu().numpy(), _cache["smooth", normalize]), (tile, normalize)
            _same_bytes(autocorr.smooth(far, s, g, normalize=normalize, gene_tile=tile), panel, "smooth")


# ----------------------------------------------------------------------------------------------------------------- knn

@functools.lru_cache(maxsize=None)
def _knn_case():
    import knn_model
    P = knn_model.gaussian(KNN["N"], KNN["d"], 2200 * 33)
    assert knn_model.no_subnormal_terms(P)
    return (P,) + knn_model.model(P, KNN["k"])


@pytest.mark.parametrize("path", sorted(KNN_PATHS))
def test_knn(arena, path):
    from prosstt_amd import neighbors
    stride, shift = KNN_PATHS[path]
    P, want_idx, want_d2 = _knn_case()
    far = _far(arena, P, stride, shift)
    assert 2048 * stride >= 1 << 31
    got = neighbors.knn(far, KNN["k"], chunk_rows=KNN["chunk"])
    np.testing.assert_array_equal(got.indices, want_idx)
    np.testing.assert_array_equal(got.sq_distances.view(np.uint32), want_d2.view(np.uint32))
