"""-m gpu: the pass of libprosstt_amd_autocorr.so (prosstt_amd/csrc/autocorr/autocorr.hip) and prosstt_amd.autocorr on top
of it.

The four sums per gene and the smoothed panel are compared BIT FOR BIT with tests/autocorr_model.py, which takes the
device's own float32 entries log1p(x * inv_size) (``test_gpu_markers._a32``: embed's selection panels) and the mean the call
centred with, and repeats the kernel's operations one rounding at a time in the kernel's order.  So equal bits here also
prove that the pass forms embed's entries.  The matrices are test_gpu_markers' draws (two thirds zeros, a few counts up to
2^31) in its two views: "aligned", and "shifted" (odd row stride, base 4 bytes past 16-byte alignment, filled padding)."""
import ctypes

import numpy as np
import pytest

import autocorr_model as am
from test_autocorr_model import planted_case
from test_gpu_markers import VIEWS, _a32, _host, _same_bits, _view

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 63), (63, 64), (64, 65), (65, 257), (130, 300), (300, 130)]
ROWS_PER_BLOCK = [0, 1, 64, 100]
TILES = [64, 256]
GRAPHS = ["knn", "hand"]
# (neighbors.knn does not define the 4 nearest other cells of fewer than five: (1, 1) runs on the hand-made graph alone)
CASES = [(N, G, kind) for N, G in SHAPES for kind in GRAPHS if kind == "hand" or N >= 5]

_cache = {}


def _hand_graph(N):
    """An asymmetric CSR: row 0 a hub of all N - 1 other cells, row 1 empty, row 2 with a self-loop, the others up to six
    entries in random order (repeats among them); weights log-uniform in [1e-9, 1], one of them exactly 1e-9, one exactly
    1, and one stored zero."""
    rng = np.random.default_rng(1000 + N)
    rows = []
    for i in range(N):
        if i == 0:
            at = np.arange(1, N) if N > 1 else np.array([0])
        elif i == 1:
            at = np.array([], dtype=np.int64)
        else:
            at = rng.integers(0, N, size=rng.integers(1, 7))
            if i == 2:
                at[0] = 2
        rows.append(at)
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    data = 10.0 ** rng.uniform(-9, 0, size=indices.size)
    data[0] = 1e-9
    data[-1] = 1.0
    if indices.size > 3:
        data[indices.size // 2] = 0.0
    return indptr, indices, data


def _graph(N, kind):
    """(indptr, indices, data) host arrays: the library's own connectivities of random 5-d points with k = 4, or the
    hand-made graph."""
    if ("graph", N, kind) not in _cache:
        if kind == "hand":
            g = _hand_graph(N)
        else:
            from prosstt_amd import graph, neighbors
            pts = np.random.default_rng(N).standard_normal((N, 5)).astype(np.float32)
            c = graph.connectivities(neighbors.knn(pts, 4), out="scipy")
            g = (c.indptr, c.indices, c.data)
        _cache["graph", N, kind] = g
    return _cache["graph", N, kind]


def _as_graph(csr):
    from prosstt_amd import graph
    return graph.Connectivities(*csr, None, None)


def _mean(N, G):
    """The mu of the drawn matrix as ``graph_sums`` computes it: S1 / N of embed's gene moments."""
    from prosstt_amd import embed
    if ("mean", N, G) not in _cache:
        _cache["mean", N, G] = embed.LogNormalized(_view(N, G, "aligned"), _host(N, G)[1]).gene_moments()[0] / N
    return _cache["mean", N, G]


def _model(N, G, kind, rpb, mean=None):
    """The model's four sums for the drawn matrix centred with ``mean`` (None: ``_mean``)."""
    mean = _mean(N, G) if mean is None else mean
    key = ("model", N, G, kind, rpb, mean.tobytes())
    if key not in _cache:
        _cache[key] = am.sums(_a32(N, G), *_graph(N, kind), mean, rpb or am.default_rows_per_block(N))
    return _cache[key]


def _model_smooth(N, G, kind, normalize):
    key = ("smooth", N, G, kind, normalize)
    if key not in _cache:
        _cache[key] = am.smooth(_a32(N, G), *_graph(N, kind), normalize)
    return _cache[key]


def _bits32(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _check(gs, want, what):
    for name, w in zip(("cross", "sqdiff", "m2", "m4"), want):
        assert _same_bits(getattr(gs, name), w), (name, what)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("N,G,kind", CASES)
def test_sums_bit_for_bit(N, G, kind, view):
    from prosstt_amd import autocorr
    csr = _graph(N, kind)
    if kind == "hand" and N == 300:
        assert np.diff(csr[0]).max() == 299                            # the hub: more than 256 entries
    s = _host(N, G)[1]
    X = _view(N, G, view)
    first = autocorr.graph_sums(X, s, _as_graph(csr))
    assert first.n_cells == N and first.mean.shape == (G,)
    np.testing.assert_allclose(first.mean, _mean(N, G), rtol=1e-13)      # (its own gene_moments call: that library's order)
    assert (first.w_total, first.s1, first.s2) == autocorr.graph_constants(*csr)
    _check(first, _model(N, G, kind, 0, first.mean), "the default call")
    for rpb in ROWS_PER_BLOCK:
        for tile in TILES:
            gs = autocorr.graph_sums(X, s, _as_graph(csr), rows_per_block=rpb, gene_tile=tile, mean=_mean(N, G))
            _check(gs, _model(N, G, kind, rpb), (rpb, tile))


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("N,G,kind", CASES)
def test_smooth_bit_for_bit(N, G, kind, view):
    from prosstt_amd import autocorr
    csr = _graph(N, kind)
    s = _host(N, G)[1]
    for normalize in (True, False):
        want = _model_smooth(N, G, kind, normalize)
        for tile in [0] + TILES:
            got = autocorr.smooth(_view(N, G, view), s, _as_graph(csr), normalize=normalize, gene_tile=tile)
            assert got.is_cuda and got.dtype.is_floating_point and tuple(got.shape) == (N, G)
            assert _bits32(got.cpu().numpy(), want), (normalize, tile)
    if kind == "hand" and N > 1:
        assert not want[1].any()                                       # the empty row gives zeros


def test_graphs_as_device_tensors_transitions_and_neighbors():
    """The three kinds of graph argument, on the device: all end in the same CSR arrays."""
    import torch
    from prosstt_amd import autocorr, graph, neighbors
    N, G = 130, 300
    s = _host(N, G)[1]
    X = _view(N, G, "aligned")
    pts = np.random.default_rng(N).standard_normal((N, 5)).astype(np.float32)
    nb = neighbors.knn(pts, 4, out="torch")
    want = _model(N, G, "knn", 0)
    _check(autocorr.graph_sums(X, s, nb), want, "Neighbors")
    _check(autocorr.graph_sums(X, s, graph.connectivities(nb, out="torch")), want, "device Connectivities")
    T = graph.transitions(nb)
    assert isinstance(T, graph.Transitions) and T.data.is_cuda
    on_device = autocorr.graph_sums(X, s, T, out="torch")
    assert on_device.cross.is_cuda and on_device.cross.dtype == torch.float64 and isinstance(on_device.mean, np.ndarray)
    csr = tuple(t.cpu().numpy() for t in (T.indptr, T.indices, T.data))
    _check(autocorr.graph_sums(X, s, T), am.sums(_a32(N, G), *csr, _mean(N, G), am.default_rows_per_block(N)), "Transitions")
    bad = graph.Connectivities(csr[0], np.where(csr[1] == 3, N, csr[1]).astype(np.int32), csr[2], None, None)
    with pytest.raises(ValueError, match="CSR"):
        autocorr.graph_sums(X, s, bad)


def test_a_column_slice_gives_those_columns_bits():
    from prosstt_amd import autocorr
    N, G = 130, 300
    s = _host(N, G)[1]
    for view in VIEWS:
        for kind in GRAPHS:
            csr = _graph(N, kind)
            X = _view(N, G, view)
            full = autocorr.graph_sums(X, s, _as_graph(csr))
            gs = autocorr.graph_sums(X[:, 10:50], s, _as_graph(csr), mean=full.mean[10:50])
            for name in ("cross", "sqdiff", "m2", "m4"):
                assert _same_bits(getattr(gs, name), getattr(full, name)[10:50]), (name, view, kind)
            own = autocorr.graph_sums(X[:, 10:50], s, _as_graph(csr))    # centred with its own gene_moments call
            _check(own, am.sums(_a32(N, G)[:, 10:50], *csr, own.mean, am.default_rows_per_block(N)), (view, kind))
            got = autocorr.smooth(X[:, 10:50], s, _as_graph(csr)).cpu().numpy()
            assert _bits32(got, _model_smooth(N, G, kind, True)[:, 10:50])


@pytest.mark.parametrize("rpb", [0, 64])
def test_presented_counts(rpb):
    """Rows permuted: the matrix is read in place, the graph's node i stays cell i of the plan, and the sums take the cells
    in the order of the matrix's rows -- the model's order for that row order, which is also what the call on the matrix
    permuted on the host and the graph relabelled to match gives.  The panel comes back in plan order."""
    import torch
    from prosstt_amd import autocorr, device
    N, G = 300, 130
    X, s = _host(N, G)
    cell_of_row = np.random.default_rng(N).permutation(N)
    presented = device.PresentedCounts(torch.as_tensor(X[cell_of_row]).cuda(), cell_of_row)
    for kind in GRAPHS:
        csr = _graph(N, kind)
        for tile in TILES:
            gs = autocorr.graph_sums(presented, s, _as_graph(csr), rows_per_block=rpb, gene_tile=tile)
            want = am.sums(_a32(N, G), *csr, gs.mean, rpb or am.default_rows_per_block(N), cell_of_row)
            _check(gs, want, (kind, tile))                               # (centred with the mean of its own gene_moments call)
            plan = autocorr.graph_sums(_view(N, G, "aligned"), s, _as_graph(csr), rows_per_block=rpb, gene_tile=tile, mean=gs.mean)
            _check(plan, _model(N, G, kind, rpb, gs.mean), (kind, tile, "plan order"))
            for name in ("cross", "sqdiff", "m2", "m4"):                 # another order of the same terms
                np.testing.assert_allclose(getattr(gs, name), getattr(plan, name), rtol=1e-9, atol=1e-9 * np.abs(want[2]).max())
            got = autocorr.smooth(presented, s, _as_graph(csr), gene_tile=tile, out="numpy")
            assert _bits32(got, _model_smooth(N, G, kind, True))


def test_within_the_exact_arithmetic_bound():
    """The device's sums against the definitions in rational arithmetic, for the first genes of one matrix: within (n + 4)
    2^-53 sum |terms| for n terms."""
    from prosstt_amd import autocorr
    N, G, take = 63, 64, 6
    s = _host(N, G)[1]
    csr = _graph(N, "hand")
    gs = autocorr.graph_sums(_view(N, G, "aligned"), s, _as_graph(csr))
    values, masses, counts = am.exact_sums(_a32(N, G)[:, :take], *csr, gs.mean[:take])
    for name, want, mass, n in zip(("cross", "sqdiff", "m2", "m4"), values, masses, counts):
        got = getattr(gs, name)
        worst = 0.0
        for g in range(take):
            err = abs(am.Fraction(float(got[g])) - want[g])
            worst = max(worst, float(err / mass[g]) if mass[g] else 0.0)
            assert err <= (n + 4) * am.Fraction(2) ** -53 * mass[g], (name, g)
        print("%s: worst error %.3g of the sum of |terms| (bound %.3g)" % (name, worst, (n + 4) * 2.0 ** -53))


def test_statistics_equal_the_models():
    from prosstt_amd import autocorr
    N, G = 130, 300
    s = _host(N, G)[1]
    for kind in GRAPHS:
        csr = _graph(N, kind)
        cross, sqdiff, m2, _ = _model(N, G, kind, 0)
        w0 = autocorr.graph_constants(*csr)[0]
        X = _view(N, G, "shifted")
        assert _same_bits(autocorr.morans_i(X, s, _as_graph(csr)), am.morans_i(cross, m2, N, w0))
        assert _same_bits(autocorr.gearys_c(X, s, _as_graph(csr)), am.gearys_c(sqdiff, m2, N, w0))
        ac = autocorr.autocorrelation(X, s, _as_graph(csr), 7)
        assert ac.order.shape == (7,) and _same_bits(ac.morans_i, am.morans_i(cross, m2, N, w0))


def test_equal_bits_across_calls_and_streams():
    import torch
    from prosstt_amd import autocorr
    N, G = 300, 130
    s = _host(N, G)[1]
    g = _as_graph(_graph(N, "hand"))
    X = _view(N, G, "aligned")
    first = autocorr.graph_sums(X, s, g, out="torch")
    again = autocorr.graph_sums(X, s, g, out="torch")
    panel = autocorr.smooth(X, s, g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = autocorr.graph_sums(X, s, g, out="torch")
        other_panel = autocorr.smooth(X, s, g)
    side.synchronize()
    for a in ("cross", "sqdiff", "m2", "m4"):
        x = getattr(first, a)
        assert x.is_cuda and x.shape == (G,)
        for y in (getattr(again, a), getattr(other, a)):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), a
    assert torch.equal(panel.view(torch.int32), other_panel.view(torch.int32))


def test_a_negative_count_raises():
    import torch
    from prosstt_amd import autocorr
    N, G = 64, 65
    X, s = _host(N, G)
    g = _as_graph(_graph(N, "hand"))
    for at in ((N - 1, G - 1), (1, 0)):                    # (cell 1 has no entries: it is read as its own row all the same)
        bad = torch.as_tensor(X).cuda()
        bad[at] = -1
        for tile in TILES:
            with pytest.raises(ValueError, match="negative"):
                autocorr.graph_sums(bad, s, g, gene_tile=tile)
            with pytest.raises(ValueError, match="negative"):
                autocorr.smooth(bad, s, g, gene_tile=tile)


def test_refusals_of_the_abi():
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load("autocorr")
    N, G = 63, 64
    X = _view(N, G, "aligned")
    indptr, indices, data = (torch.as_tensor(a).cuda() for a in _graph(N, "hand"))
    nnz = indices.numel()
    inv = torch.ones(N, dtype=torch.float32, device="cuda")
    mean = torch.zeros(G, dtype=torch.float64, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_autocorr_workspace_bytes(N, G, 0, ctypes.byref(need)), "autocorr")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = torch.empty((4, G), dtype=torch.float64, device="cuda")
    panel = torch.empty((N, G), dtype=torch.float32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    off = lambda t, b: ctypes.c_void_p(t.data_ptr() + b)                # noqa: E731

    def sums(X_=_ptr(X), N=N, G=G, ld=X.stride(0), inv_=_ptr(inv), indptr_=_ptr(indptr), indices_=_ptr(indices),
             data_=_ptr(data), nnz=nnz, mean_=_ptr(mean), rpb=0, tile=0, perm_=None, ws_=_ptr(ws), bytes_=need.value, cross_=_ptr(out[0]),
             status_=_ptr(status)):
        return L.prosstt_amd_autocorr_gene_sums(None, X_, N, G, ld, inv_, perm_, indptr_, indices_, data_, nnz, mean_, rpb, tile,
                                                ws_, bytes_, cross_, _ptr(out[1]), _ptr(out[2]), _ptr(out[3]), status_)

    def smooth(X_=_ptr(X), N=N, G=G, ld=X.stride(0), indptr_=_ptr(indptr), data_=_ptr(data), nnz=nnz, tile=0, out_=_ptr(panel),
               ldo=G, status_=_ptr(status)):
        return L.prosstt_amd_autocorr_smooth(None, X_, N, G, ld, _ptr(inv), None, indptr_, _ptr(indices), data_, nnz, 1, tile,
                                             out_, ldo, status_)

    assert sums() == 0 and smooth() == 0
    for kw, text in ((dict(N=0), "N"), (dict(N=1 << 31), "N"), (dict(G=0), "G"), (dict(ld=G - 1), "row stride"),
                     (dict(nnz=-1), "nnz"), (dict(rpb=-1), "rows_per_block"), (dict(tile=128), "gene_tile"),
                     (dict(bytes_=need.value - 1), "workspace"), (dict(X_=None), "NULL"), (dict(inv_=None), "NULL"),
                     (dict(indptr_=None), "NULL"), (dict(indices_=None), "NULL"), (dict(data_=None), "NULL"),
                     (dict(mean_=None), "NULL"), (dict(ws_=None), "NULL"), (dict(cross_=None), "NULL"), (dict(status_=None), "NULL"),
                     (dict(X_=off(X, 2)), "misaligned"), (dict(indptr_=off(indptr, 4)), "misaligned"),
                     (dict(data_=off(data, 4)), "misaligned"), (dict(mean_=off(mean, 4)), "misaligned"),
                     (dict(cross_=off(out, 4)), "misaligned"), (dict(ws_=off(ws, 8)), "16-byte"),
                     (dict(perm_=off(indices, 2)), "misaligned")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(sums(**kw), "autocorr")
    for kw, text in ((dict(N=0), "N"), (dict(N=1 << 31), "N"), (dict(G=0), "G"), (dict(ld=G - 1), "row stride"),
                     (dict(ldo=G - 1), "output row stride"), (dict(nnz=-1), "nnz"), (dict(tile=1), "gene_tile"),
                     (dict(X_=None), "NULL"), (dict(indptr_=None), "NULL"), (dict(data_=None), "NULL"), (dict(out_=None), "NULL"),
                     (dict(status_=None), "NULL"), (dict(X_=off(X, 1)), "misaligned"), (dict(out_=off(panel, 2)), "misaligned"),
                     (dict(indptr_=off(indptr, 4)), "misaligned")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(smooth(**kw), "autocorr")
    for sizes, text in (((0, G, 0), "N"), ((1 << 31, G, 0), "N"), ((N, 0, 0), "G"), ((N, G, -1), "rows_per_block")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_autocorr_workspace_bytes(*sizes, ctypes.byref(need)), "autocorr")
    with pytest.raises(_native.NativeError, match="NULL"):
        _native.check(L.prosstt_amd_autocorr_workspace_bytes(N, G, 0, None), "autocorr")
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_planted_genes_on_the_device():
    import torch
    from prosstt_amd import autocorr, embed
    X, s, csr, planted = planted_case()
    Xd = torch.as_tensor(X).cuda()
    ac = autocorr.autocorrelation(Xd, s, _as_graph(csr))
    # the model on the device's own entries: equal sums, so the model's order
    N, G = X.shape
    A = embed.LogNormalized(Xd, s).matmul(torch.eye(G, dtype=torch.float32, device="cuda")).cpu().numpy()
    gs = autocorr.graph_sums(Xd, s, _as_graph(csr))
    want = am.sums(A, *csr, gs.mean, am.default_rows_per_block(N))
    _check(gs, want, "planted")
    model = autocorr.statistics(gs._replace(cross=want[0], sqdiff=want[1], m2=want[2], m4=want[3]))
    assert np.array_equal(ac.order, model.order)
    H = len(planted)
    assert set(ac.order[:H]) == set(planted) and ac.z_i[:H].min() > ac.z_i[H:].max() and np.all(np.abs(ac.z_i[H:]) < 4)


def test_whole_call_on_a_sampled_tree():
    from prosstt_amd import autocorr, device, embed, neighbors, simulation as sim, workloads
    work = workloads.build("C2", G=300)
    np.random.seed(10)
    X, pt, br, sc = sim.sample_density(work.tree, 600, alpha=work.alpha, beta=work.beta, seed=10, out="torch")
    assert isinstance(X, device.PresentedCounts)
    nb = neighbors.knn(embed.pca(X, sc).scores, 14)
    gs = autocorr.graph_sums(X, sc, nb)
    ac = autocorr.statistics(gs)
    live = gs.m2 > 0
    assert live.any() and np.all(np.isfinite(ac.morans_i[live])) and np.all(np.abs(ac.morans_i[live]) <= 1.5)
    assert np.all(np.isnan(ac.morans_i[~live])) and np.all(np.isfinite(ac.gearys_c[live]))
    print("600 cells of C2 at 300 genes: %d genes vary, I in [%.3f, %.3f], %d genes with adjusted p < 0.01"
          % (live.sum(), np.nanmin(ac.morans_i), np.nanmax(ac.morans_i), int(np.sum(ac.pvals_adj < 0.01))))
    panel = autocorr.smooth(X, sc, nb, out="numpy")
    assert panel.shape == (600, 300) and np.all(np.isfinite(panel)) and panel.min() >= 0
