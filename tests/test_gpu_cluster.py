"""-m gpu: the kernels of libprosstt_amd_cluster.so (prosstt_amd/csrc/cluster/cluster.hip) and prosstt_amd.cluster on top of
them, against tests/cluster_model.py.  Everything is compared BIT FOR BIT: communities, counts of moved nodes, the int64
totals, the aggregated graphs, the labels, and Q (an exact sum of terms computed by the same binary64 operations).

The hand-built level graphs (cluster_model.hand_built) reach what kNN graphs of test size do not: rows of exactly 1, 16, 17,
64, 65, 512 and 513 entries (one past what each short path and the LDS table hold), a dense row of n entries, diagonals, entries
of weight 0, a node with k = 0.  They come with weights of 2^32 throughout and, since 2100 rows of 2^32 stay below 2^53, also
with weights of 2^47 + 1 + (i + j) % 3, whose row sums and totals exceed 2^53 with low bits set: a sum that passed through
binary64 would differ there.  n = 2100 makes the range path take two passes."""
import ctypes

import numpy as np
import pytest

import cluster_model as cm
import graph_model

pytestmark = pytest.mark.gpu

KNN_CASES = [(3, 2), (64, 5), (65, 14), (300, 14)]
HAND_SIZES = [5, 130, 700, 2100]
WEIGHTS = {"2^32": (1 << 32, False), "2^47": ((1 << 47) + 1, True)}
PATHS = [0, 1, 2, 3, 4]
ROW_LIMIT = {0: None, 1: 16, 2: 64, 3: 512, 4: None}
LOUVAIN_CASES = [(300, 5), (1000, 14)]
GAMMAS = [0.5, 1.0, 2.0]

_cache = {}


def _connectivities(N, k):
    from prosstt_amd import graph
    case = graph_model.case(N, k)
    W = case["W"]
    return graph.Connectivities(W.indptr.astype(np.int64), W.indices.astype(np.int32), W.data.astype(np.float64),
                                case["rho"], case["sigma"])


def _knn_level(N, k):
    """(the model's level-0 graph, the device's) of graph_model.case(N, k)."""
    from prosstt_amd import cluster
    if ("knn", N, k) not in _cache:
        _cache["knn", N, k] = (cm.quantize(graph_model.case(N, k)["W"]), cluster.quantize(_connectivities(N, k)))
    return _cache["knn", N, k]


def _hand_level(n, weight):
    from prosstt_amd import cluster
    if ("hand", n, weight) not in _cache:
        model, lengths = cm.hand_built(n, *WEIGHTS[weight])
        dev = cluster.LevelGraph.from_csr(model.indptr, model.indices.astype(np.int32), model.u)
        _cache["hand", n, weight] = (model, dev, int(lengths.max()))
    return _cache["hand", n, weight]


def _starts(n):
    """Start communities: every node its own; three communities, so that many lanes share one; a scattered few."""
    i = np.arange(n, dtype=np.int64)
    return [i, i % 3, (i * 7919) % min(n, 40)]


def _same_level(dev, model):
    assert dev.M2 == model.M2
    for name in ("indptr", "indices", "u", "k"):
        assert np.array_equal(getattr(dev, name).cpu().numpy().astype(np.int64), getattr(model, name)), name


def _check_sweeps(model, dev, longest):
    from prosstt_amd import _native, cluster
    for c in _starts(model.n):
        tot, _ = cm.totals(model, c)
        for parity in (0, 1):
            want, moved = cm.sweep(model, c, tot, parity, 1.0)
            for path in PATHS:
                if ROW_LIMIT[path] is not None and longest > ROW_LIMIT[path]:
                    with pytest.raises(_native.NativeError, match="rows are longer"):
                        cluster.sweep(dev, c, parity, 1.0, path)
                    continue
                got, got_moved = cluster.sweep(dev, c, parity, 1.0, path)
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (parity, path)
                assert got_moved == moved, (parity, path)


@pytest.mark.parametrize("N,k", KNN_CASES)
def test_sweep_bit_for_bit_on_knn_graphs(N, k):
    model, dev = _knn_level(N, k)
    _same_level(dev, model)                              # the quantisation itself: u, k and M2
    _check_sweeps(model, dev, int(np.diff(model.indptr).max()))


@pytest.mark.parametrize("weight", list(WEIGHTS))
@pytest.mark.parametrize("n", HAND_SIZES)
def test_sweep_bit_for_bit_on_hand_built_graphs(n, weight):
    model, dev, longest = _hand_level(n, weight)
    assert longest == n and model.k[1] == 0 and (model.u == 0).any()
    if weight == "2^47" and n >= 130:
        assert model.k.max() > 1 << 53
    _same_level(dev, model)
    _check_sweeps(model, dev, longest)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_sweep_follows_the_resolution(gamma):
    from prosstt_amd import cluster
    model, dev, _ = _hand_level(130, "2^47")
    c = _starts(130)[2]
    tot, _ = cm.totals(model, c)
    for parity in (0, 1):
        want, moved = cm.sweep(model, c, tot, parity, gamma)
        got, got_moved = cluster.sweep(dev, c, parity, gamma)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and got_moved == moved


@pytest.mark.parametrize("path", PATHS)
def test_an_exact_tie_goes_to_the_lower_community(path):
    from prosstt_amd import cluster
    model = cm.tie_graph()
    dev = cluster.LevelGraph.from_csr(model.indptr, model.indices.astype(np.int32), model.u)
    c = np.arange(5, dtype=np.int64)
    tot, _ = cm.totals(model, c)
    g = cm.gain([model.u[0]] * 2, [model.k[4]] * 2, [tot[1], tot[2]], 1.0, model.M2)
    assert g[0] == g[1] > 0.0                            # the tie, above the stay of a node alone (0)
    got, moved = cluster.sweep(dev, c, 0, 1.0, path)
    assert got.cpu().tolist() == [0, 1, 2, 1, 1] and moved == 2
    assert np.array_equal(cm.sweep(model, c, tot, 0, 1.0)[0], [0, 1, 2, 1, 1])


@pytest.mark.parametrize("weight", list(WEIGHTS))
@pytest.mark.parametrize("n", HAND_SIZES)
def test_totals_and_aggregate_on_hand_built_graphs(n, weight):
    from prosstt_amd import cluster
    model, dev, _ = _hand_level(n, weight)
    for c in _starts(n) + [np.zeros(n, dtype=np.int64), np.full(n, n - 1, dtype=np.int64)]:     # the last two: one run holds every entry
        tot, inn = cm.totals(model, c)
        got_tot, got_in = cluster.totals(dev, c)
        assert np.array_equal(got_tot.cpu().numpy(), tot) and np.array_equal(got_in.cpu().numpy(), inn)
        nxt, cnew = cm.aggregate(model, c)
        got_nxt, got_cnew = cluster.aggregate(dev, c)
        assert np.array_equal(got_cnew.cpu().numpy().astype(np.int64), cnew)
        _same_level(got_nxt, nxt)
        longest = int(np.diff(nxt.indptr).max())
        assert got_nxt.bins == tuple(int((np.diff(nxt.indptr) <= b).sum()) for b in (16, 64, 512)), longest


def test_totals_and_aggregate_on_a_knn_graph():
    from prosstt_amd import cluster
    model, dev = _knn_level(300, 14)
    c = (np.arange(300, dtype=np.int64) * 7919) % 25
    tot, inn = cm.totals(model, c)
    got_tot, got_in = cluster.totals(dev, c)
    assert np.array_equal(got_tot.cpu().numpy(), tot) and np.array_equal(got_in.cpu().numpy(), inn)
    nxt, cnew = cm.aggregate(model, c)
    got_nxt, got_cnew = cluster.aggregate(dev, c)
    assert np.array_equal(got_cnew.cpu().numpy().astype(np.int64), cnew)
    _same_level(got_nxt, nxt)


def _model_louvain(N, k, gamma):
    if ("louvain", N, k, gamma) not in _cache:
        _cache["louvain", N, k, gamma] = cm.louvain(graph_model.case(N, k)["W"], gamma)
    return _cache["louvain", N, k, gamma]


def _same_clusters(got, want):
    assert np.array_equal(got.labels, want.labels) and got.labels.dtype == np.int32
    assert np.array_equal(got.sizes, want.sizes)
    assert got.levels == want.levels                     # nodes, communities, rounds and Q to the bit, per level
    assert got.modularity == want.modularity
    assert len(got.level_labels) == len(want.level_labels)
    for a, b in zip(got.level_labels, want.level_labels):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("N,k", LOUVAIN_CASES)
def test_louvain_equals_the_model(N, k, gamma):
    from prosstt_amd import _native, cluster
    want = _model_louvain(N, k, gamma)
    g = _connectivities(N, k)
    got = cluster.louvain(g, gamma)
    _same_clusters(got, want)
    assert cluster.modularity(g, got.labels, gamma) == want.modularity
    for path in (2, 3, 4):                               # (rows of these graphs have at most 64 entries on every level)
        _same_clusters(cluster.louvain(g, gamma, path=path), want)
    try:                                                 # 16 lanes hold no level of these graphs whole
        _same_clusters(cluster.louvain(g, gamma, path=1), want)
    except _native.NativeError as exc:
        assert "rows are longer" in str(exc)


def test_equal_bits_across_calls_streams_and_outputs():
    import torch
    from prosstt_amd import cluster
    want = _model_louvain(1000, 14, 1.0)
    g = _connectivities(1000, 14)
    first = cluster.louvain(g, out="torch")
    assert first.labels.is_cuda and first.labels.dtype == torch.int32 and first.sizes.is_cuda
    assert all(t.is_cuda for t in first.level_labels)
    again = cluster.louvain(g, out="torch")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = cluster.louvain(g, out="torch")
    side.synchronize()
    for res in (first, again, other):
        assert np.array_equal(res.labels.cpu().numpy(), want.labels) and np.array_equal(res.sizes.cpu().numpy(), want.sizes)
        assert res.levels == want.levels and res.modularity == want.modularity
        for a, b in zip(res.level_labels, want.level_labels):
            assert np.array_equal(a.cpu().numpy(), b)


def test_neighbors_and_connectivities_give_the_same():
    import torch
    from prosstt_amd import cluster, graph, neighbors
    case = graph_model.case(300, 14)
    nb = neighbors.knn(torch.from_numpy(case["P"].copy()).cuda(), 14, out="torch")
    a = cluster.louvain(nb)
    g = graph.connectivities(nb, out="torch")
    b = cluster.louvain(g)
    _same_clusters(a, b)
    assert a.modularity == cluster.modularity(g, a.labels) == cm.modularity(g.to_csr(), a.labels)
    assert a.sizes.sum() == 300 and np.all(np.diff(a.sizes) <= 0)


@pytest.mark.parametrize("gamma", GAMMAS)
def test_modularity_of_any_labelling(gamma):
    from prosstt_amd import cluster
    W = graph_model.case(300, 14)["W"]
    g = _connectivities(300, 14)
    rng = np.random.default_rng(3)
    for labels in (rng.integers(0, 7, 300), np.zeros(300, dtype=np.int64), np.arange(300), np.array(list("abc") * 100)):
        assert cluster.modularity(g, labels, gamma) == cm.modularity(W, labels, gamma)


def test_clusters_go_straight_into_the_markers():
    from prosstt_amd import cluster, embed, markers, neighbors, simulation as sim, workloads
    work = workloads.build("C2", G=300)
    np.random.seed(10)
    X, pt, br, sc = sim.sample_density(work.tree, 600, alpha=work.alpha, beta=work.beta, seed=10, out="torch")
    p = embed.pca(X, sc, 20)
    cl = cluster.louvain(neighbors.knn(p.scores, 14, out="torch"))
    assert cl.labels.shape == (600,) and len(cl.sizes) >= 2 and cl.modularity > 0.3
    res = markers.rank_genes_groups(X, sc, cl.labels)
    assert list(res.groups) == list(range(len(cl.sizes)))
    assert np.array_equal(res.moments.n, cl.sizes)
    assert res.names.shape[0] == len(cl.sizes)


def test_bad_weights_and_an_empty_graph_raise():
    from prosstt_amd import cluster
    g = _connectivities(64, 5)
    for bad in (1.5, np.nan, -0.25):
        data = g.data.copy()
        data[7] = bad
        with pytest.raises(ValueError, match="NaN, negative or above 1"):
            cluster.louvain(g._replace(data=data))
        with pytest.raises(ValueError, match="NaN, negative or above 1"):
            cluster.modularity(g._replace(data=data), np.zeros(64))
    with pytest.raises(ValueError, match="no weight"):
        cluster.louvain(g._replace(data=np.zeros_like(g.data)))
    with pytest.raises(ValueError, match="no weight"):
        cluster.louvain(g._replace(indptr=np.zeros(65, dtype=np.int64), indices=g.indices[:0], data=g.data[:0]))
    with pytest.raises(ValueError, match="CSR"):
        cluster.louvain(g._replace(indices=np.where(np.arange(g.indices.size) == 3, 64, g.indices).astype(np.int32)))


def test_bad_level_graphs_and_communities_raise():
    from prosstt_amd import cluster
    model, dev, _ = _hand_level(130, "2^32")
    idx = model.indices.astype(np.int32)
    with pytest.raises(ValueError, match="CSR"):
        cluster.LevelGraph.from_csr(model.indptr[::-1].copy(), idx, model.u)
    with pytest.raises(ValueError, match="CSR"):
        cluster.LevelGraph.from_csr(model.indptr, np.where(np.arange(idx.size) == 9, 130, idx).astype(np.int32), model.u)
    with pytest.raises(ValueError, match="overflows"):
        cluster.LevelGraph.from_csr(model.indptr, idx, np.full_like(model.u, 1 << 60))
    with pytest.raises(ValueError, match="overflows"):
        cluster.LevelGraph.from_csr(model.indptr, idx, -model.u)
    c = np.arange(130, dtype=np.int64)
    c[5] = 130
    for call in (lambda: cluster.sweep(dev, c, 0), lambda: cluster.totals(dev, c), lambda: cluster.aggregate(dev, c)):
        with pytest.raises(ValueError, match="community"):
            call()


def test_refusals_of_the_abi():
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load("cluster")
    model, dev, _ = _hand_level(130, "2^32")
    n, nnz = dev.n, dev.indices.numel()
    c = torch.arange(n, dtype=torch.int32, device="cuda")
    c_new = torch.empty_like(c)
    tot, inn = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    W = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    u, k = torch.empty(nnz, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_cluster_workspace_bytes(n, nnz, ctypes.byref(need)), "cluster")
    assert need.value >= 8 * nnz
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")

    def sweep(n=n, nnz=nnz, bins=dev.bins, M2=dev.M2, gamma=1.0, parity=0, path=0, c_new=c_new, rows=dev.rows):
        return L.prosstt_amd_cluster_sweep(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(dev.u), _ptr(dev.k), n, nnz, _ptr(rows),
                                           *bins, _ptr(c), _ptr(tot), M2, gamma, parity, path, _ptr(c_new), _ptr(flags[1:]),
                                           _ptr(flags))

    assert sweep() == 0
    b16, b64, b512 = dev.bins
    assert b16 < b64 < b512 == n                          # rows of 17, 65 and 130 entries
    for kw, text in ((dict(n=0), "n"), (dict(n=1 << 31), "n"), (dict(nnz=0), "nnz"), (dict(nnz=1 << 31), "nnz"),
                     (dict(bins=(b64, b16, b512)), "n16"), (dict(bins=(b16, b64, n + 1)), "n512"), (dict(bins=(-1, b64, b512)), "n16"),
                     (dict(M2=0), "M2"), (dict(gamma=0.0), "resolution"), (dict(gamma=float("nan")), "resolution"),
                     (dict(gamma=float("inf")), "resolution"), (dict(parity=2), "parity"), (dict(path=5), "path"),
                     (dict(path=-1), "path"), (dict(path=1), "rows are longer"), (dict(path=2), "rows are longer"),
                     (dict(c_new=c), "alias"), (dict(rows=None), "NULL")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(sweep(**kw), "cluster")
    assert sweep(path=3) == 0 and sweep(path=4) == 0
    calls = (
        (lambda: L.prosstt_amd_cluster_workspace_bytes(0, nnz, ctypes.byref(need)), "n"),
        (lambda: L.prosstt_amd_cluster_workspace_bytes(n, nnz, None), "NULL"),
        (lambda: L.prosstt_amd_cluster_quantize(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(W), 2, nnz, _ptr(u), _ptr(k),
                                                _ptr(flags)), "3 <= N"),
        (lambda: L.prosstt_amd_cluster_quantize(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(W), n, 1 << 30, _ptr(u), _ptr(k),
                                                _ptr(flags)), "2\\^30"),
        (lambda: L.prosstt_amd_cluster_quantize(None, _ptr(dev.indptr), _ptr(dev.indices), None, n, nnz, _ptr(u), _ptr(k),
                                                _ptr(flags)), "NULL"),
        (lambda: L.prosstt_amd_cluster_totals(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(dev.u), _ptr(dev.k), n, nnz, _ptr(c),
                                              _ptr(tot), _ptr(tot), _ptr(flags)), "alias"),
        (lambda: L.prosstt_amd_cluster_totals(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(dev.u), _ptr(dev.k), 0, nnz, _ptr(c),
                                              _ptr(tot), _ptr(inn), _ptr(flags)), "n"),
        (lambda: L.prosstt_amd_cluster_aggregate_emit(None, _ptr(dev.indptr), _ptr(dev.indices), n, nnz, _ptr(c), n + 1, _ptr(ws),
                                                      need.value, _ptr(flags)), "n_new"),
        (lambda: L.prosstt_amd_cluster_aggregate_emit(None, _ptr(dev.indptr), _ptr(dev.indices), n, nnz, _ptr(c), n, _ptr(ws),
                                                      8 * nnz - 8, _ptr(flags)), "workspace"),
        (lambda: L.prosstt_amd_cluster_aggregate_emit(None, _ptr(dev.indptr), _ptr(dev.indices), n, nnz, _ptr(c), n,
                                                      ctypes.c_void_p(ws.data_ptr() + 8), need.value, _ptr(flags)), "aligned"),
        (lambda: L.prosstt_amd_cluster_aggregate_fold(None, _ptr(u), _ptr(u), _ptr(u), _ptr(dev.u), nnz, n, nnz + 1, _ptr(tot),
                                                      _ptr(c), _ptr(u), _ptr(flags)), "nnz_new"),
        (lambda: L.prosstt_amd_cluster_aggregate_fold(None, _ptr(u), _ptr(u), _ptr(u), _ptr(dev.u), nnz, 0, nnz, _ptr(tot),
                                                      _ptr(c), _ptr(u), _ptr(flags)), "n"),
    )
    for call, text in calls:
        with pytest.raises(_native.NativeError, match=text):
            _native.check(call(), "cluster")
    torch.cuda.synchronize()
    assert int(flags[0].item()) == 0


def test_rows_binned_too_short_are_cut_and_reported():
    """The C ABI's own guard (cluster.py counts the bins itself): counts that put a long row on a short path set a bit, and
    the kernel reads no more of the row than the path holds."""
    import torch
    from prosstt_amd import _native, cluster
    from prosstt_amd.device import _ptr
    L = _native.load("cluster")
    model, dev, _ = _hand_level(130, "2^32")
    n, nnz = dev.n, dev.indices.numel()
    c = torch.arange(n, dtype=torch.int32, device="cuda")
    tot = dev.k.clone()
    for path in (1, 2):
        c_new = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        flags = torch.zeros(2, dtype=torch.int32, device="cuda")
        _native.check(L.prosstt_amd_cluster_sweep(None, _ptr(dev.indptr), _ptr(dev.indices), _ptr(dev.u), _ptr(dev.k), n, nnz,
                                                  _ptr(dev.rows), n, n, n, _ptr(c), _ptr(tot), dev.M2, 1.0, 0, path, _ptr(c_new),
                                                  _ptr(flags[1:]), _ptr(flags)), "cluster")
        assert int(flags[0].item()) == cluster.BAD_BINS
        got = c_new.cpu().numpy()
        assert np.all((got >= 0) & (got < n))             # every node was decided, within range
