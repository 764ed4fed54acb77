"""-m gpu: prosstt_amd.graph (libprosstt_amd_graph.so) against the binary64 model of tests/graph_model.py: connectivities and
transitions over sizes at the edges of the memberships kernel's row loop and of every product path, on the test cloud and
on duplicated and tied inputs; the product kernel per forced path against the bound of any summation order; the diffusion
map against dense eigh of the model's operator; repeats and another stream; refusals through the ABI.

Measured on an MI355X: over CONNECTIVITY_CASES the largest relative difference to the model was 4.30e-14
(T at (3001, 1024); W's data 4.28e-14 there; sigma at most 6.3e-16, q 9.8e-16, z 4.4e-16; rho exact; (3, 2), the duplicates
and W of the lattice bit for bit).  It grows with k as the exponent g / sigma does.  REL_BOUND is 16 x that."""
import ctypes
import functools

import numpy as np
import pytest

import graph_model

pytestmark = pytest.mark.gpu

REL_BOUND = 16 * 4.3e-14        # 16 x the largest relative difference measured; it may never exceed 1e-9
assert REL_BOUND <= 1e-9

# (N, k, d, kind): the lane-strided row loop's edges at 64 and 1024 neighbours, rows shorter and longer than every group
CONNECTIVITY_CASES = [(3, 2), (63, 5), (64, 14), (65, 63), (257, 64), (257, 65), (257, 255), (1000, 14), (1000, 700),
                      (3001, 1024), (2000, 100)]
CONNECTIVITY_CASES = [(N, k, 10, "tree") for N, k in CONNECTIVITY_CASES] + [(1200, 15, 3, "duplicates"), (1200, 15, 4, "lattice")]
# degenerate rows wider than one slot of the 16 a lane keeps: twelve points a hundred times each.  k = 70: every row is all
# zero over two slots (rho = 0, sigma = 2^-64 in the model); k = 130: the first positive distance sits in column 99, so
# the minimum that gives rho comes from the second slot
CONNECTIVITY_CASES += [(1200, 70, 3, "copies100"), (1200, 130, 3, "copies100")]


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()               # (a copy: the shared model arrays are read-only)


def _neighbors(case):
    from prosstt_amd import neighbors
    return neighbors.Neighbors(_cuda(case["idx"]), _cuda(case["d2"]))


def _relative(got, want):
    """The largest |got - want| / |want| (0 where both are 0, inf where only want is)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(diff == 0, 0.0, diff / np.abs(want))
    return float(rel.max()) if rel.size else 0.0


@pytest.mark.parametrize("N,k,d,kind", CONNECTIVITY_CASES)
def test_connectivities_and_transitions_against_the_model(N, k, d, kind):
    import torch
    from prosstt_amd import graph
    case = graph_model.case(N, k, d, kind)
    g = graph.connectivities(_neighbors(case), out="torch")
    assert g.indptr.dtype == torch.int64 and g.indices.dtype == torch.int32 and g.data.dtype == torch.float64
    W = case["W"]
    np.testing.assert_array_equal(g.indptr.cpu().numpy(), W.indptr)
    np.testing.assert_array_equal(g.indices.cpu().numpy(), W.indices)
    per_row = np.diff(W.indptr)
    assert per_row.min() >= k and per_row.max() <= N - 1
    if kind == "copies100":
        assert np.all(case["d2"][:, :min(k, 99)] == 0) and np.all(case["d2"][:, 99:] > 0)
        if k < 100:
            assert np.all(case["rho"] == 0) and np.all(case["sigma"] == 2.0 ** -64)
        else:
            assert np.all(case["rho"] == np.sqrt(case["d2"][:, 99].astype(np.float64)))
    elif kind != "tree":
        assert np.any(case["d2"] == 0) and np.any(case["rho"] == 0 if kind == "duplicates" else case["rho"] > 0)
    t = graph.transitions(g)
    assert t.indptr.data_ptr() == g.indptr.data_ptr() and t.indices.data_ptr() == g.indices.data_ptr()
    rel = dict(data=_relative(g.data.cpu().numpy(), W.data), rho=_relative(g.rho.cpu().numpy(), case["rho"]),
               sigma=_relative(g.sigma.cpu().numpy(), case["sigma"]), T=_relative(t.data.cpu().numpy(), case["T"].data),
               q=_relative(t.q.cpu().numpy(), case["q"]), z=_relative(t.z.cpu().numpy(), case["z"]))
    print("relative difference to the model (%d, %d, %s): %s" % (N, k, kind, "  ".join("%s %.3g" % kv for kv in rel.items())))
    for name, value in rel.items():
        assert value <= REL_BOUND, (name, value)
    # symmetric to the bit
    host = g.to_csr()
    assert (host != host.T).nnz == 0
    Tm = t.to_csr()
    assert (Tm != Tm.T).nnz == 0
    # the host form is the same graph
    if N <= 257:
        h = graph.connectivities((case["idx"], case["d2"]))
        assert isinstance(h.data, np.ndarray)
        np.testing.assert_array_equal(h.data, g.data.cpu().numpy())
        np.testing.assert_array_equal(h.sigma, g.sigma.cpu().numpy())
        assert (h.to_csr() != host).nnz == 0


def test_graph_bits_repeat_on_any_stream():
    import torch
    from prosstt_amd import graph
    for N, k in ((1000, 14), (257, 65)):
        nb = _neighbors(graph_model.case(N, k))
        first = graph.transitions(graph.connectivities(nb, out="torch"))
        second = graph.transitions(nb)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            g3 = graph.connectivities(nb, out="torch")
            third = graph.transitions(g3)
        st.synchronize()
        g1 = graph.connectivities(nb, out="torch")
        for name in ("indptr", "indices", "data", "rho", "sigma"):
            assert torch.equal(getattr(g1, name), getattr(g3, name)), name
        for other in (second, third):
            for name in ("indptr", "indices", "data", "q", "z"):
                assert torch.equal(getattr(first, name), getattr(other, name)), name


@functools.lru_cache(maxsize=None)
def _hub_cloud():
    """T of the 20 000 x 14 test cloud in 50 dimensions, neighbours from the device's own search: its hubs make rows far
    longer than any group."""
    from prosstt_amd import graph, neighbors
    P = graph_model.tree_points(20000, 50, 20014)
    return graph.transitions(neighbors.knn(_cuda(P), 14, out="torch"))


@pytest.mark.parametrize("shape", [(65, 63), (1000, 14), (1000, 700), "hubs"])
def test_product_kernel_on_every_path(shape):
    import torch
    from prosstt_amd import graph
    t = _hub_cloud() if shape == "hubs" else graph.transitions(_neighbors(graph_model.case(*shape)))
    T = t.to_csr()
    N = T.shape[0]
    per_row = np.diff(T.indptr)
    if shape == "hubs":
        print("longest row of the 20 000 x 14 cloud: %d entries" % per_row.max())
        assert per_row.max() > 4 * 64 and per_row.min() >= 14
    x = np.random.default_rng(N).standard_normal(N)
    y64 = T @ x
    bound = per_row * 2.0 ** -52 * (abs(T) @ np.abs(x))
    xd = _cuda(x)
    for lanes in (4, 16, 64, 0):
        y = graph.spmv(t, xd, lanes)
        again = graph.spmv(t, xd, lanes)
        assert torch.equal(y, again), lanes
        err = np.abs(y.cpu().numpy() - y64)
        print("lanes %2d: largest error / bound %.3g" % (lanes, float(np.max(err / bound))))
        assert np.all(err <= bound), lanes


@functools.lru_cache(maxsize=None)
def _spectrum(N, k, d):
    """(eigenvalues by descending magnitude, eigenvectors, gap of every eigenvalue to the rest) of the model's T."""
    lam, vec = graph_model.dense_spectrum(graph_model.case(N, k, d)["T"])
    ordered = np.sort(lam)
    at = np.searchsorted(ordered, lam)
    below = np.where(at > 0, lam - ordered[np.maximum(at - 1, 0)], np.inf)
    above = np.where(at < lam.size - 1, ordered[np.minimum(at + 1, lam.size - 1)] - lam, np.inf)
    return lam, vec, np.minimum(below, above)


def _check_diffmap(dm, N, k, d, n_comps, tol=1e-10):
    case = graph_model.case(N, k, d)
    lam, vec, gap = _spectrum(N, k, d)
    leading = np.sort(lam[:n_comps + 1])[::-1]
    assert np.min(-np.diff(leading)) >= 2e-5, "the test input has degenerated: eigenvalues %r" % (leading,)
    want_values, want_vectors = graph_model.leading(lam, vec, n_comps)
    order = np.argsort(-lam[:n_comps], kind="stable")
    gaps = gap[:n_comps][order]
    values, vectors = dm.eigenvalues, dm.eigenvectors
    assert values.shape == (n_comps,) and vectors.shape == (N, n_comps) and dm.residuals.shape == (n_comps,)
    assert dm.steps <= 256 and np.all(dm.residuals < tol)
    print("(%d, %d, %d): %d steps, largest eigenvalue error %.3g" % (N, k, d, dm.steps, np.abs(values - want_values).max()))
    assert np.all(np.abs(values - want_values) <= 2e-9)
    T = dm.transitions
    assert np.all(np.linalg.norm(T @ vectors - vectors * values, axis=0) <= 2 * tol)
    assert np.all(np.abs(np.linalg.norm(vectors, axis=0) - 1) <= 1e-14)
    along = np.sum(vectors * want_vectors, axis=0)
    sines = np.linalg.norm(vectors - want_vectors * along, axis=0)
    assert np.all(sines <= 2 * (tol + 1e-9) / gaps), (sines, gaps)
    z = case["z"]
    assert np.all(np.abs(vectors[:, 0] - z / np.linalg.norm(z)) <= 1e-9) and abs(values[0] - 1) <= 2e-9
    first = np.argmax(np.abs(vectors), axis=0)
    assert np.all(vectors[first, np.arange(n_comps)] > 0)


@pytest.mark.parametrize("N,k", [(40, 10), (300, 5), (1000, 14), (2000, 100)])
def test_diffmap_against_dense_eigh(N, k):
    from prosstt_amd import graph
    dm = graph.diffmap(_neighbors(graph_model.case(N, k)), 15)
    assert isinstance(dm.eigenvectors, np.ndarray)
    _check_diffmap(dm, N, k, 10, 15)


def test_diffmap_of_the_devices_own_neighbours():
    import torch
    from prosstt_amd import graph, neighbors
    N, d, k = 2000, 50, 14
    case = graph_model.case(N, k, d)
    nb = neighbors.knn(_cuda(case["P"]), k, out="torch")
    np.testing.assert_array_equal(nb.indices.cpu().numpy(), case["idx"])
    dm = graph.diffmap(nb, out="torch")
    assert dm.eigenvectors.is_cuda and dm.eigenvalues.is_cuda and dm.transitions.data.is_cuda
    host = graph.DiffusionMap(dm.eigenvalues.cpu().numpy(), dm.eigenvectors.cpu().numpy(), dm.steps, dm.residuals,
                              dm.transitions.to_csr())
    _check_diffmap(host, N, k, d, 15)


def test_diffmap_bits_repeat_and_not_converged():
    from prosstt_amd import graph
    nb = _neighbors(graph_model.case(1000, 14))
    first = graph.diffmap(nb)
    second = graph.diffmap(graph.connectivities(nb, out="torch"))
    np.testing.assert_array_equal(first.eigenvalues, second.eigenvalues)
    np.testing.assert_array_equal(first.eigenvectors, second.eigenvectors)
    assert first.steps == second.steps
    other = graph.diffmap(nb, seed=1)
    assert not np.array_equal(first.eigenvectors, other.eigenvectors)
    assert np.all(np.abs(first.eigenvalues - other.eigenvalues) <= 4e-10)
    with pytest.raises(graph.NotConverged, match="20 Lanczos steps") as info:
        graph.diffmap(nb, max_steps=20)
    assert info.value.steps == 20 and info.value.residuals.shape == (15,) and info.value.residuals.max() >= 1e-10


def test_refusals_through_the_abi():
    import torch
    from prosstt_amd import _native, graph, neighbors
    from prosstt_amd.device import _ptr
    case = graph_model.case(63, 5)
    idx, d2 = _cuda(case["idx"]), _cuda(case["d2"])
    for row, col, value, text in ((7, 2, 63, "outside"), (7, 2, -1, "outside"), (62, 4, 62, "its own neighbour")):
        bad = idx.clone()
        bad[row, col] = value
        for call in (graph.connectivities, graph.diffmap, graph.transitions):
            with pytest.raises(ValueError, match=text):
                call(neighbors.Neighbors(bad, d2))
    for value in (-1.0, float("nan"), float("inf"), -0.5e-30):
        bad = d2.clone()
        bad[11, 0] = value
        with pytest.raises(ValueError, match="negative, infinite or NaN"):
            graph.connectivities(neighbors.Neighbors(idx, bad))
    g = graph.connectivities(neighbors.Neighbors(idx, d2), out="torch")
    for field, bad in (("indptr", g.indptr + 1), ("indptr", g.indptr.flip(0)), ("indices", g.indices + 1),
                       ("indices", g.indices - 1)):
        with pytest.raises(ValueError, match="not those of a CSR matrix"):
            graph.diffmap(g._replace(**{field: bad}), 3)
    with pytest.raises(ValueError, match="positive finite"):
        graph.transitions(g._replace(data=torch.zeros_like(g.data)))
    # sizes are refused by the library before anything is enqueued
    L = _native.load("graph")
    N, k = 63, 5
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_graph_workspace_bytes(N, k, ctypes.byref(need)), "graph")
    assert need.value >= 2 * 16 * N * k
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    a = torch.full((N, k), -7.0, dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n, kk in ((2, 1), (63, 1), (63, 63), (2000, 1025)):
        with pytest.raises(_native.NativeError, match="need "):
            _native.check(L.prosstt_amd_graph_workspace_bytes(n, kk, ctypes.byref(need)), "graph")
        with pytest.raises(_native.NativeError, match="need "):
            _native.check(L.prosstt_amd_graph_symmetrize_emit(stream, _ptr(idx), _ptr(a), n, kk, _ptr(ws), ws.numel()), "graph")
    with pytest.raises(_native.NativeError, match="workspace of %d bytes" % (ws.numel() - 1)):
        _native.check(L.prosstt_amd_graph_symmetrize_emit(stream, _ptr(idx), _ptr(a), N, k, _ptr(ws), ws.numel() - 1), "graph")
    t = graph.transitions(g)
    x = torch.ones(N, dtype=torch.float64, device="cuda")
    y = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    for lanes in (1, 8, 32, 128, -4):
        with pytest.raises(_native.NativeError, match="lanes_per_row"):
            _native.check(L.prosstt_amd_graph_spmv(stream, _ptr(t.indptr), _ptr(t.indices), _ptr(t.data), N,
                                                   t.indices.numel(), _ptr(x), _ptr(y), lanes), "graph")
    with pytest.raises(_native.NativeError, match="alias"):
        _native.check(L.prosstt_amd_graph_spmv(stream, _ptr(t.indptr), _ptr(t.indices), _ptr(t.data), N,
                                               t.indices.numel(), _ptr(x), _ptr(x), 0), "graph")
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())                                # nothing was enqueued
    with pytest.raises(ValueError, match="float64 vector"):
        graph.spmv(t, x.float())
