"""-m gpu: neighbors.knn (libprosstt_amd_knn.so) bit for bit against the scalar model of tests/knn_model.py over odd sizes,
every k path, forced chunk boundaries, host arrays, contiguous tensors and unaligned column views, on Gaussian, tied,
duplicated and badly scaled inputs; several default chunks against a torch restatement on the device; repeats and
another stream; the sampler's PCA scores; errors through the ABI."""
import ctypes

import numpy as np
import pytest

import knn_model

pytestmark = pytest.mark.gpu

# (N, d, k, chunk_rows, view, kind).  k "N-1" and chunk "N" are taken from N.  view: None = a host array (copied to rows
# padded to 16 bytes: the 16-byte load path), (pad, shift) = the columns shift .. shift + d of a device tensor d + pad wide
# ((0, 0): contiguous; pad 3, shift 1: rows that do not start on 16 bytes, the 4-byte load path).
# N in {2, 3, 63, 64, 65, 257, 1000, 3001}, d in {1, 2, 3, 31, 32, 33, 50, 128}, k in {1, 2, 15, 16, 17, 255, 256, 700,
# 1024, N - 1}, chunk_rows in {None, 1, 7, 64, N}: every value at least twice, (3001, 128) once.
CASES = [
    (2, 1, 1, None, None, "gaussian"),
    (2, 33, "N-1", 1, (3, 1), "gaussian"),
    (3, 2, 2, 1, (0, 0), "gaussian"),
    (3, 128, 1, "N", (3, 1), "scaled"),
    (63, 3, 15, 7, None, "gaussian"),
    (63, 31, "N-1", None, (3, 1), "scaled"),
    (64, 32, 16, 64, (0, 0), "gaussian"),
    (64, 1, 17, 1, (3, 0), "gaussian"),
    (64, 50, "N-1", None, None, "gaussian"),
    (65, 33, 2, 7, (0, 0), "scaled"),
    (65, 50, 17, 64, (3, 1), "gaussian"),
    (65, 128, "N-1", "N", None, "gaussian"),
    (257, 2, 255, None, None, "gaussian"),
    (257, 31, 256, 7, (3, 1), "gaussian"),
    (257, 128, 16, "N", (0, 0), "scaled"),
    (257, 3, 1, 1, (0, 0), "gaussian"),
    (1000, 50, 700, None, None, "gaussian"),
    (1000, 32, 255, 64, (0, 0), "gaussian"),
    (1000, 3, "N-1", 7, (3, 1), "scaled"),
    (1000, 128, 256, "N", None, "gaussian"),
    (1000, 33, 17, 1, (3, 1), "scaled"),
    (3001, 50, 15, None, (0, 0), "gaussian"),
    (3001, 128, 1024, 64, None, "gaussian"),
    (3001, 1, 700, "N", (3, 1), "gaussian"),
    (3001, 32, 1024, None, (0, 0), "scaled"),
    (3001, 2, 16, 7, None, "gaussian"),
    (1000, 4, 15, None, (0, 0), "lattice"),
    (1000, 4, 256, 7, (3, 1), "lattice"),
    (1000, 4, 700, 64, None, "lattice"),
    (1200, 3, 15, None, None, "duplicates"),
    (1200, 50, 64, 7, (3, 1), "duplicates"),
]
# Exact ties that span the select kernel's segments of 1024 candidates: at least 0.30 of the rows of each case below take
# the keys equal to the k-th from a later segment after an earlier one supplied some but not all of them, with more equal
# keys than places (knn_model.tie_spans; tests/test_knn_host.py asserts the shares, and that they are 0 in the four tie cases
# above).  N = 2049 has one candidate in the third segment.
SPANNING_TIE_CASES = [
    (3001, 4, 15, None, (0, 0), "lattice"),
    (3001, 4, 255, 7, (3, 1), "lattice"),
    (3001, 4, 700, 64, None, "lattice"),
    (3001, 4, 1024, "N", (3, 1), "lattice"),
    (2049, 4, 15, None, None, "lattice"),
    (3000, 3, 150, 64, (0, 0), "copies100"),
]
TIE_CASES = [c for c in CASES if c[5] in ("lattice", "duplicates")]
CASES += SPANNING_TIE_CASES


def _input(P, view):
    """The panel as the case passes it: a host array, or a column view of a device tensor."""
    import torch
    if view is None:
        return P
    pad, shift = view
    N, d = P.shape
    wide = np.random.default_rng(5).standard_normal((N, d + pad)).astype(np.float32)
    wide[:, shift:shift + d] = P
    return torch.as_tensor(wide).cuda()[:, shift:shift + d]


@pytest.mark.parametrize("N,d,k,chunk,view,kind", CASES)
def test_bit_for_bit_against_the_model(N, d, k, chunk, view, kind):
    from prosstt_amd import neighbors
    k = N - 1 if k == "N-1" else k
    chunk = N if chunk == "N" else chunk
    P = knn_model.KINDS[kind](N, d, 1000 * N + 10 * d + k)
    assert P.shape == (N, d) and P.dtype == np.float32 and knn_model.no_subnormal_terms(P)
    want_idx, want_d2 = knn_model.model(P, k)
    got = neighbors.knn(_input(P, view), k, chunk_rows=chunk)
    assert got.indices.dtype == np.int32 and got.sq_distances.dtype == np.float32
    np.testing.assert_array_equal(got.indices, want_idx)
    np.testing.assert_array_equal(got.sq_distances.view(np.uint32), want_d2.view(np.uint32))


def test_default_chunks_with_a_ragged_last_one():
    """20 000 x 50, k = 30: the default chunk is 2496 rows, so eight whole chunks and one of 32 rows.  The reference is the
    definition restated in torch on the device, in row blocks of 2000: separate float32 sub, mul and add_ per coordinate,
    self masked, a stable sort (ties to the lower index)."""
    import torch
    from prosstt_amd import neighbors
    N, d, k = 20000, 50, 30
    P = torch.as_tensor(knn_model.gaussian(N, d, 99)).cuda()
    got = neighbors.knn(P, k, out="torch")
    assert got.indices.shape == (N, k) and got.indices.dtype == torch.int32 and got.sq_distances.dtype == torch.float32
    cols = [P[:, c].contiguous() for c in range(d)]
    for lo in range(0, N, 2000):
        hi = min(N, lo + 2000)
        acc = torch.zeros((hi - lo, N), dtype=torch.float32, device="cuda")
        for c in range(d):
            t = torch.sub(cols[c][lo:hi, None], cols[c][None, :])
            t = torch.mul(t, t)
            acc.add_(t)
        acc[torch.arange(hi - lo, device="cuda"), torch.arange(lo, hi, device="cuda")] = float("inf")
        val, order = torch.sort(acc, dim=1, stable=True)
        assert torch.equal(got.indices[lo:hi].long(), order[:, :k]), lo
        assert torch.equal(got.sq_distances[lo:hi].view(torch.int32), val[:, :k].contiguous().view(torch.int32)), lo
        del acc, val, order, t
    torch.cuda.empty_cache()


def test_repeats_and_streams_are_bit_identical():
    import torch
    from prosstt_amd import neighbors
    P = torch.as_tensor(knn_model.gaussian(3001, 50, 17)).cuda()
    first = neighbors.knn(P, 15, out="torch")
    second = neighbors.knn(P, 15, out="torch")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        third = neighbors.knn(P, 15, out="torch", chunk_rows=1000)
    st.synchronize()
    for other in (second, third):
        assert torch.equal(first.indices, other.indices) and torch.equal(first.sq_distances, other.sq_distances)
    host = neighbors.knn(P, 15)
    np.testing.assert_array_equal(host.indices, first.indices.cpu().numpy())
    np.testing.assert_array_equal(host.sq_distances, first.sq_distances.cpu().numpy())
    wide = neighbors.knn(P.double(), 15)                         # float64 holding float32 values: rounded once, the same
    np.testing.assert_array_equal(host.indices, wide.indices)
    np.testing.assert_array_equal(host.sq_distances, wide.sq_distances)


def test_neighbours_of_the_samplers_pca_scores():
    pytest.importorskip("scipy")
    from prosstt_amd import workloads, simulation as sim, embed, neighbors
    work = workloads.build("C2")
    np.random.seed(12)
    presented, pt, br, sc = sim.sample_density(work.tree, 3000, alpha=work.alpha, beta=work.beta, out="torch")
    p = embed.pca(presented, sc, 20)
    nb = neighbors.knn(p.scores, 14)
    want_idx, want_d2 = knn_model.model(p.scores.astype(np.float32), 14)
    np.testing.assert_array_equal(nb.indices, want_idx)
    np.testing.assert_array_equal(nb.sq_distances.view(np.uint32), want_d2.view(np.uint32))
    g = nb.to_csr()
    assert g.shape == (3000, 3000)
    np.testing.assert_array_equal(np.diff(g.indptr), np.full(3000, 14))
    assert np.all(np.diff(g.indices.reshape(3000, 14), axis=1) > 0)


def test_errors_through_the_abi():
    import torch
    from prosstt_amd import _native, neighbors
    from prosstt_amd.device import _ptr
    L = _native.load("knn")
    N, d, k = 100, 5, 3
    P = torch.as_tensor(knn_model.gaussian(N, d, 1)).cuda()
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_knn_workspace_bytes(N, d, k, 0, ctypes.byref(need)), "knn")
    assert need.value >= 4 * N * N
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    index = torch.full((N, k), -7, dtype=torch.int32, device="cuda")
    sqdist = torch.full((N, k), -7.0, dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def search(ld, ws_bytes, n=N, dd=d, kk=k, chunk=0):
        return L.prosstt_amd_knn_search(stream, _ptr(P), n, dd, ld, kk, chunk, _ptr(index), _ptr(sqdist), _ptr(ws), ws_bytes)

    with pytest.raises(_native.NativeError, match="workspace of %d bytes, %d needed" % (need.value - 1, need.value)):
        _native.check(search(d, need.value - 1), "knn")
    with pytest.raises(_native.NativeError, match="row stride 4 is below the row length 5"):
        _native.check(search(d - 1, need.value), "knn")
    for bad in (dict(n=1), dict(dd=0), dict(dd=129), dict(kk=0), dict(kk=N), dict(chunk=-1), dict(chunk=N + 1)):
        with pytest.raises(_native.NativeError, match="need "):
            _native.check(search(d, need.value, **bad), "knn")
    torch.cuda.synchronize()
    assert bool((index == -7).all()) and bool((sqdist == -7.0).all())        # nothing was enqueued
    _native.check(search(d, need.value), "knn")
    want_idx, want_d2 = knn_model.model(P.cpu().numpy(), k)
    np.testing.assert_array_equal(index.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(sqdist.cpu().numpy(), want_d2)
    bad = P.clone()
    bad[17, 2] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        neighbors.knn(bad, k)
    bad[17, 2] = 2.0 ** 59
    with pytest.raises(ValueError, match="finite"):
        neighbors.knn(bad, k)
    with pytest.raises(TypeError, match="float32 or float64"):
        neighbors.knn(P.half(), k)
