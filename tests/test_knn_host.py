"""neighbors.knn without a device: the scalar model (tests/knn_model.py) against a binary64 brute force and on exact ties;
the argument checks that refuse before any device use; Neighbors.distances and to_csr() on a hand-made result."""
import numpy as np
import pytest

import knn_model

torch = pytest.importorskip("torch")

from prosstt_amd import neighbors  # noqa: E402


def test_model_against_binary64():
    N, d, k = 1500, 50, 15
    P = knn_model.gaussian(N, d, 20261018)
    idx, d2 = knn_model.model(P, k)
    ref_idx, ref_d2 = knn_model.brute64(P, k)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == d2.shape == (N, k)
    np.testing.assert_array_equal(idx, ref_idx)
    # d roundings of the sum, one of each square and of each difference (2 per term, relative to the term): below
    # (d + 2) 2^-24 of the sum of non-negative terms
    assert np.all(np.abs(d2.astype(np.float64) - ref_d2) <= (d + 2) * 2.0 ** -24 * ref_d2)
    assert np.all(np.diff(d2, axis=1) >= 0) and not np.any(idx == np.arange(N)[:, None])


def test_model_resolves_ties_to_the_lower_index():
    N, k = 1000, 15
    P = knn_model.lattice(N, 7)
    idx, d2 = knn_model.model(P, k)
    full = ((P[:, None, :].astype(np.float64) - P[None, :, :]) ** 2).sum(axis=2)     # small integers: exact
    tied = 0
    for i in range(N):
        row = full[i].copy()
        row[i] = np.inf
        kth = np.sort(row)[k - 1]
        tied += int(np.sort(row)[k] == kth)
        below = np.flatnonzero(row < kth)
        equal = np.flatnonzero(row == kth)[:k - below.size]          # the lowest indices among the tied
        want = np.concatenate([below, equal])
        want = want[np.lexsort((want, row[want]))]
        np.testing.assert_array_equal(idx[i], want)
        np.testing.assert_array_equal(d2[i], row[want].astype(np.float32))
    assert tied > N // 2, tied


def test_which_tie_cases_span_the_select_kernels_segments():
    """The share of rows whose keys equal to the k-th come from more than one segment of 1024 candidates, the later one
    after 0 < ties so far < need, while ties are cut at k: at least 0.30 in every case added for it (the smallest measured
    was 0.37, lattice at N = 3001 and k = 255), and 0 in the four tie cases from before, which fit their ties into one
    segment or cross none: they stay as small inputs and test_gpu_knn.SPANNING_TIE_CASES carry the running count."""
    import test_gpu_knn
    assert len(test_gpu_knn.TIE_CASES) == 5 and len(test_gpu_knn.SPANNING_TIE_CASES) == 6
    for cases, spanning in ((test_gpu_knn.SPANNING_TIE_CASES, True), (test_gpu_knn.TIE_CASES, False)):
        for N, d, k, _, _, kind in cases:
            P = knn_model.KINDS[kind](N, d, 1000 * N + 10 * d + k)
            crosses, cut = knn_model.tie_spans(P, k)
            share = float(np.mean(crosses & cut))
            print("%s N = %d, k = %d: %.3f of the rows cross a segment with ties cut at k" % (kind, N, k, share))
            assert cut.any()
            assert share >= 0.30 if spanning else share == 0.0, (N, d, k, kind, share)


def test_tie_spans_on_a_hand_made_row():
    # candidates on a line seen from cell 0, in segments of three: (self), 1, 1 | 4, 4, 4 | 4, 4, 9
    P = np.array([[0], [1], [-1], [2], [-2], [2], [-2], [2], [3]], dtype=np.float32)
    for k, crosses, cut in ((2, False, False), (3, False, True), (4, False, True), (5, False, True), (6, True, True),
                            (7, True, False), (8, False, False)):
        got = knn_model.tie_spans(P, k, seg=3)
        assert (bool(got[0][0]), bool(got[1][0])) == (crosses, cut), k
    assert not knn_model.tie_spans(P, 6, seg=1024)[0].any()


def test_symmetric_bits():
    P = knn_model.scaled(300, 33, 3)
    idx, d2 = knn_model.model(P, 299)
    full = np.empty((300, 300), np.float32)
    np.put_along_axis(full, idx, d2, axis=1)
    np.fill_diagonal(full, 0)
    np.testing.assert_array_equal(full.view(np.uint32), full.T.view(np.uint32))
    assert knn_model.no_subnormal_terms(P)


def test_refusals_before_any_device_use():
    P = knn_model.gaussian(20, 5, 1)
    with pytest.raises(TypeError, match="floating"):
        neighbors.knn(P.astype(np.int32), 3)
    with pytest.raises(TypeError, match="floating"):
        neighbors.knn(torch.ones((20, 5), dtype=torch.int64), 3)
    with pytest.raises(ValueError, match="dimensions"):
        neighbors.knn(P[0], 3)
    with pytest.raises(ValueError, match="dimensions"):
        neighbors.knn(P.reshape(2, 10, 5), 3)
    with pytest.raises(ValueError, match="cells"):
        neighbors.knn(P[:1], 1)
    with pytest.raises(ValueError, match="coordinates"):
        neighbors.knn(np.zeros((20, 0), np.float32), 3)
    with pytest.raises(ValueError, match="coordinates"):
        neighbors.knn(np.zeros((20, 129), np.float32), 3)
    for k in (0, -1, 20, 2.5):
        with pytest.raises(ValueError, match="n_neighbors"):
            neighbors.knn(P, k)
    with pytest.raises(ValueError, match="n_neighbors"):
        neighbors.knn(np.zeros((2000, 2), np.float32), 1025)
    with pytest.raises(ValueError, match="out must be"):
        neighbors.knn(P, 3, out="csr")
    for chunk in (0, 21, 1.5):
        with pytest.raises(ValueError, match="chunk_rows"):
            neighbors.knn(P, 3, chunk_rows=chunk)
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 59, -2.0 ** 60):
        Q = P.astype(np.float64)
        Q[7, 2] = bad
        with pytest.raises(ValueError, match="finite"):
            neighbors.knn(Q, 3)
        with pytest.raises(ValueError, match="finite"):
            neighbors.knn(torch.as_tensor(Q), 3)                  # a CPU tensor is a host array


def test_neighbors_result():
    pytest.importorskip("scipy")
    idx = np.array([[2, 1], [0, 3], [3, 0], [2, 1]], dtype=np.int32)
    d2 = np.array([[0.0, 4.0], [4.0, 9.0], [0.25, 0.25], [0.25, 16.0]], dtype=np.float32)
    nb = neighbors.Neighbors(idx, d2)
    assert nb.indices is idx and nb.sq_distances is d2
    dist = nb.distances
    assert dist.dtype == np.float64
    np.testing.assert_array_equal(dist, [[0.0, 2.0], [2.0, 3.0], [0.5, 0.5], [0.5, 4.0]])
    g = nb.to_csr()
    assert g.shape == (4, 4) and g.dtype == np.float64 and g.nnz == 8
    np.testing.assert_array_equal(g.indptr, [0, 2, 4, 6, 8])
    np.testing.assert_array_equal(g.indices, [1, 2, 0, 3, 0, 3, 1, 2])
    np.testing.assert_array_equal(g.data, [2.0, 0.0, 2.0, 3.0, 0.5, 0.5, 4.0, 0.5])
    t = neighbors.Neighbors(torch.as_tensor(idx), torch.as_tensor(d2))               # tensors: the same graph
    assert t.distances.dtype == torch.float64
    assert (t.to_csr() != g).nnz == 0
