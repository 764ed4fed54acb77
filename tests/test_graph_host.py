"""prosstt_amd.graph without a device: the argument checks that refuse before any device use; the binary64 model
(tests/graph_model.py) against its own definitions on the (300, 5, 5) test cloud."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

import graph_model  # noqa: E402
from prosstt_amd import graph, neighbors  # noqa: E402

N, D, K = 300, 5, 5


@pytest.fixture(scope="module")
def cloud():
    return graph_model.case(N, K, D)


def _nb(n=20, k=3):
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)
    return neighbors.Neighbors(idx, rng.random((n, k)).astype(np.float32))


def test_neighbour_refusals_before_any_device_use():
    nb = _nb()
    calls = (graph.connectivities, graph.diffmap, graph.transitions)
    for call in calls:
        with pytest.raises(ValueError, match="pair"):
            call(nb.indices)
        with pytest.raises(ValueError, match="indices must be int32"):
            call(neighbors.Neighbors(nb.indices.astype(np.int64), nb.sq_distances))
        with pytest.raises(ValueError, match="indices must be int32"):
            call(neighbors.Neighbors(torch.as_tensor(nb.indices).long(), torch.as_tensor(nb.sq_distances)))
        with pytest.raises(ValueError, match="sq_distances must be float32"):
            call(neighbors.Neighbors(nb.indices, nb.sq_distances.astype(np.float64)))
        with pytest.raises(ValueError, match="dimensions"):
            call(neighbors.Neighbors(nb.indices[0], nb.sq_distances[0]))
        with pytest.raises(ValueError, match="differ in shape"):
            call(neighbors.Neighbors(nb.indices, nb.sq_distances[:, :2]))
        with pytest.raises(ValueError, match="cells"):
            call(neighbors.Neighbors(nb.indices[:2, :1], nb.sq_distances[:2, :1]))
        with pytest.raises(ValueError, match="neighbours"):
            call(neighbors.Neighbors(nb.indices[:, :1], nb.sq_distances[:, :1]))               # k = 1
        with pytest.raises(ValueError, match="neighbours"):
            call(neighbors.Neighbors(nb.indices[:3], nb.sq_distances[:3]))                     # k = N
        with pytest.raises(ValueError, match="neighbours"):
            call(neighbors.Neighbors(np.zeros((2000, 1025), np.int32), np.zeros((2000, 1025), np.float32)))
    with pytest.raises(ValueError, match="out must be"):
        graph.connectivities(nb, out="numpy")
    with pytest.raises(ValueError, match="out must be"):
        graph.diffmap(nb, 3, out="scipy")


def test_diffmap_refusals_before_any_device_use():
    nb = _nb()
    for n_comps in (0, -1, 20, 21, 2.5):
        with pytest.raises(ValueError, match="n_comps"):
            graph.diffmap(nb, n_comps)
    for tol in (0, -1e-10, float("inf"), float("nan"), "tight"):
        with pytest.raises(ValueError, match="tol"):
            graph.diffmap(nb, 3, tol=tol)
    for seed in (-1, 0.5):
        with pytest.raises(ValueError, match="seed"):
            graph.diffmap(nb, 3, seed=seed)
    for max_steps in (0, 2, 7.5):
        with pytest.raises(ValueError, match="max_steps"):
            graph.diffmap(nb, 3, max_steps=max_steps)
    with pytest.raises(ValueError, match="lanes_per_row"):
        graph.spmv(None, None, lanes_per_row=8)
    # a Connectivities is checked for dtypes and shapes on the host too
    good = graph.Connectivities(np.zeros(21, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64), None, None)
    for field, bad in (("indptr", np.zeros(21, np.int32)), ("indices", np.zeros(0, np.int64)),
                       ("data", np.zeros(0, np.float32)), ("indptr", np.zeros((21, 1), np.int64)),
                       ("indptr", np.zeros(3, np.int64)), ("data", np.zeros(4, np.float64))):
        with pytest.raises(ValueError, match="must be a 1-D|cells|differ in length"):
            graph.diffmap(good._replace(**{field: bad}), 3)


def test_model_connectivities_are_symmetric_to_the_bit(cloud):
    W = cloud["W"]
    assert W.data.dtype == np.float64 and W.shape == (N, N)       # (scipy keeps both index arrays in one type of its choice)
    dense = W.toarray()
    np.testing.assert_array_equal(dense.view(np.uint64), dense.T.copy().view(np.uint64))
    assert not np.any(np.diag(dense))
    per_row = np.diff(W.indptr)
    assert per_row.min() >= K and per_row.max() <= N - 1
    for i in range(N):
        cols = W.indices[W.indptr[i]:W.indptr[i + 1]]
        assert np.all(np.diff(cols) > 0), i
    # every directed membership is there, and W = a + b - a b of the two directions
    a, _, _ = graph_model.memberships(cloud["d2"])
    A = np.zeros((N, N))
    np.put_along_axis(A, cloud["idx"].astype(np.int64), a, axis=1)
    np.testing.assert_array_equal(dense != 0, (A != 0) | (A.T != 0))
    np.testing.assert_allclose(dense, A + A.T - A * A.T, rtol=0, atol=2.0 ** -52)


def test_model_sigma_solves_its_equation(cloud):
    d = np.sqrt(cloud["d2"].astype(np.float64))
    rho, sigma = cloud["rho"], cloud["sigma"]
    np.testing.assert_array_equal(rho, d.min(axis=1))              # no zero distance in this cloud
    free = sigma > 1e-3 * d.mean(axis=1)                           # the floor is inactive
    assert free.sum() > N // 2
    f = graph_model.f_of_sigma(cloud["d2"], rho, sigma)
    assert np.all(np.abs(f[free] - np.log2(K + 1)) <= 1e-12)


def test_model_transitions_fix_z(cloud):
    T, z = cloud["T"], cloud["z"]
    dense = T.toarray()
    np.testing.assert_array_equal(dense.view(np.uint64), dense.T.copy().view(np.uint64))
    assert np.all(np.abs(T @ z - z) <= 1e-13)
    assert np.array_equal(T.indices, cloud["W"].indices) and np.array_equal(T.indptr, cloud["W"].indptr)


def test_model_lanczos_reproduces_dense_eigh(cloud):
    T = cloud["T"]
    lam, vec = graph_model.dense_spectrum(T)
    assert np.min(-np.diff(np.sort(lam[:16])[::-1])) >= 2e-5
    want_values, want_vectors = graph_model.leading(lam, vec, 15)
    values, vectors, steps, residuals = graph_model.lanczos(T, 15)
    assert steps <= 128 and np.all(residuals < 1e-10)
    assert np.all(np.abs(values - want_values) <= 1e-12)
    assert np.all(np.diff(values) < 0) and abs(values[0] - 1) <= 1e-12
    # eigenvectors: sin of the angle to dense eigh's, and the sign rule
    cosines = np.abs(np.sum(vectors * want_vectors, axis=0))
    assert np.all(np.sqrt(np.maximum(1 - cosines ** 2, 0)) <= 1e-6)
    first = np.argmax(np.abs(vectors), axis=0)
    assert np.all(vectors[first, np.arange(15)] > 0)
    assert np.all(np.linalg.norm(T @ vectors - vectors * values, axis=0) <= 1e-10)
