"""prosstt_amd.cluster without a device: the argument checks that refuse before any device use, the order of the labels and
the quality sum."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

import cluster_model as cm  # noqa: E402
from prosstt_amd import cluster, device, graph, neighbors  # noqa: E402


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the loader of every library and torch's own switch."""
    def reached(*args, **kwargs):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(device, "need_device", reached)
    monkeypatch.setattr(graph, "_on_device", reached)


def _nb(n=20, k=3):
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)
    return neighbors.Neighbors(idx, rng.random((n, k)).astype(np.float32))


def _conn(n=20):
    return graph.Connectivities(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64), None, None)


def test_louvain_refusals_before_any_device_use(no_device):
    nb = _nb()
    with pytest.raises(ValueError, match="pair"):
        cluster.louvain(nb.indices)
    with pytest.raises(ValueError, match="indices must be int32"):
        cluster.louvain(neighbors.Neighbors(nb.indices.astype(np.int64), nb.sq_distances))
    with pytest.raises(ValueError, match="neighbours"):
        cluster.louvain(neighbors.Neighbors(nb.indices[:, :1], nb.sq_distances[:, :1]))
    with pytest.raises(ValueError, match="must be a 1-D"):
        cluster.louvain(_conn()._replace(indptr=np.zeros(21, np.int32)))
    with pytest.raises(ValueError, match="cells"):
        cluster.louvain(_conn(2))
    for bad in (0, -1.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="resolution"):
            cluster.louvain(nb, bad)
        with pytest.raises(ValueError, match="resolution"):
            cluster.modularity(nb, np.zeros(20), bad)
    for bad in (-1e-9, float("inf"), float("nan"), "small", None):
        with pytest.raises(ValueError, match="tol"):
            cluster.louvain(nb, tol=bad)
    for name in ("max_rounds", "max_levels"):
        for bad in (0, -1, 2.5, "many", None, True):
            with pytest.raises(ValueError, match=name):
                cluster.louvain(nb, **{name: bad})
    for bad in (-1, 5, 1.5, "0", None, True):
        with pytest.raises(ValueError, match="path"):
            cluster.louvain(nb, path=bad)
    with pytest.raises(ValueError, match="out must be"):
        cluster.louvain(nb, out="scipy")


def test_modularity_refusals_before_any_device_use(no_device):
    nb = _nb()
    for labels in (np.zeros(19), np.zeros(21), np.zeros((20, 1)), 3):
        with pytest.raises(ValueError, match="one label per cell"):
            cluster.modularity(nb, labels)
    with pytest.raises(ValueError, match="one label per cell"):
        cluster.modularity(_conn(), np.zeros(5))
    with pytest.raises(ValueError, match="must be a 1-D"):
        cluster.modularity(_conn()._replace(data=np.zeros(0, np.float32)), np.zeros(20))


def test_level_graph_argument_checks(no_device):
    indptr, indices, u = np.array([0, 1, 2], np.int64), np.array([1, 0], np.int32), np.array([5, 5], np.int64)
    for bad in (dict(indptr=indptr.astype(np.int32)), dict(indices=indices.astype(np.int64)), dict(u=u.astype(np.float64)),
                dict(u=u.astype(np.int32)), dict(indptr=indptr[None]), dict(indices=[1, 0]),
                dict(indptr=torch.from_numpy(indptr).to(torch.int32))):
        kw = dict(indptr=indptr, indices=indices, u=u)
        kw.update(bad)
        with pytest.raises(ValueError, match="must be a 1-D"):
            cluster.LevelGraph.from_csr(**kw)
    with pytest.raises(ValueError, match="nodes"):
        cluster.LevelGraph.from_csr(indptr[:1], indices, u)
    with pytest.raises(ValueError, match="differ in length"):
        cluster.LevelGraph.from_csr(indptr, indices, u[:1])
    with pytest.raises(ValueError, match="stored entries"):
        cluster.LevelGraph.from_csr(np.zeros(3, np.int64), indices[:0], u[:0])
    host = cluster.LevelGraph(indptr, indices, u, u, 10, None, (2, 2, 2))          # host arrays: no device graph
    for call in (lambda: cluster.sweep(host, np.zeros(2, np.int32), 0), lambda: cluster.totals(host, np.zeros(2, np.int32)),
                 lambda: cluster.aggregate(host, np.zeros(2, np.int32)), lambda: cluster.sweep("graph", [0, 0], 0)):
        with pytest.raises(ValueError, match="LevelGraph of device tensors"):
            call()
    with pytest.raises(ValueError, match="parity"):
        cluster.sweep(host, np.zeros(2, np.int32), 2)
    with pytest.raises(ValueError, match="path"):
        cluster.sweep(host, np.zeros(2, np.int32), 0, 1.0, 7)
    with pytest.raises(ValueError, match="resolution"):
        cluster.sweep(host, np.zeros(2, np.int32), 0, 0.0)


def test_the_order_of_the_labels():
    labels, sizes = cluster.order_labels(np.array([5, 5, 2, 2, 9, 9, 9, 1]))
    assert labels.dtype == np.int32 and sizes.dtype == np.int64
    assert labels.tolist() == [1, 1, 2, 2, 0, 0, 0, 3] and sizes.tolist() == [3, 2, 2, 1]       # 5 before 2: it holds cell 0
    labels, sizes = cluster.order_labels(np.array([3, 1, 2, 0]))                                 # all equal: by first cell
    assert labels.tolist() == [0, 1, 2, 3] and sizes.tolist() == [1, 1, 1, 1]
    labels, sizes = cluster.order_labels(np.zeros(4, dtype=np.int32))
    assert labels.tolist() == [0, 0, 0, 0] and sizes.tolist() == [4]
    rng = np.random.default_rng(0)
    comm = rng.integers(0, 12, 200) * 17
    labels, sizes = cluster.order_labels(comm)
    want, want_sizes = cm.order_labels(comm)
    assert np.array_equal(labels, want) and np.array_equal(sizes, want_sizes)
    assert np.all(np.diff(sizes) <= 0) and np.array_equal(np.bincount(labels), sizes)
    for a in range(len(sizes) - 1):
        if sizes[a] == sizes[a + 1]:
            assert np.flatnonzero(labels == a)[0] < np.flatnonzero(labels == a + 1)[0]
    for bad in (np.zeros((2, 2)), np.zeros(0)):
        with pytest.raises(ValueError):
            cluster.order_labels(bad)


def test_the_quality_sum_is_the_models():
    rng = np.random.default_rng(1)
    tot = rng.integers(0, 1 << 58, 50)
    inn = rng.integers(0, 1 << 57, 50)
    M2 = int(tot.sum())
    for gamma in (0.5, 1.0, 2.0):
        assert cluster.quality(tot, inn, M2, gamma) == cm.quality(tot, inn, M2, gamma)
    assert cluster.quality(np.array([M2]), np.array([M2]), M2, 1.0) == 0.0                       # one community: 1 - 1
