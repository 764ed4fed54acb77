"""prosstt_amd.autocorr on the host: every refusal of ``graph_sums`` and ``smooth`` that comes before a device is used (this
file runs where there is none), and the graph's constants."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import autocorr_model as am  # noqa: E402
from prosstt_amd import autocorr, graph  # noqa: E402

N, G = 12, 5


def _inputs():
    """A CPU int32 tensor (refused last of all, as "not on a device"), size factors and a path graph of N cells."""
    X = torch.zeros((N, G), dtype=torch.int32)
    s = np.full(N, 1.5)
    return X, s, graph.Connectivities(*am.path_graph(N), None, None)


CALLS = [autocorr.graph_sums, autocorr.smooth]


@pytest.mark.parametrize("call", CALLS)
def test_count_inputs_are_refused(call):
    X, s, g = _inputs()
    with pytest.raises(TypeError, match="host arrays are refused"):
        call(X.numpy(), s, g)
    with pytest.raises(TypeError, match="int32"):
        call(X.to(torch.int64), s, g)
    with pytest.raises(TypeError, match="int32"):
        call(X.to(torch.float32), s, g)
    with pytest.raises(ValueError, match="dimensions"):
        call(X[0], s, g)
    with pytest.raises(ValueError, match="at least one cell"):
        call(X[:0], s, g)
    with pytest.raises(ValueError, match="device tensor"):            # everything else is in order: the CPU tensor itself
        call(X, s, g)


@pytest.mark.parametrize("call", CALLS)
def test_size_factors_are_refused(call):
    X, s, g = _inputs()
    for bad in (s[:-1], np.zeros(N), -s, np.full(N, np.inf), np.full(N, np.nan), np.full(N, 1e-40), np.full(N, 2.0 ** 127)):
        with pytest.raises(ValueError, match="size factor"):
            call(X, bad, g)


@pytest.mark.parametrize("call", CALLS)
def test_graphs_are_refused(call):
    X, s, g = _inputs()
    indptr, indices, data = g.indptr, g.indices, g.data
    other = graph.Connectivities(*am.path_graph(N + 1), None, None)
    with pytest.raises(ValueError, match="the graph has %d cells, the matrix %d" % (N + 1, N)):
        call(X, s, other)
    with pytest.raises(ValueError, match="the graph has"):              # a Transitions is read the same way
        call(X, s, graph.Transitions(*am.path_graph(N + 1), None, None))
    for bad, text in ((g._replace(indptr=indptr.astype(np.int32)), "indptr"), (g._replace(indices=indices.astype(np.int64)), "indices"),
                      (g._replace(data=data.astype(np.float32)), "data"), (g._replace(data=data[:-1]), "differ in length"),
                      (g._replace(indptr=indptr[:1]), "the graph has|at least two"), (g._replace(data=data.reshape(2, -1)), "data"),
                      (g._replace(indices=list(indices)), "indices")):
        with pytest.raises(ValueError, match=text):
            call(X, s, bad)
    # a graph whose arrays lie on another device than the matrix
    meta = graph.Connectivities(*(torch.as_tensor(a).to("meta") for a in (indptr, indices, data)), None, None)
    with pytest.raises(ValueError, match="the graph lies on meta, the matrix on cpu"):
        call(X, s, meta)
    # neighbours: what graph.connectivities refuses, and another number of cells
    idx = np.zeros((N + 2, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="the graph has %d cells" % (N + 2)):
        call(X, s, (idx, np.zeros((N + 2, 3), dtype=np.float32)))
    with pytest.raises(ValueError, match="int32"):
        call(X, s, (idx.astype(np.int64), np.zeros((N + 2, 3), dtype=np.float32)))
    with pytest.raises(ValueError, match="Neighbors"):
        call(X, s, 5)


def test_options_are_refused():
    X, s, g = _inputs()
    for bad in (-1, 1.5, "4", 1 << 31, None):
        with pytest.raises(ValueError, match="rows_per_block"):
            autocorr.graph_sums(X, s, g, rows_per_block=bad)
    for call in CALLS:
        for bad in ("scipy", None, 1):
            with pytest.raises(ValueError, match="out must be"):
                call(X, s, g, out=bad)
        for bad in (1, 128, True, "64"):
            with pytest.raises(ValueError, match="gene_tile"):
                call(X, s, g, gene_tile=bad)
    for bad in (np.zeros(G + 1), np.full(G, np.nan), np.zeros((G, 1))):
        with pytest.raises(ValueError, match="mean"):
            autocorr.graph_sums(X, s, g, mean=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="normalize"):
            autocorr.smooth(X, s, g, normalize=bad)
    for bad in (0, G + 1, 2.5):
        with pytest.raises(ValueError, match="n_genes"):
            autocorr.autocorrelation(X, s, g, bad)


def test_graph_constants():
    rng = np.random.default_rng(0)
    W = np.where(rng.random((9, 9)) < 0.4, rng.uniform(0.1, 2.0, size=(9, 9)), 0.0)       # asymmetric, with a diagonal
    got = autocorr.graph_constants(*am.csr_of(W))
    np.testing.assert_allclose(got, am.graph_constants(W), rtol=1e-14)
    as_tensors = autocorr.graph_constants(*(torch.as_tensor(a) for a in am.csr_of(W)))
    assert as_tensors == got
