"""tests/cluster_model.py, the numpy model of prosstt_amd.cluster, against networkx's Louvain and modularity and against its
own definition.  No GPU.

Measured with this model (networkx 3.4.2, seeds 0, 1, 2 of louvain_communities), Q and the deficit to the lowest seed:
(300, 5) 0.8396, 0.0025; (1000, 14) 0.8314, -0.0017; (2000, 14) 0.8381, -0.0005; (1000, 14) at gamma 0.5 0.8855, -0.0027; at
gamma 2 0.7553, -0.0041.  The model's exact Q differs from networkx.community.modularity on the unquantised W by at most
1.4e-12 on these graphs."""
import functools

import numpy as np
import pytest

nx = pytest.importorskip("networkx")
sparse = pytest.importorskip("scipy.sparse")

import cluster_model as cm  # noqa: E402
import graph_model  # noqa: E402

QUALITY_CASES = [(300, 5, 1.0), (1000, 14, 1.0), (2000, 14, 1.0), (1000, 14, 0.5), (1000, 14, 2.0)]
SLACK = 0.02


@functools.lru_cache(maxsize=None)
def _case(N, k, gamma):
    """(W, its networkx graph, the model's result, networkx's partitions of seeds 0, 1, 2)."""
    W = graph_model.case(N, k)["W"]
    G = nx.from_scipy_sparse_array(W)
    parts = tuple(nx.community.louvain_communities(G, resolution=gamma, seed=s) for s in (0, 1, 2))
    return W, G, cm.louvain(W, gamma), parts


def _communities(labels):
    return [set(np.flatnonzero(labels == a).tolist()) for a in np.unique(labels)]


def _labels(parts, N):
    labels = np.empty(N, dtype=np.int64)
    for a, members in enumerate(parts):
        labels[list(members)] = a
    return labels


@pytest.mark.parametrize("N,k,gamma", QUALITY_CASES)
def test_exact_modularity_against_networkx(N, k, gamma):
    W, G, res, parts = _case(N, k, gamma)
    bound = 3 * W.nnz * 2.0 ** -33 / W.sum()                 # the quantisation's: every weight moves by at most 2^-33
    assert bound < 2e-9
    worst = 0.0
    for labels in [res.labels] + [_labels(p, N) for p in parts]:
        got = cm.modularity(W, labels, gamma)
        want = nx.community.modularity(G, _communities(labels), resolution=gamma)
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= bound
    assert cm.modularity(W, res.labels, gamma) == res.modularity      # the last accepted Q is the Q of the labels
    print("(%d, %d) gamma %g: max |Q - networkx's| = %.2e (bound %.2e)" % (N, k, gamma, worst, bound))


@pytest.mark.parametrize("N,k,gamma", QUALITY_CASES)
def test_quality_is_networkx_louvains(N, k, gamma):
    W, G, res, parts = _case(N, k, gamma)
    theirs = [nx.community.modularity(G, p, resolution=gamma) for p in parts]
    print("(%d, %d) gamma %g: Q = %.4f, networkx %s, deficit %.4f" % (N, k, gamma, res.modularity,
                                                                     ["%.4f" % q for q in theirs], min(theirs) - res.modularity))
    assert res.modularity >= min(theirs) - SLACK


def test_the_levels_of_a_small_case_are_pinned():
    res = _case(300, 5, 1.0)[2]
    assert [(n, m, rounds) for n, m, rounds, _ in res.levels] == [(300, 35, 8), (35, 14, 3), (14, 14, 0)]
    assert len(res.sizes) == 14 and res.sizes.sum() == 300
    assert len(res.level_labels) == 3 and [int(l.max()) + 1 for l in res.level_labels] == [35, 14, 14]
    # a coarser level only merges the communities of the finer one
    fine, coarse = res.level_labels[0], res.level_labels[1]
    assert len(set(zip(fine.tolist(), coarse.tolist()))) == 35
    assert np.array_equal(cm.order_labels(res.level_labels[-1])[0], res.labels)


@pytest.mark.parametrize("N,k,gamma", QUALITY_CASES[:2])
def test_q_increases_strictly_with_every_accepted_round(N, k, gamma):
    res = _case(N, k, gamma)[2]
    flat = [q for trace in res.trace for q in trace]
    assert len(flat) == sum(rounds for _, _, rounds, _ in res.levels)
    assert all(b > a + 1e-7 for a, b in zip(flat, flat[1:]))
    assert flat[-1] == res.modularity
    for (_, _, rounds, Q), trace in zip(res.levels, res.trace):
        assert len(trace) == rounds and (not trace or trace[-1] == Q)


def _ring_of_cliques(cliques=6, size=8, bridge=0.1):
    n = cliques * size
    A = np.zeros((n, n))
    for q in range(cliques):
        A[q * size:(q + 1) * size, q * size:(q + 1) * size] = 1.0
        a, b = q * size + size - 1, ((q + 1) % cliques) * size
        A[a, b] = A[b, a] = bridge
    np.fill_diagonal(A, 0.0)
    return sparse.csr_matrix(A)


def test_a_ring_of_cliques_is_recovered_in_one_level():
    res = cm.louvain(_ring_of_cliques())
    assert np.array_equal(res.labels, np.repeat(np.arange(6), 8))     # equal sizes: numbered by their first cell
    assert res.sizes.tolist() == [8] * 6
    assert [(n, m) for n, m, _, _ in res.levels] == [(48, 6), (6, 6)]


def test_components_never_share_a_label():
    a, b = graph_model.case(300, 5)["W"], graph_model.case(64, 5)["W"]
    W = sparse.block_diag([a, b], format="csr")
    W.sort_indices()
    res = cm.louvain(W)
    assert not set(res.labels[:300]) & set(res.labels[300:])
    for labels in res.level_labels:
        assert not set(labels[:300]) & set(labels[300:])


def test_the_order_of_the_labels():
    labels, sizes = cm.order_labels(np.array([7, 7, 3, 3, 9, 9, 9, 0]))
    assert labels.tolist() == [1, 1, 2, 2, 0, 0, 0, 3] and sizes.tolist() == [3, 2, 2, 1]       # 7 before 3: it holds cell 0
    for N, k, gamma in QUALITY_CASES[:2]:
        res = _case(N, k, gamma)[2]
        assert np.all(np.diff(res.sizes) <= 0) and np.array_equal(np.bincount(res.labels), res.sizes)
        for a in range(len(res.sizes) - 1):
            if res.sizes[a] == res.sizes[a + 1]:
                assert np.flatnonzero(res.labels == a)[0] < np.flatnonzero(res.labels == a + 1)[0]


def test_a_sweep_against_a_loop_over_the_definition():
    """The vectorised sweep against the definition written as plain loops over Python integers and floats."""
    for level in (cm.hand_built(130, (1 << 47) + 1, True)[0], cm.quantize(graph_model.case(64, 5)["W"]), cm.tie_graph()):
        n = level.n
        for c in (np.arange(n), np.arange(n) % 3, (np.arange(n) * 7919) % min(n, 40)):
            tot, inn = cm.totals(level, c)
            assert int(tot.sum()) == level.M2 and int(inn.sum()) <= level.M2
            for parity in (0, 1):
                got, moved = cm.sweep(level, c, tot, parity, 1.0)
                want = c.copy()
                for i in range(n):
                    e = {}
                    for p in range(level.indptr[i], level.indptr[i + 1]):
                        j = int(level.indices[p])
                        if j != i:
                            e[int(c[j])] = e.get(int(c[j]), 0) + int(level.u[p])
                    ki, ci = int(level.k[i]), int(c[i])

                    def g(ee, T):
                        return float(ee) - (1.0 * (float(ki) * float(T))) / float(level.M2)
                    best = None
                    for d in sorted(e):
                        if d != ci and (d < ci if parity == 0 else d > ci):
                            if best is None or g(e[d], int(tot[d])) > best[0]:
                                best = (g(e[d], int(tot[d])), d)
                    if best is not None and best[0] > g(e.get(ci, 0), int(tot[ci]) - ki):
                        want[i] = best[1]
                assert np.array_equal(got, want) and moved == int((want != c).sum())


def test_aggregation_keeps_every_weight():
    level = cm.quantize(graph_model.case(300, 14)["W"])
    c = (np.arange(300) * 7919) % 25
    nxt, cp = cm.aggregate(level, c)
    assert nxt.n == 25 and nxt.M2 == level.M2 and np.array_equal(cp, np.searchsorted(np.unique(c), c))
    tot, inn = cm.totals(level, c)
    assert np.array_equal(nxt.k, tot[np.unique(c)])
    dense = sparse.csr_matrix((nxt.u.astype(np.float64), nxt.indices, nxt.indptr), shape=(25, 25)).toarray()
    assert np.array_equal(dense, dense.T) and np.array_equal(np.diag(dense), inn[np.unique(c)].astype(np.float64))
    assert all(np.all(np.diff(nxt.indices[nxt.indptr[a]:nxt.indptr[a + 1]]) > 0) for a in range(25))
    one, _ = cm.aggregate(level, np.zeros(300, dtype=np.int64))
    assert one.n == 1 and one.u.tolist() == [level.M2] and one.indices.tolist() == [0]
