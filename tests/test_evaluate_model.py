"""The numpy model of the evaluate library (tests/evaluate_model.py) and the host statistics of prosstt_amd/evaluate.py
against outside libraries: Kendall's tau-b and Pearson's r of scipy, the shortest paths of scipy's csgraph on the node graph
of three trees, scikit-learn's adjusted Rand index and normalised mutual information, and the permutation search of
tests/ptree_quality.py.  No GPU.

The bounds.  tau-b: both routes divide exact integers by square roots in binary64, scipy's with five roundings and ours with
three, each of relative size 2^-53, on a value of at most 1: 1e-15 holds eight of them.  Pearson: scipy centres and sums about
2 000 pair distances in binary64, an error of at most n 2^-53 = 2.3e-13 relative per sum, three sums: 1e-11.  ARI and NMI:
sums of at most 36 terms in binary64 on values of at most 1: 1e-12.  The accuracy is a count divided by N on both routes:
equal."""
import numpy as np
import pytest
import scipy.sparse
import scipy.sparse.csgraph
import scipy.stats

import evaluate_model as em
import ptree_quality

from prosstt_amd import evaluate

CHAIN = dict(topology=[["A", "B"], ["B", "C"]], time={"A": 5, "B": 3, "C": 4}, branches=["A", "B", "C"])
FORK = dict(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, branches=["A", "B", "C"])        # smoke()'s
TWO_LEVEL = dict(topology=[["A", "B"], ["A", "C"], ["B", "D"], ["B", "E"], ["C", "F"], ["C", "G"]],
                 time={"A": 4, "B": 3, "C": 5, "D": 2, "E": 6, "F": 1, "G": 3}, branches=list("ABCDEFG"))
TREES = {"chain": CHAIN, "fork": FORK, "two levels": TWO_LEVEL}


def _counts_of(a, b, classes, K):
    order, offsets = em.by_class(classes, K)
    c = em.pair_counts(np.asarray(a)[order], np.asarray(b)[order], offsets)
    return evaluate.PairCounts(c[..., 0], c[..., 1], c[..., 2], c[..., 3], em.pairs(offsets))


def test_tau_b_of_the_counts_is_scipys_on_tied_values():
    rng = np.random.default_rng(700)
    a, b = rng.integers(0, 40, 700), rng.integers(0, 25, 700)
    b[:300] = a[:300] // 2                                         # some agreement
    classes = rng.integers(0, 4, 700)
    pc = _counts_of(a, b, classes, 4)
    want = scipy.stats.kendalltau(a, b).statistic
    assert abs(pc.tau_b() - want) <= 1e-15
    # one class: the same pairs in one set
    assert abs(_counts_of(a, b, np.zeros(700, dtype=int), 1).tau_b() - want) <= 1e-15
    # per class pair: the diagonal sets are the classes on their own
    for k in range(4):
        sel = classes == k
        one = np.zeros((4, 4), dtype=bool)
        one[k, k] = True
        assert abs(pc.tau_b(one) - scipy.stats.kendalltau(a[sel], b[sel]).statistic) <= 1e-15
    # the identities of the header
    n = 700 * 699 // 2
    assert int(pc.pairs.sum()) == n
    ties_a = n - sum(int(v) for v in pc.a2.ravel())
    assert ties_a == sum(int(c) * (int(c) - 1) // 2 for c in np.bincount(a))
    assert np.array_equal(pc.concordant() + pc.discordant(), pc.p) and np.array_equal(pc.concordant() - pc.discordant(), pc.s)


def test_gamma_and_tau_a_against_a_direct_count():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 6, 300), rng.integers(0, 6, 300)
    classes = rng.integers(0, 3, 300)
    pc = _counts_of(a, b, classes, 3)
    assert pc.gamma() == em.gamma(a, b)
    i, j = np.triu_indices(300, 1)
    s = int((np.sign(a[i] - a[j]) * np.sign(b[i] - b[j])).sum())
    assert pc.tau_a() == s / (300 * 299 // 2)
    assert _counts_of(a, a, classes, 3).gamma() == 1.0 and _counts_of(a, -a, classes, 3).gamma() == -1.0
    assert _counts_of(a, a, classes, 3).tau_b() == 1.0 and _counts_of(a, -a, classes, 3).tau_b() == -1.0


def _node_graph(tree):
    """(h, c, the matrix of shortest paths) of every node of a tree: nodes are the time steps of the branches, a branch's
    first node hangs on its parent's last."""
    first, last, _ = em.tree_arrays(tree["topology"], tree["time"], tree["branches"])
    index, h, c = {}, [], []
    for x, b in enumerate(tree["branches"]):
        for t in range(tree["time"][b]):
            index[(b, t)] = len(h)
            h.append(first[x] + t)
            c.append(x)
    edges = [(index[(b, t)], index[(b, t + 1)]) for b in tree["branches"] for t in range(tree["time"][b] - 1)]
    edges += [(index[(par, tree["time"][par] - 1)], index[(child, 0)]) for par, child in tree["topology"]]
    n = len(h)
    g = scipy.sparse.coo_matrix((np.ones(len(edges)), tuple(zip(*edges))), shape=(n, n))
    return np.array(h), np.array(c), scipy.sparse.csgraph.shortest_path(g, directed=False, unweighted=True)


@pytest.mark.parametrize("name", list(TREES))
def test_tree_distances_are_the_shortest_paths_on_the_node_graph(name):
    tree = TREES[name]
    h, c, want = _node_graph(tree)
    _, _, J = em.tree_arrays(tree["topology"], tree["time"], tree["branches"])
    every = np.arange(len(h))
    got = em.distances(h, c, J, every, every)
    assert np.array_equal(got, want.astype(np.int64))
    # and the package's junction rule gives the same table
    from prosstt_amd.tree import Tree
    from prosstt_amd.trends import _Nodes
    forks = len({par for par, _ in tree["topology"]})
    t = Tree(topology=tree["topology"], time=tree["time"], num_branches=len(tree["branches"]), branch_points=forks, modules=0,
             G=4)
    nodes = _Nodes(t)
    assert nodes.names == tree["branches"]
    _, _, J_pkg = evaluate._depths(nodes, h, np.array(tree["branches"])[c], 1, "the tree")
    assert np.array_equal(J_pkg, J)


def test_pearson_of_the_moments_is_scipys_on_the_pair_list():
    rng = np.random.default_rng(11)
    tree, tree2 = TWO_LEVEL, FORK
    first, last, J = em.tree_arrays(tree["topology"], tree["time"], tree["branches"], ticks=4)
    first2, last2, J2 = em.tree_arrays(tree2["topology"], tree2["time"], tree2["branches"], ticks=4)
    N = 64
    c = rng.integers(0, 7, N)
    h = np.array([rng.integers(first[x] * 4, last[x] * 4 + 1) for x in c])
    c2 = rng.integers(0, 3, N)
    h2 = np.array([rng.integers(first2[x] * 4, last2[x] * 4 + 1) for x in c2])
    order, offsets = em.by_class(c, 7)
    sums = em.pair_moments(h[order], offsets, J, h2[order], c2[order], J2)
    pm = evaluate.moments_from_words(em.words(sums), em.pairs(offsets), 4)
    i, j = np.triu_indices(N, 1)
    d = em.distances(h, c, J, np.arange(N), np.arange(N))[i, j]
    e = em.distances(h2, c2, J2, np.arange(N), np.arange(N))[i, j]
    assert sum(pm.d.ravel().tolist()) == int(d.sum()) and sum(pm.dd2.ravel().tolist()) == int((d * e).sum())
    assert abs(pm.pearson() - scipy.stats.pearsonr(d, e).statistic) <= 1e-11
    same = evaluate.moments_from_words(em.words(em.pair_moments(h[order], offsets, J, h[order], c[order], J)), em.pairs(offsets), 4)
    assert same.pearson() == 1.0


def _table(true, found):
    tv, ti = np.unique(true, return_inverse=True)
    fv, fi = np.unique(found, return_inverse=True)
    t = np.zeros((len(tv), len(fv)), dtype=np.int64)
    np.add.at(t, (ti, fi), 1)
    return t, tv, fv


@pytest.mark.parametrize("seed", range(6))
def test_ari_and_nmi_are_scikit_learns(seed):
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(seed)
    Kt, Kf = rng.integers(1, 7), rng.integers(1, 7)
    true = rng.integers(0, Kt, 400)
    found = np.where(rng.random(400) < 0.6, true % Kf, rng.integers(0, Kf, 400))
    ls = evaluate.label_scores(*_table(true, found))
    assert abs(ls.ari - metrics.adjusted_rand_score(true, found)) <= 1e-12
    assert abs(ls.nmi - metrics.normalized_mutual_info_score(true, found)) <= 1e-12
    perfect = evaluate.label_scores(*_table(true, (true + 1) % Kt))
    assert perfect.ari == 1.0 and abs(perfect.nmi - 1.0) <= 1e-12 and perfect.accuracy == 1.0
    assert np.all(perfect.jaccard == 1.0) and np.all(perfect.f1 == 1.0)


@pytest.mark.parametrize("Kt,Kf", [(1, 1), (2, 2), (3, 3), (3, 2), (4, 4), (5, 5), (5, 3)])
def test_the_matched_accuracy_is_the_permutation_searchs(Kt, Kf):
    rng = np.random.default_rng(10 * Kt + Kf)
    true = np.concatenate([np.arange(Kt), rng.integers(0, Kt, 300)])
    found = np.concatenate([np.arange(Kt) % Kf, rng.integers(0, Kf, 300)])
    found = np.where(rng.random(len(true)) < 0.5, (true * 3 + 1) % Kf, found)
    found[:Kf] = np.arange(Kf)                                    # every found label occurs
    ls = evaluate.label_scores(*_table(true, found))
    assert ls.accuracy == ptree_quality.branch_accuracy(found, true)
    matched = sum(int(ls.table[list(ls.true_labels).index(t), list(ls.found_labels).index(f)]) for t, f in ls.matching.items())
    assert matched / ls.n == ls.accuracy
