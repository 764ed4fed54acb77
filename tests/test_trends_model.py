"""The numpy model of the expression trends (tests/trends_model.py) against independent arithmetic: its tree distance against
scipy's shortest paths on the node graph, its quantised tricube weight against exact rational arithmetic of the same formula,
and its vectorised integer sums against term-by-term Python integers.  No GPU, and nothing of prosstt_amd.trends."""
from fractions import Fraction

import numpy as np
import pytest

import trends_model as tm
from prosstt_amd.tree import Tree

TREES = {
    "chain": ([["A", "B"], ["B", "C"]], {"A": 5, "B": 3, "C": 4}, "A"),
    "bifurcation": ([["A", "B"], ["A", "C"]], {"A": 6, "B": 4, "C": 7}, "A"),
    "star5": ([["R", "a"], ["R", "b"], ["R", "c"], ["R", "d"], ["R", "e"]],
              {"R": 4, "a": 3, "b": 5, "c": 1, "d": 2, "e": 6}, "R"),
    # the double bifurcation of the reference's axolotl notebook
    "double": ([["progenitor", "nonskeletal"], ["progenitor", "intermediate"], ["intermediate", "bone"],
                ["intermediate", "cartilage"]],
               {"progenitor": 5, "nonskeletal": 7, "intermediate": 3, "bone": 6, "cartilage": 4}, "progenitor"),
}


def make_tree(name, G=3):
    topology, time, root = TREES[name]
    return Tree(topology=topology, time=time, num_branches=len(time), branch_points=len({p for p, _ in topology}),
                modules=0, G=G, root=root)


@pytest.mark.parametrize("name", sorted(TREES))
def test_distance_is_the_shortest_path_on_the_node_graph(name):
    import scipy.sparse as sparse
    from scipy.sparse.csgraph import shortest_path
    tree = make_tree(name)
    nodes = tm.Nodes(tree)
    # the node graph: consecutive time steps of a branch, and a parent's last node with each child's first
    rows, cols = [], []
    for b, n in enumerate(nodes.length):
        for j in range(n - 1):
            rows.append(nodes.offset[b] + j)
            cols.append(nodes.offset[b] + j + 1)
        if nodes.parent[b] >= 0:
            p = nodes.parent[b]
            rows.append(nodes.offset[p] + nodes.length[p] - 1)
            cols.append(nodes.offset[b])
    graph = sparse.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(nodes.R, nodes.R))
    want = shortest_path(graph, directed=False, unweighted=True)
    assert np.all(np.isfinite(want))
    bt = tree.branch_times()
    for b, name_b in enumerate(nodes.names):         # the model's times are Tree.branch_times's
        assert [nodes.first[b], nodes.last[b]] == list(bt[name_b])
    got = np.array([[tm.distance(nodes, int(nodes.node_branch[r]), nodes.node_time[r], int(nodes.node_branch[s]),
                                 nodes.node_time[s]) for s in range(nodes.R)] for r in range(nodes.R)])
    np.testing.assert_array_equal(got, want)


def exact_q_times_two(d, h):
    """2 * (4096 w) as an exact rational for the rational d and h: floor(x + 1/2) is decided by it."""
    u = Fraction(d) / Fraction(h)
    if u >= 1:
        return None
    w = (1 - u ** 3) ** 3
    return 2 * 4096 * w


def test_quantised_weight_against_exact_rational_arithmetic():
    rng = np.random.default_rng(4096)
    cases = [(d, h) for h in (0.3, 1.0, 3.0, 17.5) for d in np.concatenate([rng.uniform(0, 1.1 * h, 400), np.arange(0, 20),
                                                                             [h, np.nextafter(h, 0), 0.0]])]
    equal = near_half = 0
    for d, h in cases:
        got = tm.tricube_q(d, h)
        x2 = exact_q_times_two(float(d), float(h))
        if x2 is None:
            assert got == 0
            continue
        assert 0 <= got <= 4096
        # exact 4096 w = x2 / 2; its distance from the nearest half-integer
        frac = (x2 / 2) % 1
        off_half = abs(frac - Fraction(1, 2))
        want = (x2 + 1) // 2                         # floor(x + 1/2)
        if off_half > Fraction(1, 10 ** 9):
            assert got == want, (d, h)
            equal += 1
        else:
            below = (x2 / 2).numerator // (x2 / 2).denominator
            assert got in (below, below + 1), (d, h)              # one of the two neighbours
            near_half += 1
    assert equal > 1000
    assert tm.tricube_q(0.0, 3.0) == 4096 and tm.tricube_q(3.0, 3.0) == 0 and tm.tricube_q(2.999, 3.0) == 0


def test_rounding_of_a_u_just_below_one_is_no_entry_only_at_or_above_one():
    h = 3.0
    d = np.nextafter(h, 0)
    assert d / h < 1.0 and tm.tricube_q(d, h) == 0   # an entry by u < 1, dropped by q = 0


def test_sums_in_python_integers():
    rng = np.random.default_rng(7)
    N, G, R = 9, 5, 4
    X = rng.integers(0, 50, size=(N, G)).astype(np.int32)
    X[0, 0] = X[3, 0] = X[5, 1] = 2 ** 31 - 1
    indptr = np.array([0, 3, 3, 9, 12], dtype=np.int64)
    indices = np.array([0, 3, 3, 5, 0, 1, 2, 8, 0, 3, 5, 0], dtype=np.int32)          # repeats, an empty row
    weights = np.array([4096, 4096, 4095, 1, 0, 7, 4096, 9, 4096, 4096, 4096, 4096], dtype=np.int32)
    E1, E2 = tm.node_sums_exact(X, indptr, indices, weights)
    S1, S2 = tm.node_sums(X, indptr, indices, weights)
    assert S1.tolist() == E1.tolist() and S2.tolist() == E2.tolist()
    assert E1[0, 0] == (4096 + 4096 + 4095) * (2 ** 31 - 1)
    assert E2[0, 0] == (4096 + 4096 + 4095) * (2 ** 31 - 1) ** 2 and E2[0, 0] > 1 << 64
    assert all(v == 0 for v in E1[1]) and all(v == 0 for v in E2[1])
    w = tm.words(S2)
    assert w.dtype == np.uint64 and w.shape == (R, G, 2)
    assert (int(w[0, 0, 1]) << 64) | int(w[0, 0, 0]) == E2[0, 0] and w[0, 0, 1] > 0
    assert tm.as_int64(S1).dtype == np.int64 and tm.as_int64(S1)[0, 0] == E1[0, 0]


def test_dense_weights_of_a_bifurcation_by_hand():
    tree = make_tree("bifurcation")                  # A: 0..5, B: 6..9, C: 6..12
    pt = np.array([5.0, 6.0, 6.0, 2.5])
    br = np.array(["A", "B", "C", "A"])
    Q, labels = tm.dense_weights(tree, pt, br, 2.0)
    assert labels.tolist() == [5, 6, 10, 3]          # 2.5 rounds half up
    # node (B, 6) is row 6: distances 1, 0, 2 (through the junction at 5), 3.5
    assert Q[6].tolist() == [tm.tricube_q(1.0, 2.0), 4096, 0, 0]
    assert Q[5].tolist() == [4096, tm.tricube_q(1.0, 2.0), tm.tricube_q(1.0, 2.0), 0]
    Qn, ln = tm.dense_weights(tree, pt, br, 2.0, kernel="nearest")
    assert ln.tolist() == labels.tolist() and Qn.sum() == 4 * 4096 and all(Qn[labels[i], i] == 4096 for i in range(4))
