"""The host half of prosstt_amd.ptree: the refusals, which come before any device use, and ``to_tree`` on hand-made trees (a
chain, one fork, a fork of degree 4, a twig that is pruned, a root cell in the middle of a branch).  No GPU."""
import numpy as np
import pytest

import ptree_model as pm

from prosstt_amd import ptree, trends


def _fit(centres, edges, Y, root, min_branch_nodes=3):
    centres = np.asarray(centres, dtype=np.float32)
    Y = np.asarray(Y, dtype=np.float32)
    best = pm.assign(Y, centres, 0.0, False).best
    return pm.to_tree(Y, centres, np.asarray(edges, dtype=np.int32), best, root, min_branch_nodes, G=7)


def _check(lf, n_cells):
    """What every result must satisfy: the tree's own checks, and the libraries downstream accept the fields."""
    from prosstt_amd import simulation as sim
    t = lf.tree
    t._check_topology()
    bt = t.branch_times()
    assert lf.pseudotime.dtype == np.int64 and lf.node.dtype == np.int32 and lf.position.dtype == np.float64
    assert len(lf.branches) == len(lf.pseudotime) == len(lf.node) == len(lf.position) == n_cells
    for b, time in zip(lf.branches, lf.pseudotime):
        assert bt[b][0] <= time <= bt[b][1]
    nodes = trends._Nodes(t)
    times, codes = trends._cells(nodes, lf.pseudotime, lf.branches)
    assert np.array_equal(times, lf.pseudotime.astype(np.float64))
    assert np.array_equal(sim.cell_rows(t, lf.pseudotime, lf.branches), lf.node)
    assert sum(int(t.time[b]) for b in t.branches) == len(lf.kept) == len(lf.node_rows)
    assert sorted(lf.node_rows.tolist()) == list(range(len(lf.kept)))
    density = np.concatenate([t.density[b] for b in t.branches])
    assert np.array_equal(density, np.bincount(lf.node, minlength=len(lf.kept)) / n_cells)
    assert t.G == 7 and t.num_branches == len(t.branches)
    assert np.all(lf.position >= 0) and np.all(lf.position <= max(v[1] for v in bt.values()))


def _line(n, start=0.0):
    return [[start + i, 0.0] for i in range(n)]


def test_a_chain_is_one_branch_from_the_tip_nearest_the_root_cell():
    centres = _line(6)
    edges = [[i, i + 1] for i in range(5)]
    Y = [[0.2, 0.1], [4.9, -0.1], [2.5, 0.3], [3.0, 0.0]]
    lf = _fit(centres, edges, Y, root=1)                                     # cell 1 lies on node 5: that tip is the root
    _check(lf, 4)
    assert lf.tree.topology == [] and lf.tree.branches == ["B0"] and int(lf.tree.time["B0"]) == 6
    assert lf.pseudotime.tolist() == [5, 0, 2, 2] or lf.pseudotime.tolist() == [5, 0, 3, 2]
    assert lf.position.tolist() == pytest.approx([4.8, 0.1, 2.5, 2.0])
    other = _fit(centres, edges, Y, root=0)
    assert other.pseudotime.tolist()[:2] == [0, 5] and other.position.tolist() == pytest.approx([0.2, 4.9, 2.5, 3.0])
    # a root cell in the middle of the chain: the nearer tip, the lower node on a tie
    assert _fit(centres, edges, Y, root=3).pseudotime[1] == 0                # node 3: two edges from tip 5, three from tip 0
    assert _fit(_line(5), edges[:4], Y, root=2).pseudotime[0] == 0           # node 2 or 3 of five: hops 2 and 2 -> tip 0


def _fork():
    """Nodes 0 .. 3 along x, the fork at node 3, then 4 .. 6 up and 7 .. 9 down."""
    centres = _line(4) + [[3.0 + i, float(i)] for i in (1, 2, 3)] + [[3.0 + i, -float(i)] for i in (1, 2, 3)]
    edges = [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [5, 6], [3, 7], [7, 8], [8, 9]]
    return centres, edges


def test_one_fork_gives_three_branches_with_the_fork_last_on_its_parent():
    centres, edges = _fork()
    Y = [[0.1, 0.0], [3.1, 0.1], [4.0, 1.1], [6.0, 3.0], [5.0, -2.0], [1.6, 0.0]]
    lf = _fit(centres, edges, Y, root=0)
    _check(lf, 6)
    assert lf.tree.topology == [["B0", "B1"], ["B0", "B2"]] and lf.tree.root == "B0" and lf.tree.branch_points == 1
    assert {b: int(lf.tree.time[b]) for b in lf.tree.branches} == {"B0": 4, "B1": 3, "B2": 3}
    assert lf.branches.tolist() == ["B0", "B0", "B1", "B1", "B2", "B0"]
    assert lf.pseudotime.tolist() == [0, 3, 4, 6, 5, 2]
    assert lf.node.tolist() == [0, 3, 4, 6, 8, 2] and lf.kept.tolist() == list(range(10))
    assert lf.position.tolist() == pytest.approx([0.1, 3.1, 4.05, 6.0, 5.0, 1.6], abs=1e-6)
    # rooted at the tip of the upper arm: that arm is the root branch and runs down to the fork
    up = _fit(centres, edges, Y, root=3)
    _check(up, 6)
    assert {b: int(up.tree.time[b]) for b in up.tree.branches} == {"B0": 4, "B1": 3, "B2": 3}
    assert up.branches.tolist() == ["B1", "B0", "B0", "B0", "B2", "B1"] and up.pseudotime[3] == 0
    # a root cell in the middle of the stem (node 2): tip 0 is two edges away, the others four
    middle = _fit(centres, edges, Y, root=5)
    assert middle.branches.tolist() == lf.branches.tolist() and np.array_equal(middle.pseudotime, lf.pseudotime)


def test_a_fork_of_degree_4():
    centres = [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [2, 1], [2, 2], [2, -1], [2, -2]]
    edges = [[0, 1], [1, 2], [2, 3], [3, 4], [2, 5], [5, 6], [2, 7], [7, 8]]
    Y = [[0, 0], [4, 0], [2, 2], [2, -2], [2.1, 0]]
    lf = _fit(centres, edges, Y, root=0, min_branch_nodes=2)
    _check(lf, 5)
    assert lf.tree.topology == [["B0", "B1"], ["B0", "B2"], ["B0", "B3"]] and lf.tree.branch_points == 1
    assert {b: int(lf.tree.time[b]) for b in lf.tree.branches} == {"B0": 3, "B1": 2, "B2": 2, "B3": 2}
    assert lf.branches.tolist() == ["B0", "B1", "B2", "B3", "B0"]          # children in ascending order of their first node
    assert lf.pseudotime.tolist() == [0, 4, 4, 4, 2]


def test_a_twig_is_pruned_and_its_cells_go_to_the_kept_nodes():
    centres, edges = _fork()
    centres = centres + [[2.0, 0.6]]                                        # node 10: a twig of one node on node 2
    edges = edges + [[2, 10]]
    Y = [[0.1, 0.0], [2.0, 0.7], [6.0, 3.0], [6.0, -3.0]]
    lf = _fit(centres, edges, Y, root=0)
    _check(lf, 4)
    assert lf.kept.tolist() == list(range(10)) and lf.tree.topology == [["B0", "B1"], ["B0", "B2"]]
    assert int(lf.tree.time["B0"]) == 4 and lf.node.tolist() == [0, 2, 6, 9]
    # without pruning the twig is a branch, and node 2 a fork
    full = _fit(centres, edges, Y, root=0, min_branch_nodes=0)
    _check(full, 4)
    assert len(full.tree.branches) == 5 and len(full.kept) == 11 and full.tree.branch_points == 2
    assert full.tree.topology[:2] == [["B0", "B1"], ["B0", "B2"]] and int(full.tree.time["B0"]) == 3
    # the shortest twig goes first (node 10, then the stem 0 .. 2: of three tips of three nodes the lowest); what is left is a
    # chain, and a chain is never pruned
    kept, _ = ptree.prune(11, np.array(edges), 4)
    assert kept.tolist() == [3, 4, 5, 6, 7, 8, 9]
    assert ptree.prune(6, np.array([[i, i + 1] for i in range(5)]), 100)[0].tolist() == list(range(6))
    # the root cell sat on the pruned twig: the nearest kept tip still roots the tree
    assert _fit(centres, edges, Y, root=1).branches.tolist() == lf.branches.tolist()


def test_refusals_come_before_any_device_use():
    Y = np.zeros((10, 3), dtype=np.float32)
    C = np.ones((4, 3), dtype=np.float32)
    bad_panels = [
        (np.zeros(10, dtype=np.float32), C, "2|dimensions"), (np.zeros((10, 0), dtype=np.float32), C[:, :0], "coordinates"),
        (np.zeros((10, 129), dtype=np.float32), np.zeros((4, 129), dtype=np.float32), "coordinates <= 128"),
        (np.zeros((0, 3), dtype=np.float32), C, "cells"), (Y, np.zeros((4097, 3), dtype=np.float32), "nodes <= 4096"),
        (Y, np.ones((4, 2), dtype=np.float32), "3 coordinates, the centres 2"),
        (np.full((10, 3), np.nan), C, "finite"), (Y, np.full((4, 3), np.inf), "finite"), (np.full((10, 3), 1e300), C, "finite"),
    ]
    for y, c, match in bad_panels:
        with pytest.raises(ValueError, match=match):
            ptree.assign(y, c)
        with pytest.raises(ValueError, match=match):
            ptree.project(y, c, np.array([[0, 1]]))
    for y in (np.zeros((10, 3), dtype=np.int32), [["a"]]):
        with pytest.raises(TypeError):
            ptree.assign(y, C)
    for sigma in (-1.0, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="sigma"):
            ptree.assign(Y, C, sigma)
    with pytest.raises(ValueError, match="out must be"):
        ptree.assign(Y, C, out="cupy")
    with pytest.raises(ValueError, match="out must be"):
        ptree.project(Y, C, np.array([[0, 1]]), out="cupy")
    for edges, match in ((np.array([0, 1]), "integer array"), (np.array([[0.0, 1.0]]), "integer array"),
                         (np.zeros((0, 2), dtype=np.int32), "edges"), (np.zeros((8193, 2), dtype=np.int32), "8192"),
                         (np.array([[0, 4]]), "outside"), (np.array([[-1, 2]]), "outside")):
        with pytest.raises(ValueError, match=match):
            ptree.project(Y, C, edges)
    for k, match in ((0, "k must be"), (11, "exceeds the 10 cells"), (4097, "k must be"), (2.0, "k must be"), (True, "k must be")):
        with pytest.raises(ValueError, match=match):
            ptree.kmeans(Y, k)
    with pytest.raises(ValueError, match="n_iter"):
        ptree.kmeans(Y, 2, n_iter=-1)
    with pytest.raises(ValueError, match="init has 3 centres"):
        ptree.kmeans(Y, 2, init=np.zeros((3, 3)))
    for options, match in ((dict(n_nodes=1), "n_nodes"), (dict(n_nodes=11), "exceeds"), (dict(sigma=0.0), "sigma"),
                           (dict(sigma=-2.0), "sigma"), (dict(lam=-1.0), "lam"), (dict(lam=float("nan")), "lam"),
                           (dict(tol=-1e-3), "tol"), (dict(n_iter=1.5), "n_iter"), (dict(init="random"), "init must be")):
        with pytest.raises(ValueError, match=match):
            ptree.principal_tree(Y, **{**dict(n_nodes=4), **options})
    with pytest.raises(ValueError, match="NONFINITE.*EDGE_RANGE"):
        ptree.check_status(3)
    ptree.check_status(0)


def test_to_tree_refuses_what_is_not_a_tree_or_a_cell():
    with pytest.raises(ValueError, match="spanning tree"):
        ptree.prune(4, np.array([[0, 1], [1, 2]]), 2)
    with pytest.raises(ValueError, match="spanning tree"):
        ptree.prune(4, np.array([[0, 1], [1, 0], [2, 3]]), 2)
    with pytest.raises(ValueError, match="spanning tree"):
        ptree.prune(3, np.array([[0, 1], [1, 3]]), 2)
    fit = ptree.PrincipalTree(None, np.zeros((3, 2), dtype=np.float32), np.array([[0, 1], [1, 2]], dtype=np.int32),
                              np.zeros(1), 1.0, 1.0, 0, False, np.zeros(5, dtype=np.int32))
    for options, match in ((dict(root=5), "root"), (dict(root=-1), "root"), (dict(root=0, min_branch_nodes=-1), "min_branch"),
                           (dict(root=0, G=0), "G must be")):
        with pytest.raises(ValueError, match=match):
            fit.to_tree(**options)
    assert "nodes=3" in repr(fit)
