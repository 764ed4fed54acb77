"""The host half of prosstt_amd.mapping, which needs no device: ``poisson_panel`` against tests/mapping_model.py, the node ->
(branch, pseudotime) table on a chain, a bifurcation and the topology of the reference's probabilistic_branching notebook, and
every refusal that comes before the pass.  No GPU."""
import numpy as np
import pytest

import mapping_model as mm

torch = pytest.importorskip("torch")

from prosstt_amd import mapping  # noqa: E402
from prosstt_amd.tree import Tree  # noqa: E402


def _tree(topology, time, G=4):
    names = sorted({b for pair in topology for b in pair}) or list(time)
    return Tree(topology=topology, time=time, num_branches=len(names), branch_points=max(0, (len(names) - 1) // 2), modules=0,
                G=G)


# ------------------------------------------------------------------------------------------------------ the panel

@pytest.mark.parametrize("weights", [False, True])
def test_poisson_panel_against_the_model(weights):
    rng = np.random.default_rng(11)
    means = rng.gamma(2.0, 3.0, size=(23, 57))
    means[rng.random(means.shape) < 0.05] = 0.0                 # floored
    w = rng.uniform(0.2, 1.0, 57) if weights else None
    panel, exposure = mapping.poisson_panel(means, w)
    want_p, want_e = mm.poisson_panel(means, w)
    assert panel.dtype == np.float32 and exposure.dtype == np.float64 and panel.shape == (23, 57)
    # the mean over the nodes is one rounded sum in either; the float32 rounding may then differ by one unit in a few entries
    scale = np.abs(want_p).astype(np.float64)
    assert np.all(np.abs(panel.astype(np.float64) - want_p) <= 2.0 ** -23 * scale + 1e-14)
    assert np.mean(panel == want_p) > 0.99
    np.testing.assert_allclose(exposure, want_e, rtol=0, atol=1e-10)
    assert not np.any((panel != 0) & (np.abs(panel) < 2.0 ** -100))
    # the floor is what an absent gene's mean becomes
    floored, _ = mapping.poisson_panel(np.array([[0.0, 1.0], [1.0, 1.0]]), floor=2.0 ** -10)
    assert floored.tolist() == [[-5 * np.log(2.0).astype(np.float32), 0.0], [5 * np.log(2.0).astype(np.float32), 0.0]]


@pytest.mark.parametrize("bad, match", [
    (np.array([[1.0, np.nan]]), "finite"), (np.array([[1.0, np.inf]]), "finite"), (np.array([[1.0, -1.0]]), "negative"),
    (np.array([1.0, 2.0]), "nodes, genes"), (np.array([["a"]]), "numbers"), (np.zeros((0, 3)), "nodes, genes"),
])
def test_poisson_panel_refuses_bad_means(bad, match):
    with pytest.raises(ValueError, match=match):
        mapping.poisson_panel(bad)


def test_poisson_panel_refuses_bad_weights_and_floor():
    means = np.ones((3, 4))
    for w in (np.ones(3), np.array([1, 1, 1, np.nan]), np.array([1, 1, 1, -1.0]), np.ones((4, 1))):
        with pytest.raises(ValueError, match="weight"):
            mapping.poisson_panel(means, w)
    for floor in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="floor"):
            mapping.poisson_panel(means, floor=floor)


# ------------------------------------------------------------------------------------------------------ the nodes

NOTEBOOK = [["A", "B"], ["B", "C"], ["B", "D"], ["D", "E"], ["C", "F"], ["F", "G"]]      # probabilistic_branching.ipynb


@pytest.mark.parametrize("topology, time", [
    ([], {"A": 5}),
    ([["A", "B"], ["A", "C"]], {"A": 4, "B": 3, "C": 6}),
    (NOTEBOOK, {b: 50 for b in "ABCDEFG"}),
    (NOTEBOOK, {"A": 1, "B": 2, "C": 3, "D": 1, "E": 5, "F": 2, "G": 1}),
])
def test_node_table(topology, time):
    from prosstt_amd import simulation as sim
    if topology:
        tree = _tree(topology, time)
    else:
        tree = Tree(topology=[], time=time, num_branches=1, branch_points=0, modules=0, G=4, root="A")
    table = mapping.node_table(tree)
    offsets, code, when = mm.node_table(topology, time, list(tree.branches), tree.root)
    assert table.names == list(tree.branches)
    assert np.array_equal(table.offsets, offsets) and table.offsets.dtype == np.int64
    assert np.array_equal(table.branch_code, code) and table.branch_code.dtype == np.int32
    assert np.array_equal(table.pseudotime, when) and table.pseudotime.dtype == np.int64
    # the table is the inverse of simulation.cell_rows
    names = np.asarray(table.names)[table.branch_code]
    assert np.array_equal(sim.cell_rows(tree, table.pseudotime, names), np.arange(offsets[-1]))
    bt = tree.branch_times()
    for k, b in enumerate(table.names):
        assert when[offsets[k]] == bt[b][0] and when[offsets[k + 1] - 1] == bt[b][1]


def test_a_sharded_tree_is_refused():
    tree = _tree([["A", "B"], ["A", "C"]], {"A": 4, "B": 3, "C": 3})
    tree._resident = ["A", "B"]
    with pytest.raises(ValueError, match="sharded over processes"):
        mapping.node_table(tree)
    X = torch.zeros((5, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="sharded over processes"):
        mapping.map_cells(X, None, tree)


# ------------------------------------------------------------------------------------------------------ refusals

def _args(N=5, G=8, R=6):
    rng = np.random.default_rng(2)
    X = torch.from_numpy(rng.poisson(2.0, size=(N, G)).astype(np.int32))          # a CPU tensor: refused last of all
    panel = rng.standard_normal((R, G)).astype(np.float32)
    return X, np.ones(N), panel, np.zeros(R)


def test_node_scores_refuses_a_host_matrix_and_other_dtypes():
    X, s, panel, expo = _args()
    with pytest.raises(TypeError, match="host arrays are refused"):
        mapping.node_scores(X.numpy(), s, panel, expo)
    with pytest.raises(TypeError, match="int32"):
        mapping.node_scores(X.to(torch.int64), s, panel, expo)
    with pytest.raises(ValueError, match="dimensions"):
        mapping.node_scores(X[0], s, panel, expo)
    with pytest.raises(ValueError, match="at least one cell and one gene"):
        mapping.node_scores(X[:0], s[:0], panel, expo)
    with pytest.raises(ValueError, match="needs a device tensor"):
        mapping.node_scores(X, s, panel, expo)                  # everything else was accepted


def test_node_scores_refuses_wrong_shapes_dtypes_and_values():
    X, s, panel, expo = _args()
    cases = [
        (dict(panel=panel.astype(np.float64)), "float32"),
        (dict(panel=panel[:, :7]), "the panel has 7 genes, the matrix 8"),
        (dict(panel=panel[0]), "float32 array"),
        (dict(panel=[[0.0] * 8]), "float32 array"),
        (dict(panel=torch.from_numpy(panel).double()), "float32"),
        (dict(sc=np.ones(4)), "one size factor per cell"),
        (dict(sc=np.array([1, 1, 1, 1, np.nan])), "size factors must be finite"),
        (dict(sc=np.array([1, 1, 1, 1, -1.0])), "size factors must be finite and not negative"),
        (dict(exposure=np.zeros(5)), "exposure must hold one number per node"),
        (dict(exposure=np.array([0, 0, 0, 0, 0, np.inf])), "exposure must be finite"),
        (dict(constants=np.zeros((6, 1))), "constants must hold one number per node"),
        (dict(constants=np.array([0, 0, 0, 0, 0, np.nan])), "constants must be finite"),
        (dict(branch_offsets=[0, 4, 3, 6]), "must ascend from 0"),
        (dict(branch_offsets=[1, 6]), "must ascend from 0"),
        (dict(branch_offsets=[0, 5]), "must ascend from 0"),
        (dict(branch_offsets=[0]), "at least two entries"),
        (dict(branch_offsets=[0.0, 6.0]), "integer array"),
        (dict(out="cupy"), "out must be"),
        (dict(node_tile=5), "node_tile"),
        (dict(node_tile=True), "node_tile"),
    ]
    for change, match in cases:
        kw = dict(sc=s, panel=panel, exposure=expo)
        kw.update(change)
        sc, p, e = kw.pop("sc"), kw.pop("panel"), kw.pop("exposure")
        with pytest.raises(ValueError, match=match):
            mapping.node_scores(X, sc, p, e, **kw)


@pytest.mark.parametrize("chain", [0, 16, 31, 33, 100, 4128, 8192, -32, 64.0, "256", True, None])
def test_a_bad_genes_per_chain_is_refused(chain):
    X, s, panel, expo = _args()
    with pytest.raises(ValueError, match="genes_per_chain must be a multiple of 32"):
        mapping.node_scores(X, s, panel, expo, genes_per_chain=chain)
    tree = _tree([["A", "B"], ["A", "C"]], {"A": 2, "B": 2, "C": 2}, G=8)
    with pytest.raises(ValueError, match="genes_per_chain must be a multiple of 32"):
        mapping.map_cells(X, s, tree, genes_per_chain=chain)


def test_map_cells_refuses_a_host_matrix_a_bad_prior_and_zeros_under_density():
    X, s, _, _ = _args()
    tree = _tree([["A", "B"], ["A", "C"]], {"A": 2, "B": 2, "C": 2}, G=8)
    with pytest.raises(TypeError, match="host arrays are refused"):
        mapping.map_cells(X.numpy(), s, tree)
    with pytest.raises(ValueError, match="prior must be"):
        mapping.map_cells(X, s, tree, prior="flat")
    with pytest.raises(ValueError, match="prior must hold one number per node"):
        mapping.map_cells(X, s, tree, prior=np.zeros(5))
    with pytest.raises(ValueError, match="prior must be finite"):
        mapping.map_cells(X, s, tree, prior=np.array([0, 0, 0, 0, 0, -np.inf]))
    density = {"A": np.array([0.5, 0.0]), "B": np.array([0.25, 0.0]), "C": np.array([0.125, 0.125])}
    tree.set_density(density)
    with pytest.raises(ValueError, match="positive density at every node: 2 of 6 nodes have none"):
        mapping.map_cells(X, s, tree, prior="density")
    with pytest.raises(ValueError, match="out must be"):
        mapping.map_cells(X, s, tree, out="csr")


def test_the_status_word_names_its_bits():
    from prosstt_amd import device
    mapping.check_status(0)
    with pytest.raises(ValueError, match=r"status bit NEGATIVE \(1\): %s" % device.NEGATIVE_ENTRY):
        mapping.check_status(1)
    with pytest.raises(ValueError, match=r"status bit BRANCH_RANGE \(2\)"):
        mapping.check_status(2)
    with pytest.raises(ValueError) as err:
        mapping.check_status(3)
    assert str(err.value).count("status bit") == 2
    with pytest.raises(RuntimeError, match="unknown status bit"):
        mapping.check_status(4)
