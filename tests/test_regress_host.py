"""The host side of prosstt_amd/regress.py without a GPU: the refusals of options and shapes (all before any device use), the
tree design on smoke()'s tree and on a tree of 8 branches, the Wald test against a hand computation, ``NormalEquations.concat``,
and the Fisher scoring's bookkeeping (genes without counts, separated coefficients) through the numpy model."""
import numpy as np
import pytest
import torch

import regress_model as M

from prosstt_amd import mapping, regress
from prosstt_amd.tree import Tree


def _smoke_tree():
    return Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1, modules=5, G=300)


def _eight():
    topology = [["A", "B"], ["A", "C"], ["B", "D"], ["B", "E"], ["C", "F"], ["C", "G"], ["D", "H"]]
    time = {"A": 12, "B": 7, "C": 9, "D": 5, "E": 6, "F": 4, "G": 8, "H": 3}
    return Tree(topology=topology, time=time, num_branches=8, branch_points=3, modules=5, G=10)


def test_refusals_of_the_matrix_the_options_and_the_shapes():
    X = torch.zeros((6, 4), dtype=torch.int32)
    sc, labels, D, coef = np.ones(6), np.zeros(6, dtype=np.int64), np.ones((1, 2)), np.zeros((4, 2))
    with pytest.raises(TypeError, match="host arrays are refused"):
        regress.normal_equations(X.numpy(), sc, labels, D, coef, 0.2, 2.0)
    with pytest.raises(TypeError, match="needs int32 counts"):
        regress.normal_equations(X.long(), sc, labels, D, coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="needs a device tensor"):
        regress.normal_equations(X, sc, labels, D, coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="out must be"):
        regress.normal_equations(X, sc, labels, D, coef, 0.2, 2.0, out="cupy")
    for split in (4, 64, True, 16.5):
        with pytest.raises(ValueError, match="split must be 0"):
            regress.normal_equations(X, sc, labels, D, coef, 0.2, 2.0, split=split)
    with pytest.raises(ValueError, match="need 1 <= p <= 16 coefficients"):
        regress.normal_equations(X, sc, labels, np.ones((3, 17)), np.zeros((4, 17)), 0.2, 2.0)
    with pytest.raises(ValueError, match=r"the design must be a \(rows, p\) array"):
        regress.normal_equations(X, sc, labels, np.ones(3), coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="the design must be finite"):
        regress.normal_equations(X, sc, labels, np.array([[1.0, np.nan]]), coef, 0.2, 2.0)
    with pytest.raises(ValueError, match=r"coef must be \(genes, p\) = \(4, 2\)"):
        regress.normal_equations(X, sc, labels, D, np.zeros((2, 4)), 0.2, 2.0)
    with pytest.raises(ValueError, match="alpha must be a number or one per gene"):
        regress.normal_equations(X, sc, labels, D, coef, np.ones(3), 2.0)
    with pytest.raises(ValueError, match="need one label per cell"):
        regress.normal_equations(X, sc, labels[:5], D, coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="need one size factor per cell"):
        regress.normal_equations(X, sc[:5], labels, D, coef, 0.2, 2.0)
    for options, message in ((dict(max_rounds=0), "max_rounds"), (dict(max_rounds=2.5), "max_rounds"), (dict(tol=0.0), "tol must be"),
                             (dict(tol=np.nan), "tol must be"), (dict(limit=0.0), "limit must be"), (dict(limit=701.0), "limit must be"),
                             (dict(split=7), "split must be")):
        with pytest.raises(ValueError, match=message):
            regress.regression(X, sc, labels, D, alpha=0.2, beta=2.0, **options)
    with pytest.raises(ValueError, match="a label is not below the number of rows of the design"):
        regress.regression(X, sc, labels + 1, D, alpha=0.2, beta=2.0)
    with pytest.raises(ValueError, match="status bit NEGATIVE .*; status bit ETA"):
        regress.check_status(regress.ETA | regress.NEGATIVE)
    regress.check_status(0)
    for K in (0, 2.0, True):
        with pytest.raises(ValueError, match="number of groups"):
            regress.group_design(K)
    assert np.array_equal(regress.group_design(3), np.eye(3))


def test_row_blocks_is_the_rule_of_the_other_strip_libraries():
    assert regress.row_blocks(1, 1) == (1, 1) and regress.row_blocks(64, 300) == (64, 1) and regress.row_blocks(65, 300) == (33, 2)
    assert regress.row_blocks(700, 256) == (64, 11) and regress.row_blocks(50000, 20000) == (4167, 12)
    assert regress.row_blocks(300, 257) == regress.row_blocks(300, 128) == (60, 5)


@pytest.mark.parametrize("tree,inner", [(_smoke_tree, 0), (_smoke_tree, 1), (_smoke_tree, 4), (_eight, 0)])
def test_tree_design(tree, inner):
    t = tree()
    d = regress.tree_design(t, inner)
    table = mapping.node_table(t)
    B = len(table.names)
    p = 1 + B * (inner + 1)
    assert d.matrix.shape == (int(table.offsets[-1]), p) and d.p == p and len(d.knots) == p and d.names == table.names
    assert np.all(d.matrix >= 0) and np.all((d.matrix > 0).sum(axis=1) <= 2)
    np.testing.assert_allclose(d.matrix.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.linalg.matrix_rank(d.matrix) == p
    # a knot's own node has weight 1 on it: the root's first node, every branch's last
    assert d.matrix[0, 0] == 1.0 and d.knots[0] == (table.names[0], 0.0)
    for b in range(B):
        end = 1 + b * (inner + 1) + inner
        assert d.matrix[table.offsets[b + 1] - 1, end] == 1.0
        assert d.knots[end] == (table.names[b], float(table.pseudotime[table.offsets[b + 1] - 1]))
    # a function that is linear in time along every path is reproduced: the hats interpolate
    np.testing.assert_allclose(d.matrix @ np.array([when for _, when in d.knots]), table.pseudotime, rtol=0, atol=1e-12)
    # continuity across a fork: a child's first node leans on its parent's end knot
    for b in range(1, B):
        first = d.matrix[table.offsets[b]]
        assert first[d.start[b]] > 0 and d.start[b] == 1 + d.parent[b] * (inner + 1) + inner
    constant = d.constant()
    assert constant.shape == (p - 1, p) and np.linalg.matrix_rank(constant) == p - 1 and not (constant @ np.ones(p)).any()
    for name in table.names:
        along = d.along(name)
        assert along.shape == (inner + 1, p) and np.linalg.matrix_rank(along) == inner + 1 and not (along @ np.ones(p)).any()
    a, b = table.names[1], table.names[2]
    between = d.between(a, b)
    assert between.shape == (inner + 1, p) and np.linalg.matrix_rank(between) == inner + 1
    same = np.ones(p)                                            # equal knots at equal depth satisfy it, a shift of one branch not
    assert not (between @ same).any()
    same[d.branch_knots(a)[1:]] += 1.0
    assert (between @ same).all()
    with pytest.raises(ValueError, match="same parent"):
        d.between(table.names[0], a)
    with pytest.raises(ValueError, match="same parent"):
        d.between(a, a)
    with pytest.raises(ValueError, match="not a branch"):
        d.along("nowhere")


def test_tree_design_refusals():
    with pytest.raises(ValueError, match=r"inner = 1 on 8 branches makes 17"):
        regress.tree_design(_eight(), 1)
    with pytest.raises(ValueError, match=r"inner = 5 on 3 branches makes 19"):
        regress.tree_design(_smoke_tree(), 5)
    for inner in (-1, 1.0, True):
        with pytest.raises(ValueError, match="inner must be an integer"):
            regress.tree_design(_smoke_tree(), inner)
    short = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 5, "B": 1, "C": 5}, num_branches=3, branch_points=1, modules=5, G=3)
    with pytest.raises(ValueError, match="too few time steps"):
        regress.tree_design(short, 1)


def _regression(coef, cov, robust=None):
    G, p = coef.shape
    return regress.Regression(coef, cov, robust, np.sqrt(np.diagonal(cov, axis1=1, axis2=2)), np.zeros(G), np.ones(G, dtype=np.int64),
                              np.ones(G, dtype=bool), np.zeros(G, dtype=bool), np.zeros(G, dtype=bool), np.eye(p))


def test_wald_against_a_hand_computation():
    import scipy.stats
    from prosstt_amd import markers
    coef = np.array([[1.0, 3.0, 2.0], [0.5, 0.5, 0.5], [np.nan, 0.0, 0.0]])
    cov = np.stack([np.diag([0.5, 0.25, 1.0]), np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]), np.eye(3)])
    r = _regression(coef, cov)
    w = r.wald([[-1.0, 1.0, 0.0]])
    # gene 0: (3 - 1)^2 / (0.5 + 0.25); gene 1: 0; gene 2: no statistic
    np.testing.assert_allclose(w.statistic[:2], [4.0 / 0.75, 0.0], rtol=1e-14)
    assert np.isnan(w.statistic[2]) and np.isnan(w.pvals[2]) and np.isnan(w.pvals_adj[2]) and np.all(w.df == 1)
    np.testing.assert_allclose(w.pvals[:2], scipy.stats.chi2.sf([4.0 / 0.75, 0.0], 1), rtol=1e-14)
    np.testing.assert_allclose(w.pvals_adj[:2], markers.benjamini_hochberg(w.pvals[:2]), rtol=0)
    L = np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    w = r.wald(L)
    # gene 0 by hand: L c = (2, 1); L V L' = [[0.75, 0.5], [0.5, 1.5]], determinant 0.875
    want = (2 * (1.5 * 2 - 0.5 * 1) + 1 * (-0.5 * 2 + 0.75 * 1)) / 0.875
    np.testing.assert_allclose(w.statistic[0], want, rtol=1e-14)
    assert np.all(w.df == 2) and w.statistic[1] == 0.0
    # the sandwich covariance takes the model's place
    robust = _regression(coef, cov, 2.0 * cov).wald(L)
    np.testing.assert_allclose(robust.statistic[0], want / 2.0, rtol=1e-14)
    for bad in (np.ones((2, 2)), np.array([[1.0, -1.0, 0.0], [2.0, -2.0, 0.0]]), np.array([[np.inf, 0.0, 0.0]])):
        with pytest.raises(ValueError):
            r.wald(bad)
    np.testing.assert_allclose(r.fitted()[:, :2], np.exp(coef[:2].T), rtol=1e-15)
    assert r.fitted(np.ones((4, 3))).shape == (4, 3)
    with pytest.raises(ValueError, match="3 columns"):
        r.fitted(np.ones((4, 2)))


def test_concat_adds_in_list_order_and_refuses_what_does_not_fit():
    rng = np.random.default_rng(2)
    X = rng.poisson(3.0, size=(90, 5))
    sc, labels, D = rng.lognormal(0, 0.3, size=90), rng.integers(-1, 4, size=90), rng.dirichlet(np.ones(3), size=4)
    coef = rng.normal(0, 0.2, size=(5, 3))
    parts = [M.normal_equations(X[lo:hi], sc[lo:hi], labels[lo:hi], D, coef, 0.2, 2.0).ne for lo, hi in ((0, 30), (30, 50), (50, 90))]
    whole = regress.NormalEquations.concat(parts)
    assert whole.n_cells == 90 and whole.n_genes == 5 and whole.p == 3 and not whole.meat
    assert whole.score.tobytes() == ((parts[0].score + parts[1].score) + parts[2].score).tobytes()
    assert whole.information.tobytes() == ((parts[0].information + parts[1].information) + parts[2].information).tobytes()
    assert whole.q.tobytes() == ((parts[0].q + parts[1].q) + parts[2].q).tobytes()
    assert np.array_equal(whole.used, parts[0].used + parts[1].used + parts[2].used) and whole.used.dtype == np.int64
    one = M.normal_equations(X, sc, labels, D, coef, 0.2, 2.0).ne
    np.testing.assert_allclose(whole.score, one.score, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(whole.information, one.information, rtol=1e-12)
    assert "genes=5, p=3, cells=90" in repr(whole)
    with pytest.raises(ValueError, match="at least one"):
        regress.NormalEquations.concat([])
    with pytest.raises(TypeError, match="concat takes NormalEquations"):
        regress.NormalEquations.concat([parts[0], parts[0].score])
    meat = M.normal_equations(X[:30], sc[:30], labels[:30], D, coef, 0.2, 2.0, meat=True).ne
    with pytest.raises(ValueError, match="mix the information and the meat"):
        regress.NormalEquations.concat([parts[0], meat])
    fewer = M.normal_equations(X[:30, :4], sc[:30], labels[:30], D, coef[:4], 0.2, 2.0).ne
    with pytest.raises(ValueError, match="different genes or coefficients"):
        regress.NormalEquations.concat([parts[0], fewer])
    with pytest.raises(ValueError, match="score must be"):
        regress.NormalEquations(np.zeros((5, 3)), np.zeros((5, 3, 2)), np.zeros(5), np.zeros(5), 3)


def test_a_singular_gene_does_not_change_the_others():
    """numpy refuses a whole stack for one singular matrix; the fallback is gene by gene, the pseudo-inverse for that gene
    alone, so the other genes keep the bits they have without it."""
    rng = np.random.default_rng(0)
    A = rng.normal(size=(5, 3, 3))
    info, score = A @ A.transpose(0, 2, 1), rng.normal(size=(5, 3))
    solved, inverse = regress._solve(info, score), regress._inverse(info)
    info[2] = np.diag([2.0, 0.0, 0.0])
    again, inverse_again = regress._solve(info, score), regress._inverse(info)
    keep = [0, 1, 3, 4]
    assert again[keep].tobytes() == solved[keep].tobytes() and inverse_again[keep].tobytes() == inverse[keep].tobytes()
    np.testing.assert_allclose(again[2], [score[2, 0] / 2.0, 0.0, 0.0], rtol=1e-15)
    np.testing.assert_allclose(inverse_again[2], np.diag([0.5, 0.0, 0.0]), rtol=1e-15)


def test_genes_without_counts_and_separated_coefficients():
    """A gene without any count takes no part and comes back blank; a group whose cells hold no count of a gene drives its
    coefficient to the limit, where it is stopped and named; the robust covariance is the sandwich of one meat pass."""
    rng = np.random.default_rng(9)
    N, G, K = 200, 6, 3
    labels = rng.integers(0, K, size=N)
    sc = rng.lognormal(0, 0.3, size=N)
    X = rng.poisson(sc[:, None] * 4.0, size=(N, G))
    X[:, 2] = 0
    X[labels == 1, 4] = 0
    r = M.regression(X, sc, labels, regress.group_design(K), 0.1, 1.5, robust=True)
    assert r.no_counts.tolist() == [False, False, True, False, False, False]
    assert np.all(np.isnan(r.coef[2])) and np.all(np.isnan(r.cov[2])) and np.isnan(r.q[2]) and not r.converged[2] and r.rounds[2] == 0
    assert r.separated.tolist() == [False, False, False, False, True, False]
    assert r.coef[4, 1] == -regress.LIMIT and r.converged[4]
    assert r.converged[[0, 1, 3, 5]].all() and r.rounds.max() <= 25
    keep = [0, 1, 3, 5]
    at = M.normal_equations(X, sc, labels, np.eye(K), np.where(np.isnan(r.coef), 0.0, r.coef), 0.1, 1.5, meat=True).ne
    np.testing.assert_allclose(r.robust_cov[keep], r.cov[keep] @ at.information[keep] @ r.cov[keep], rtol=1e-12)
    np.testing.assert_allclose(r.se[keep], np.sqrt(np.diagonal(r.robust_cov[keep], axis1=1, axis2=2)), rtol=1e-15)
    start = regress.start_coefficients(np.eye(K), X.sum(axis=0), sc.sum())
    np.testing.assert_allclose(start[0], np.log(X[:, 0].sum() / sc.sum()), rtol=1e-12)
