"""The numpy model of ptree (tests/ptree_model.py) and the host steps it shares with the package, each pinned on its own: d2
against tests/knn_model.py, the softmax sums against math.fsum and rational arithmetic, Prim's tree against scipy's minimum
spanning tree on distinct weights, the centre step against the energy's gradient, E non-increasing over the three steps of
every iteration up to a derived rounding term, k-means against a straightforward loop.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import knn_model
import ptree_model as pm

from prosstt_amd import ptree

EPS = 2.0 ** -53


@pytest.mark.parametrize("kind", ("gaussian", "scaled", "lattice"))
def test_d2_is_the_neighbour_searchs_distance(kind):
    P = knn_model.KINDS[kind](150, 7, 3)
    index, sq = knn_model.model(P, 9)
    D = pm.d2(P, P)
    assert D.dtype == np.float32
    assert np.array_equal(np.take_along_axis(D, index.astype(np.int64), axis=1).view(np.uint32), sq.view(np.uint32))
    best, m = pm.argmin_key(D)
    assert np.array_equal(best, np.argmin(D, axis=1)) and np.all(m == D.min(axis=1))


def test_softmax_sums_against_fsum_and_rational_arithmetic():
    rng = np.random.default_rng(1)
    for N, R, d in ((1, 1, 1), (5, 3, 2), (9, 70, 3), (140, 5, 2)):
        Y = rng.standard_normal((N, d)).astype(np.float32)
        C = rng.standard_normal((R, d)).astype(np.float32)
        sigma = 0.37
        a = pm.assign(Y, C, sigma)
        D = pm.d2(Y, C).astype(np.float64)
        w = np.array([[math.exp(-((D[i, k] - float(a.sq_distance[i])) / sigma)) for k in range(R)] for i in range(N)])
        depth = -(-R // 64) + 6
        for i in range(N):
            z = math.fsum(w[i])
            assert z >= 1.0
            assert abs(pm.butterfly_sum(w[i:i + 1])[0] - z) <= depth * EPS * z
            total = sum(Fraction(float(v)) for v in a.resp[i])
            assert abs(total - 1) <= Fraction((depth + 2) * EPS)
            assert abs(a.free_energy[i] - (float(a.sq_distance[i]) - sigma * math.log(z))) <= 1e-14 * (1 + abs(a.free_energy[i]))
        n = min(N, 128) + -(-N // 128)
        for k in range(R):
            exact = sum(Fraction(float(a.resp[i, k])) for i in range(N))
            assert abs(Fraction(float(a.gamma[k])) - exact) <= n * EPS * exact
            for c in range(d):
                terms = [Fraction(float(a.resp[i, k])) * Fraction(float(Y[i, c])) for i in range(N)]
                assert abs(Fraction(float(a.sums[k, c])) - sum(terms)) <= (n + 1) * EPS * sum(abs(t) for t in terms)


def test_hard_pass_counts_and_sums_exactly():
    Y, C = pm.eighths(300, 4, 1), pm.eighths(17, 4, 2)
    a = pm.assign(Y, C, 0.0)
    assert np.array_equal(a.gamma, np.bincount(a.best, minlength=17))
    for k in range(17):
        assert np.array_equal(a.sums[k], Y[a.best == k].astype(np.float64).sum(axis=0))
    assert np.array_equal(a.free_energy, a.sq_distance.astype(np.float64)) and np.array_equal(a.resp.sum(axis=1), np.ones(300))
    parts = ptree.Assignment.concat(pm.assign(Y[lo:lo + 128], C, 0.0) for lo in range(0, 300, 128))
    assert all(np.array_equal(x, y) for x, y in zip(parts, a))


@pytest.mark.parametrize("R", (2, 3, 30, 200))
def test_prims_tree_is_scipys_minimum_spanning_tree_on_distinct_weights(R):
    from scipy.sparse.csgraph import minimum_spanning_tree
    C = np.random.default_rng(R).standard_normal((R, 3)).astype(np.float32)
    D = ptree.centre_distances(C)
    assert np.array_equal(D, D.T) and len(np.unique(D[np.triu_indices(R, 1)])) == R * (R - 1) // 2
    edges = ptree.spanning_tree(C)
    assert edges.shape == (R - 1, 2) and edges.dtype == np.int32 and edges[0, 0] == 0
    want = minimum_spanning_tree(D).tocoo()
    assert {tuple(sorted(e)) for e in edges.tolist()} == {tuple(sorted(e)) for e in zip(want.row.tolist(), want.col.tolist())}
    assert math.fsum(D[edges[:, 0], edges[:, 1]]) == pytest.approx(want.data.sum(), rel=1e-14)
    seen = {0}
    for parent, child in edges.tolist():                                     # every edge grows the tree from node 0
        assert parent in seen and child not in seen
        seen.add(child)
    assert pm.prim_margin(D) > 0


def test_prims_ties_go_to_the_lowest_distance_parent_child():
    D = np.ones((5, 5)) - np.eye(5)                                          # every edge weighs 1
    assert ptree.prim(D).tolist() == [[0, 1], [0, 2], [0, 3], [0, 4]]
    C = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=np.float32)         # a unit square
    assert ptree.spanning_tree(C).tolist() == [[0, 1], [0, 2], [1, 3]]
    assert ptree.spanning_tree(C[:1]).shape == (0, 2)


def test_centre_step_zeroes_the_gradient_of_the_energy():
    Y, _, _ = pm.three_branches(400, 6, 2)
    C = pm.initial_centres(Y, 20, 1)
    a = pm.assign(Y, C, 0.3)
    edges = ptree.spanning_tree(C)
    lam = 0.4 * 400 / 20
    new = ptree.centre_step(a.gamma, a.sums, edges, lam, C)
    assert new.dtype == np.float32 and new.shape == C.shape
    A = np.diag(a.gamma) + lam * ptree.laplacian(20, edges)
    residual = A @ new.astype(np.float64) - a.sums                           # half the gradient
    assert np.all(np.abs(residual) <= (np.abs(A) @ np.abs(new.astype(np.float64))) * 2.0 ** -23)
    # an empty cluster at lam = 0 keeps its centre
    gamma = a.gamma.copy()
    gamma[7] = 0.0
    kept = ptree.centre_step(gamma, a.sums, edges, 0.0, C)
    assert np.array_equal(kept[7], C[7])
    others = np.arange(20) != 7
    assert np.array_equal(kept[others], (a.sums[others] / gamma[others, None]).astype(np.float32))


def _exact_energy(Y, C, edges, lam, sigma, r):
    """(E with the model's d2 at the given r, the sum of r d2)."""
    D = pm.d2(Y, C).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        entropy = np.where(r > 0, r * np.log(r), 0.0)
    fit = math.fsum((r * D).ravel().tolist())
    return fit + sigma * math.fsum(entropy.ravel().tolist()) + lam * ptree.tree_length(C, edges), fit


def test_energy_does_not_rise_over_the_three_steps_of_every_iteration():
    """The assignment, the spanning tree and the centre step each minimise E over their own variable.  What the arithmetic
    adds: d2 is a binary32 sum of d terms, within (d + 2) 2^-24 of the exact distance, so an energy is known to
    (d + 2) 2^-24 sum r d2; rounding the centres to binary32 moves the quadratic E from its minimum by at most
    2^-48 sum_c |C|^T |A| |C|."""
    N, d, R = 512, 10, 30
    Y, _, _ = pm.three_branches(N, d, 12)
    C = ptree.lloyd(Y, pm.initial_centres(Y, R, 0), lambda c: pm.assign(Y, c, 0.0, False), ptree.KMEANS_ITER).centres
    sigma = float(np.mean(pm.assign(Y, C, 0.0, False).sq_distance.astype(np.float64)))
    lam = ptree.LAM * N / R
    edges = ptree.spanning_tree(C)
    previous, drops = None, []
    for it in range(15):
        a = pm.assign(Y, C, sigma)
        e_assign, fit = _exact_energy(Y, C, edges, lam, sigma, a.resp)
        tol = 2 * (d + 2) * 2.0 ** -24 * fit + 1e-12 * abs(e_assign)
        assert abs(e_assign - ptree.energy(a.free_energy, C, edges, lam)) <= 1e-9 * abs(e_assign)   # sum F is that minimum
        if previous is not None:
            assert e_assign <= previous + tol, (it, "assign")
        new_edges = ptree.spanning_tree(C)
        e_tree = ptree.energy(a.free_energy, C, new_edges, lam)
        assert e_tree <= ptree.energy(a.free_energy, C, edges, lam) + 1e-12 * abs(e_tree), (it, "tree")
        new = ptree.centre_step(a.gamma, a.sums, new_edges, lam, C)
        e_centres, fit = _exact_energy(Y, new, new_edges, lam, sigma, a.resp)
        A = np.diag(a.gamma) + lam * ptree.laplacian(R, new_edges)
        n64 = np.abs(new.astype(np.float64))
        tol = 2 * (d + 2) * 2.0 ** -24 * fit + 2.0 ** -48 * float(np.sum(n64 * (np.abs(A) @ n64))) + 1e-12 * abs(e_centres)
        assert e_centres <= e_tree + tol, (it, "centres")
        drops.append(e_assign - e_centres)
        C, edges, previous = new, new_edges, e_centres
    assert drops[0] > 0 and sum(drops) > 0
    fitted = pm.principal_tree(Y, R)
    assert np.all(np.diff(fitted[2]) <= 1e-6 * np.abs(fitted[2][1:]))


def test_kmeans_against_a_straightforward_loop():
    Y = pm.eighths(400, 3, 5, span=40)                                       # exact sums: the order of a sum changes no bit
    k = 9
    C = pm.initial_centres(Y, k, 2)
    assert len(np.unique(C, axis=0)) == k or True
    centres = C.copy()
    labels = None
    for _ in range(100):
        D = pm.d2(Y, centres)
        new_labels = np.argmin(D, axis=1)
        if labels is not None and np.array_equal(new_labels, labels):
            break
        labels = new_labels
        for j in range(k):
            if np.any(labels == j):
                centres[j] = (Y[labels == j].astype(np.float64).sum(axis=0) / np.count_nonzero(labels == j)).astype(np.float32)
    km = pm.kmeans(Y, k, seed=2)
    assert km.converged and np.array_equal(km.labels, labels) and np.array_equal(km.centres, centres)
    assert km.inertia == pytest.approx(float(pm.d2(Y, centres).min(axis=1).astype(np.float64).sum()), rel=1e-12)
    zero = pm.kmeans(Y, k, n_iter=0, seed=2)
    assert zero.n_iter == 0 and not zero.converged and np.array_equal(zero.centres, C)
    # an empty cluster keeps its centre
    init = np.vstack([C[:2], np.full((1, 3), 1000.0, dtype=np.float32)])
    lone = pm.kmeans(Y, 3, init=init)
    assert np.array_equal(lone.centres[2], init[2]) and not np.any(lone.labels == 2)


def test_projection_on_a_segment():
    C = np.array([[0, 0], [4, 0], [4, 4]], dtype=np.float32)
    Y = np.array([[2, 1], [-3, 0], [5, 2], [4, 9], [2, 2]], dtype=np.float32)
    p = pm.project(Y, C, np.array([[0, 1], [1, 2], [1, 1]]))
    assert p.edge.tolist() == [0, 0, 1, 1, 0]                                # (2, 2) is as far from both: the lower edge
    assert p.t.tolist() == [0.5, 0.0, 0.5, 1.0, 0.5] and p.sq_distance.tolist() == [1.0, 9.0, 1.0, 25.0, 4.0]
    assert pm.project(Y, C, np.array([[1, 1]])).t.tolist() == [0.0] * 5     # an edge of zero length
