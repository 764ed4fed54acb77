"""The binary64 model of prosstt_amd.tsne (tests/tsne_model.py) against scikit-learn's own functions: the joint affinities
against ``_joint_probabilities_nn`` (whose bisection stops at an entropy tolerance of 1e-5, so the two agree to that) and
the gradient and objective against ``_kl_divergence`` (the exact method's, to rounding).  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sparse
from scipy.spatial.distance import squareform

import graph_model
import tsne_model

_t_sne = pytest.importorskip("sklearn.manifold._t_sne")

N, K, PERPLEXITY = 600, 90, 30.0


def test_joint_affinities_against_scikit_learn():
    case = graph_model.case(N, K)
    idx, d2 = case["idx"], case["d2"]
    P, beta = tsne_model.affinities(idx, d2, PERPLEXITY)
    order = np.argsort(idx, axis=1, kind="stable")
    distances = sparse.csr_matrix((np.take_along_axis(d2, order, axis=1).ravel(), np.take_along_axis(idx, order, axis=1).ravel(),
                                   np.arange(0, N * K + 1, K)), shape=(N, N))
    want = _t_sne._joint_probabilities_nn(distances, PERPLEXITY, 0)
    want.sort_indices()
    assert P.nnz == want.nnz == 60466
    np.testing.assert_array_equal(P.indptr, want.indptr)
    np.testing.assert_array_equal(P.indices, want.indices)
    worst = np.abs(P.data - want.data).max() / P.data.max()
    print("largest |P - scikit-learn's| / max P: %.3g" % worst)
    assert worst <= 2e-5
    assert abs(P.sum() - 1.0) <= 1e-12
    assert (P != P.T).nnz == 0                                    # symmetric to the bit
    assert P.diagonal().max() == 0.0
    cond = tsne_model.conditional(d2, PERPLEXITY)[0]
    perplexities = np.exp(tsne_model.row_entropy(d2, cond))
    print("largest |perplexity of a row - %g|: %.3g" % (PERPLEXITY, np.abs(perplexities - PERPLEXITY).max()))
    assert np.all(np.abs(perplexities - PERPLEXITY) <= 1e-9)
    assert np.all(np.abs(cond.sum(axis=1) - 1.0) <= K * 2.0 ** -52) and np.all(beta > 0)


def test_degenerate_rows():
    d2 = np.full((5, 14), 0.25, dtype=np.float32)
    cond, beta = tsne_model.conditional(d2, 4.0)
    assert np.all(cond == 1.0 / 14) and np.all(beta == 2.0 ** 64)


@pytest.mark.parametrize("c", [2, 3])
def test_gradient_and_objective_against_scikit_learn(c):
    case = graph_model.case(N, K)
    P, _ = tsne_model.affinities(case["idx"], case["d2"], PERPLEXITY)
    Y = np.random.default_rng(5 + c).standard_normal((N, c))
    got = tsne_model.gradient(P, Y, sums=True)
    kl, grad = _t_sne._kl_divergence(Y.ravel(), squareform(P.toarray(), checks=False), 1.0, N, c)
    grad = grad.reshape(N, c)
    worst = np.abs(got.grad - grad).max() / np.abs(grad).max()
    print("c = %d: gradient %.3g of its largest entry apart, KL %.3g relative" % (c, worst, abs(got.kl - kl) / kl))
    assert worst <= 1e-12
    assert abs(got.kl - kl) <= 1e-12 * kl
    # the sums that scale the device tests' bounds dominate what they bound
    assert np.all(np.abs(got.grad) <= 4.0 * (got.S_A + got.S_R / got.Z) * (1 + 1e-12))
    assert np.array_equal(got.L, np.diff(P.indptr))


def test_descent_improves_the_layout():
    import layout_model
    N, k = 300, 90
    case = tsne_model.case(N, k, PERPLEXITY)
    start, Y, shots = tsne_model.reference_run(N, k, PERPLEXITY, 500, "pca", keep=(0, 1, 7, 249, 250))
    assert sorted(shots) == [0, 1, 7, 249, 250] and np.array_equal(shots[0][0], start)
    before = layout_model.trustworthiness(case["P_panel"], start, 15)
    after = layout_model.trustworthiness(case["P_panel"], Y, 15)
    print("trustworthiness of the pca start %.4f, of the model's run %.4f" % (before, after))
    assert after >= 0.99 and before < after - 0.03
    assert tsne_model.gradient(case["P"], Y).kl < tsne_model.gradient(case["P"], start).kl
