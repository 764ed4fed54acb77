"""
CPU tests of the lineage model in oracle/nb_model.c (prnb_lineage_attempt, prnb_lineage_commit): the model that the
lineage kernels (K2) are held to bit for bit (-m gpu, tests/test_gpu_lineage_paths.py) is itself checked here
against an 80-bit long double statement of the operation, within rounding bounds derived below.

Notation: u = 2^-53 (binary64 unit roundoff), gamma(n) = n*u / (1 - n*u) (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1).  An fma-accumulated dot product of n terms is within gamma(n) * sum |a_i b_i| of
the exact one.
"""
import numpy as np
import pytest

from oracle import nb_model

U = 2.0 ** -53
LD = np.longdouble


def gamma(n, u=U):
    return n * u / (1 - n * u)


@pytest.fixture(scope="module", autouse=True)
def long_double():
    assert np.finfo(np.longdouble).nmant >= 63, "these tests need an 80-bit (or wider) long double as the exact reference"


def walk(rng, T, K):
    return rng.normal(0, 0.1, (T, K)).cumsum(axis=0) + np.log(rng.uniform(0.05, 1.5, K))


def coefficients(rng, K, G, zero_cols=()):
    H = rng.standard_gamma(0.05, (K, G))
    H[:, list(zero_cols)] = 0.0                  # constant genes: Pearson r is NaN in scipy, never counted
    return H


def centred_ld(P, steps):
    X = P[:steps].astype(LD)
    return X - X.sum(axis=0) / steps


def count_bound(P, S, H, common):
    """Per gene: exact centred covariance cov_g = sum_t x_t y_t in long double, and a bound on |model - exact|.

    With n = common, A_k = sum_t |P_tk| / n (the same for S: B_k), the model's centred entry is within
    gamma(n + 1) * (|Pc_tk| + A_k) of the exact one (sequential sum: gamma(n - 1) * n * A_k, the division and the
    subtraction one rounding each); its dot product x~_t is then within eps = gamma(n + K + 1) of X_t =
    sum_k (|Pc_tk| + A_k) |H_kg|, and so |x~_t y~_t - x_t y_t| <= (2 eps + eps^2) X_t Y_t.  The four chunks'
    fma sums and the three additions that join them add gamma(n + 3) * sum_t |x~_t y~_t|.  To first order the
    total is u * (3n + 2K + 5) * sum_t X_t Y_t <= 3u * (n + K + 2) * sum_t X_t Y_t; the bound below takes the
    constant 4 and n + K + 3, which covers the second-order terms and the long double's own rounding (2^-64)."""
    Pc, Sc = centred_ld(P, common), centred_ld(S, common)
    Hl = H.astype(LD)
    cov = ((Pc @ Hl) * (Sc @ Hl)).sum(axis=0)
    A = np.abs(P[:common]).astype(LD).sum(axis=0) / common
    B = np.abs(S[:common]).astype(LD).sum(axis=0) / common
    X = (np.abs(Pc) + A) @ np.abs(Hl)
    Y = (np.abs(Sc) + B) @ np.abs(Hl)
    bound = 4 * U * (common + H.shape[0] + 3) * (X * Y).sum(axis=0)
    return cov, bound


ATTEMPT_CASES = [
    # B, T, K, G, sibling lengths, constant genes
    (1, 40, 5, 700, [40], (3, 500)),
    (2, 60, 32, 1500, [20, 90, 1, 2], (0,)),
    (1, 3, 7, 400, [3, 5, 1], ()),
    (3, 97, 33, 900, [97, 50], (899,)),
    (1, 150, 64, 600, [200, 4], (10, 11)),
    (2, 1, 12, 300, [1, 8], (7,)),
]


@pytest.mark.parametrize("B,T,K,G,sib_T,zero", ATTEMPT_CASES)
def test_attempt_model_within_rounding_of_exact(B, T, K, G, sib_T, zero):
    rng = np.random.default_rng(B * 100003 + T * 101 + K)
    P = np.stack([walk(rng, T, K) for _ in range(B)])
    H = coefficients(rng, K, G, zero)
    sibs = [walk(rng, t, K) for t in sib_T]
    top, counts = nb_model.lineage_attempt(P, H, sibs)
    assert top.shape == (B,) and counts.shape == (B, len(sibs)) and counts.dtype == np.int64
    Hl = H.astype(LD)
    for b in range(B):
        # maximum: every dot product is within gamma(K) * sum_k |P_tk H_kg| of the exact one (the 1.01 covers the
        # long double's rounding of the reference, 2^-11 of binary64's)
        exact = P[b].astype(LD) @ Hl
        mag = np.abs(P[b]).astype(LD) @ np.abs(Hl)
        assert abs(LD(top[b]) - exact.max()) <= 1.01 * gamma(K) * mag.max()
        for j, S in enumerate(sibs):
            common = min(T, S.shape[0])
            if common == 1:                                   # one step: every series is constant, r is NaN
                assert counts[b, j] == 0
                continue
            cov, bound = count_bound(P[b], S, H, common)
            outside = np.abs(cov) > bound
            assert outside.mean() >= 0.99 - len(zero) / G, "the bound decides too few genes to test anything"
            neg, pos = outside & (cov < 0), outside & (cov > 0)
            # a gene's classification depends on its own column of H only: ask the model about subsets of genes
            if neg.any():
                assert nb_model.lineage_attempt(P[b:b + 1], H[:, neg], [S])[1][0, 0] == neg.sum()
            if pos.any():
                assert nb_model.lineage_attempt(P[b:b + 1], H[:, pos], [S])[1][0, 0] == 0
            assert neg.sum() <= counts[b, j] <= neg.sum() + (~outside).sum()
            if zero:
                assert nb_model.lineage_attempt(P[b:b + 1], H[:, list(zero)], [S])[1][0, 0] == 0


def test_attempt_model_batch_equals_single_attempts():
    rng = np.random.default_rng(5)
    P = np.stack([walk(rng, 30, 9) for _ in range(4)])
    H = coefficients(rng, 9, 333)
    sibs = [walk(rng, 12, 9), walk(rng, 45, 9)]
    top, counts = nb_model.lineage_attempt(P, H, sibs)
    for b in range(4):
        t1, c1 = nb_model.lineage_attempt(P[b:b + 1], H, sibs)
        assert t1[0] == top[b] and np.array_equal(c1[0], counts[b])
    t0, c0 = nb_model.lineage_attempt(P, H)
    assert np.array_equal(t0, top) and c0.shape == (4, 0)


@pytest.mark.parametrize("T,K,G", [(1, 1, 5), (2, 33, 129), (63, 32, 1000), (65, 64, 77), (7, 1024, 3)])
def test_commit_model_within_rounding_of_exact(T, K, G):
    rng = np.random.default_rng(T * 7919 + K)
    P = walk(rng, T, K)
    H = coefficients(rng, K, G, (0,))
    rel, gmax = nb_model.lineage_commit(P, H)
    exact = P.astype(LD) @ H.astype(LD)
    mag = np.abs(P).astype(LD) @ np.abs(H).astype(LD)
    assert np.all(np.abs(rel.astype(LD) - exact) <= 1.01 * gamma(K) * mag)
    assert np.array_equal(gmax, rel.max(axis=0))
    assert np.all(rel[:, 0] == 0.0)
    prior = rng.normal(0, 3, G)
    prior[::3] = np.inf                         # larger than every row: must survive
    prior[1::3] = -np.inf
    rel2, gmax2 = nb_model.lineage_commit(P, H, prior)
    assert np.array_equal(rel2, rel) and np.array_equal(gmax2, np.maximum(prior, rel.max(axis=0)))
    attempt_top = nb_model.lineage_attempt(P[None], H)[0][0]
    assert attempt_top == rel.max()            # the attempt's maximum is the commit's dot product
