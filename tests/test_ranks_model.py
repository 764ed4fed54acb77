"""The numpy model of the rank-sum step (tests/ranks_model.py) against scipy: the integers Q and T against ``rankdata``,
``tiecorrect`` and ``mannwhitneyu``'s statistic with equality, and the Wilcoxon z and p-values.  No GPU, and nothing of the
package."""
import numpy as np
import pytest
import scipy.stats

import ranks_model as rm

N, G, K = 300, 12, 4
ZERO, EQUAL = 3, 7              # an all-zero gene and a gene with one value in every cell


def _case(seed=0, empty=True):
    """(A float32 (N, G), labels): log1p of small Poisson counts over a few size factors (heavy ties, many zeros), an
    all-zero and an all-equal gene; labels in [-1, K) with about one cell in seven left out and, with ``empty``, no cell in
    group 1."""
    rng = np.random.default_rng(seed)
    s = rng.choice([0.5, 1.0, 2.0], size=N)
    X = rng.poisson(rng.uniform(0.3, 3.0, size=G)[None, :] * s[:, None])
    A = np.log1p(X / s[:, None]).astype(np.float32)
    A[:, ZERO] = 0.0
    A[:, EQUAL] = 1.25
    labels = rng.integers(0, K, size=N)
    if empty:
        labels[labels == 1] = 2
    labels[rng.random(N) < 0.15] = -1
    return A, labels


@pytest.mark.parametrize("seed", [0, 1])
def test_rank_sums_against_rankdata_and_tiecorrect(seed):
    A, labels = _case(seed)
    Q, T, n = rm.rank_sums(A, labels, K)
    keep = labels >= 0
    total = int(keep.sum())
    assert n.sum() == total and n[1] == 0 and not Q[1].any()            # an empty group gives zeros
    for j in range(G):
        ranks = scipy.stats.rankdata(A[keep, j])
        for k in range(K):
            twice = 2.0 * ranks[labels[keep] == k].sum()                    # midranks are halves: exact in binary64
            assert twice == Q[k, j] + n[k], (j, k)
        _, runs = np.unique(A[keep, j], return_counts=True)
        assert T[j] == int((runs.astype(np.int64) ** 3 - runs).sum())
        np.testing.assert_allclose(1.0 - T[j] / (float(total) ** 3 - total), scipy.stats.tiecorrect(ranks), rtol=1e-12, atol=0)
    assert T[ZERO] == total ** 3 - total and T[EQUAL] == total ** 3 - total
    assert np.array_equal(Q[:, ZERO], n * total) and np.array_equal(Q[:, ZERO], Q[:, EQUAL])


@pytest.mark.parametrize("reference", [0, 2, 1])
def test_a_reference_group_against_mannwhitneyu(reference):
    A, labels = _case(2)
    Q, T, n = rm.rank_sums(A, labels, K, reference=reference)
    if n[reference] == 0:
        assert not Q.any()                                                 # an empty counting set gives zeros
        return
    for j in range(G):
        for k in range(K):
            if n[k] == 0:
                continue
            u = scipy.stats.mannwhitneyu(A[labels == k, j], A[labels == reference, j], use_continuity=False, method="asymptotic")
            assert 2.0 * u.statistic == Q[k, j], (j, k)                     # U with half counts for ties
    # the rank sum of k within k and r together
    k = 3
    both = (labels == k) | (labels == reference)
    for j in range(G):
        ranks = scipy.stats.rankdata(A[both, j])
        assert 2.0 * ranks[labels[both] == k].sum() == Q[k, j] + n[k] * (n[k] + 1)


def test_wilcoxon_against_mannwhitneyu():
    A, labels = _case(3, empty=False)
    Q, T, n = rm.rank_sums(A, labels, K)
    st = rm.wilcoxon(Q, T, n, tie_correct=True)
    plain = rm.wilcoxon(Q, T, n)
    flat = (ZERO, EQUAL)
    for k in range(K):
        for j in range(G):
            if j in flat:                                                   # scipy divides 0 by 0; the definition: z = 0, p = 1
                assert st["z"][k, j] == 0 and st["pvals"][k, j] == 1 and plain["z"][k, j] == 0 and plain["pvals"][k, j] == 1
                continue
            own, rest = A[labels == k, j], A[(labels >= 0) & (labels != k), j]
            want = scipy.stats.mannwhitneyu(own, rest, use_continuity=False, method="asymptotic")
            np.testing.assert_allclose(st["pvals"][k, j], want.pvalue, rtol=1e-12, atol=0)
            assert (st["z"][k, j] > 0) == (want.statistic > len(own) * len(rest) / 2.0) or st["z"][k, j] == 0
            assert abs(plain["z"][k, j]) <= abs(st["z"][k, j])              # ties only ever shrink the variance
        np.testing.assert_allclose(st["pvals_adj"][k], scipy.stats.false_discovery_control(st["pvals"][k], method="bh"), rtol=1e-15)
    # against a reference group, without the tie term: the z of U
    ref = rm.wilcoxon(*rm.rank_sums(A, labels, K, reference=1), reference=1)
    assert not ref["z"][1].any()                                            # the reference against itself
    for k in (0, 2, 3):
        for j in range(G):
            n1, n2 = int((labels == k).sum()), int((labels == 1).sum())
            u = scipy.stats.mannwhitneyu(A[labels == k, j], A[labels == 1, j], use_continuity=False, method="asymptotic").statistic
            np.testing.assert_allclose(ref["z"][k, j], (u - n1 * n2 / 2.0) / np.sqrt(n1 * n2 * (n1 + n2 + 1.0) / 12.0), rtol=1e-12,
                                       atol=0)


def test_fewer_than_two_cells_and_the_pairwise_tie_term():
    Q, T = np.zeros((2, 3), dtype=np.int64), np.zeros(3, dtype=np.int64)
    with pytest.raises(ValueError):
        rm.wilcoxon(Q, T, [1, 5])
    with pytest.raises(ValueError):
        rm.wilcoxon(Q, T, [5, 1])
    with pytest.raises(ValueError):
        rm.wilcoxon(Q, T, [5, 5], reference=0, tie_correct=True)
