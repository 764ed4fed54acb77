"""The numpy model of prosstt_amd.dpt (tests/dpt_model.py) against independent computations: the concordance sums against the
dense sign matrix, a head's tau against scipy's Kendall tau, and the whole call on the noisy Y against the truth of its
generator (the figures of DESIGN section 16).  The module under test must exist: the model describes it.  No GPU."""
import numpy as np
import pytest
import scipy.stats

import dpt_model

pytest.importorskip("torch")
from prosstt_amd import dpt  # noqa: E402,F401

TABLE, SLACK = dpt_model.TABLE, dpt_model.SLACK


def _sequences(N, kind, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "permutations":
        return rng.permutation(N).astype(np.int32), rng.permutation(N).astype(np.int32)
    return rng.integers(0, 4, N).astype(np.int32), rng.integers(0, 4, N).astype(np.int32)


@pytest.mark.parametrize("kind", ["permutations", "ties"])
def test_sums_against_the_dense_sign_matrix(kind):
    N = 200
    ru, rv = _sequences(N, kind)
    s = dpt_model.sign_matrix(ru, rv)
    assert np.array_equal(s, s.T) and set(np.unique(s)) <= {-1, 0, 1}
    lower, upper = dpt_model.concordance(ru[None], rv[None], block=64)
    assert lower.dtype == np.int64 and upper.dtype == np.int64
    assert np.array_equal(lower[0], np.tril(s, -1).sum(axis=1))
    assert np.array_equal(upper[0], np.triu(s, 1).sum(axis=1))
    # H(n) and T(n) are the sums over the pairs inside the head and inside the tail
    for n in (2, 57, 198):
        assert lower[0, :n].sum() == np.triu(s[:n, :n], 1).sum()
        assert upper[0, n:].sum() == np.triu(s[n:, n:], 1).sum()


def test_a_heads_tau_is_scipys():
    N = 200
    ru, rv = _sequences(N, "permutations", 3)
    lower, upper = dpt_model.concordance(ru[None], rv[None])
    for n in (5, 64, 195):
        head = lower[0, :n].sum() / (n * (n - 1) / 2)
        tail = upper[0, n:].sum() / ((N - n) * (N - n - 1) / 2)
        assert abs(head - scipy.stats.kendalltau(ru[:n], rv[:n]).statistic) <= 1e-15 * 4
        assert abs(tail - scipy.stats.kendalltau(ru[n:], rv[n:]).statistic) <= 1e-15 * 4
    cand, diff = dpt_model.split_diff(lower[0], upper[0], 5)
    assert cand[0] == 5 and cand[-1] == N - 5
    at = 59
    assert diff[at] == lower[0, :cand[at]].sum() / (cand[at] * (cand[at] - 1) / 2) - upper[0, cand[at]:].sum() / (
        (N - cand[at]) * (N - cand[at] - 1) / 2)


def test_identical_and_reversed_sequences():
    N = 37
    r = np.arange(N, dtype=np.int32)[None]
    lower, upper = dpt_model.concordance(r, r)
    assert np.array_equal(lower[0], np.arange(N)) and np.array_equal(upper[0], N - 1 - np.arange(N))
    lower, upper = dpt_model.concordance(r, r[:, ::-1])
    assert np.array_equal(lower[0], -np.arange(N)) and np.array_equal(upper[0], np.arange(N) + 1 - N)
    lower, upper = dpt_model.concordance(np.zeros_like(r), r)
    assert not lower.any() and not upper.any()


def test_tree_truth_replays_the_generator():
    import graph_model
    N, d, seed = 500, 10, 9
    arm, pos = dpt_model.tree_truth(N, d, seed)
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((3, d))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs[0] = -dirs[0]
    clean = 10 * pos[:, None] * dirs[arm]
    # the noise has standard deviation 0.3 per coordinate
    resid = graph_model.tree_points(N, d, seed) - clean
    assert abs(resid.std() - 0.3) < 0.02 and abs(resid.mean()) < 0.02


@pytest.mark.parametrize("N,k", list(TABLE))
def test_the_noisy_y(N, k):
    c = dpt_model.case(N, k)
    res = c["model"]
    tip_arms, sizes, share, agreement = dpt_model.structure(res, c["arm"])
    tau = scipy.stats.kendalltau(res["pseudotime"], c["time"]).statistic
    print("(%d, %d): tips %s in arms %s, groups %s, splits %s, share %.4f, agreement %.4f, tau %.4f"
          % (N, k, res["tips"], tip_arms, sizes, res["splits"], share, agreement, tau))
    assert sorted(tip_arms) == [0, 1, 2]
    assert min(sizes) > 0
    assert share >= TABLE[N, k][0] - SLACK
    assert agreement >= TABLE[N, k][1] - SLACK
    assert tau >= TABLE[N, k][2] - SLACK
    assert res["pseudotime"][c["root"]] == 0 and res["pseudotime"].max() == 1
