"""The numpy model of THIN-1 (tests/thin_model.py) itself, with fixed seeds and no device: its hash is splitmix64's stream, its
parts follow the binomial law, parts that should be independent are, the identities that make up the contract hold, and the
kernel's evaluation (the needed planes only, 64 trials per word) equals the plain definition.

The chi-square tests.  n entries in cells of expected count >= 5 (cells of the pmf are pooled from the tails until they are):
the statistic has df = cells - 1 (less one per stratum for the conditional law), mean df and variance 2 df; asserted below
df + 5 sqrt(2 df), the 5 sigma quantile of its law.  The correlations: two independent parts of n entries have a sample correlation of
standard deviation 1 / sqrt(n); asserted within 5 / sqrt(n)."""
import numpy as np
import pytest
from scipy import stats

import thin_model as T

N_LAW = 200_000
COUNTS = (1, 5, 63, 64, 65, 200)
BOUNDS = (32768, 16384, 3, 40000)

_cache = {}


def _uniforms(x):
    """U of N_LAW entries (cells 0 .. 399 x genes 0 .. 499, seed 11) with the count x, by the plain definition."""
    if x not in _cache:
        K = T.keys(11, np.arange(400)[:, None], np.arange(500)[None, :]).ravel()
        assert K.size == N_LAW
        _cache[x] = T.uniform_matrix(K, x)
    return _cache[x]


def _pooled(observed, expected):
    """Cells of expected count >= 5: pooled from both tails inward."""
    obs, exp = list(observed), list(expected)
    for side in (0, -1):
        while len(exp) > 1 and exp[side] < 5.0:
            o, e = obs.pop(side), exp.pop(side)
            obs[side] += o
            exp[side] += e
    return np.array(obs, dtype=np.float64), np.array(exp)


def _chi2(observed, expected):
    obs, exp = _pooled(observed, expected)
    assert exp.min() >= 5.0 or exp.size == 1
    return float(((obs - exp) ** 2 / exp).sum()), obs.size - 1


def test_the_hash_is_splitmix64s_stream():
    """splitmix64 from the state 0 gives 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F: words 0, 1, 2 of the key 0."""
    got = T.words(np.zeros(3, dtype=np.uint64), np.zeros(3, dtype=np.int64), np.arange(3))
    assert [int(v) for v in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    assert int(T.words(np.uint64(0), 1, 0)) == int(T.mix(np.uint64((17 * 0x9E3779B97F4A7C15) % (1 << 64))))
    # the key: a function of the seed, the cell and the gene, each of which changes it
    K = T.keys(5, np.arange(4)[:, None], np.arange(3)[None, :])
    assert K.shape == (4, 3) and len(set(K.ravel().tolist()) | set(T.keys(6, np.arange(4)[:, None], np.arange(3)[None, :]).ravel().tolist())) == 24
    assert T.planes_needed(0, 32768) == 1 and T.planes_needed(1, 65536) == 16 and T.planes_needed(0, 65536) == 0
    assert T.planes_needed(16384, 16384) == 2 and T.planes_needed(0, 12288) == 4 and T.planes_needed(0, 0) == 0


@pytest.mark.parametrize("x", COUNTS)
def test_the_parts_follow_the_binomial_law(x):
    U = _uniforms(x)
    for k in BOUNDS:
        y = (U < k).sum(axis=1)
        observed = np.bincount(y, minlength=x + 1)
        expected = N_LAW * stats.binom.pmf(np.arange(x + 1), x, k / T.GRID)
        stat, df = _chi2(observed, expected)
        print("x = %d, [0, %d): chi-square %.1f on %d degrees of freedom" % (x, k, stat, df))
        if df == 0:                                              # one cell holds everything expected: (x = 1, k = 3)
            assert abs(y.sum() - N_LAW * x * k / T.GRID) <= 5.0 * np.sqrt(N_LAW * x * k / T.GRID)
        else:
            assert stat <= df + 5.0 * np.sqrt(2.0 * df), (x, k, stat, df)


def _correlation(a, b):
    return float(np.corrcoef(a.astype(np.float64), b.astype(np.float64))[0, 1])


def test_parts_that_share_nothing_are_uncorrelated():
    n, x, k = N_LAW, 20, 32768
    cells, genes = np.arange(400)[:, None], np.arange(500)[None, :]
    X = np.full((400, 500), x)
    y = T.interval(X, 0, k, seed=3)
    bound = 5.0 / np.sqrt(n - 500)
    found = {
        "neighbouring genes": _correlation(y[:, :-1].ravel(), y[:, 1:].ravel()),
        "neighbouring cells": _correlation(y[:-1].ravel(), y[1:].ravel()),
        "two seeds": _correlation(y.ravel(), T.interval(X, 0, k, seed=4).ravel()),
    }
    U = T.uniform_matrix(T.keys(3, cells, genes).ravel(), 128)
    found["neighbouring words of one entry"] = _correlation((U[:, :64] < k).sum(axis=1), (U[:, 64:] < k).sum(axis=1))
    found["neighbouring planes' bounds"] = _correlation((U[:, :64] < 3).sum(axis=1), (U[:, 64:] < 40000).sum(axis=1))
    print(", ".join("%s %.5f" % item for item in found.items()), "(bound %.5f)" % bound)
    for name, r in found.items():
        assert abs(r) <= bound, (name, r)


def test_the_part_of_a_disjoint_interval_is_binomial_on_the_rest():
    """Given a trials in [lo, mid), the x - a others are uniform on the rest of the grid: the part [mid, hi) is
    Binomial(x - a, (hi - mid) / (65536 - (mid - lo)))."""
    x, lo, mid, hi = 5, 1000, 16384, 40000
    U = _uniforms(x)
    a = ((U >= lo) & (U < mid)).sum(axis=1)
    b = ((U >= mid) & (U < hi)).sum(axis=1)
    p = (hi - mid) / (T.GRID - (mid - lo))
    stat = df = 0
    for given in range(x + 1):
        sel = a == given
        if sel.sum() < 50:
            continue
        s, d = _chi2(np.bincount(b[sel], minlength=x - given + 1), sel.sum() * stats.binom.pmf(np.arange(x - given + 1), x - given, p))
        stat, df = stat + s, df + d
    print("conditional law: chi-square %.1f on %d degrees of freedom" % (stat, df))
    assert df >= 8 and stat <= df + 5.0 * np.sqrt(2.0 * df)


def _mixed_matrix(rng, N, G):
    X = rng.poisson(1.5, size=(N, G)) * (rng.random((N, G)) < 0.4)
    planted = (63, 64, 65, 127, 128, 129, 4096)
    X.ravel()[rng.choice(N * G, size=len(planted), replace=False)] = planted
    return X.astype(np.int64)


def test_the_identities():
    rng = np.random.default_rng(8)
    X = _mixed_matrix(rng, 23, 41)
    lo, mid, hi = 777, 30001, 65535
    whole = T.interval(X, lo, hi, seed=9)
    assert np.array_equal(T.interval(X, lo, mid, seed=9) + T.interval(X, mid, hi, seed=9), whole)
    assert np.array_equal(T.interval(X, 0, T.GRID, seed=9), X)
    assert np.array_equal(T.interval(X, 0, lo, seed=9) + whole + T.interval(X, hi, T.GRID, seed=9), X)
    for k in (0, 1, 32768, 65535, 65536):
        assert not T.interval(X, k, k, seed=9).any()
    assert np.all((0 <= whole) & (whole <= X))
    # per-row bounds: every row as with its own pair
    los, his = rng.integers(0, 30000, size=23), rng.integers(30000, 65537, size=23)
    rows = T.interval(X, los, his, seed=9)
    for r in (0, 7, 22):
        assert np.array_equal(rows[r], T.interval(X[r:r + 1], int(los[r]), int(his[r]), seed=9, cell_ids=[r])[0])
    # a cell and a gene keep their bits wherever they lie and whoever is beside them
    sub = T.interval(X[5:9, 10:20], lo, hi, seed=9, cell_ids=np.arange(5, 9), gene_ids=np.arange(10, 20))
    assert np.array_equal(sub, whole[5:9, 10:20])
    # an entry outside 0 .. 2^24 gives 0
    bad = X.copy()
    bad[0, 0], bad[1, 1] = -3, T.MAX_COUNT + 1
    got = T.interval(bad, lo, hi, seed=9)
    assert got[0, 0] == 0 and got[1, 1] == 0
    others = bad == X
    assert others.sum() == X.size - 2 and np.array_equal(got[others], whole[others])


def test_the_trials_of_a_smaller_count_are_a_prefix():
    K = T.keys(2, np.arange(50)[:, None], np.arange(3)[None, :]).ravel()
    long = T.uniform_matrix(K, 200)
    for x in (1, 63, 64, 65, 130):
        assert np.array_equal(T.uniform_matrix(K, x), long[:, :x])
    y = np.stack([T.parts(K, np.full(K.size, x), 100, 50000) for x in (10, 11, 64, 65)])
    assert np.all(np.diff(y, axis=0) >= 0) and np.all(y[1] - y[0] <= 1) and np.all(y[3] - y[2] <= 1)


@pytest.mark.parametrize("lo,hi", [(0, 32768), (32768, 65536), (0, 1), (0, 65535), (1, 65536), (0, 65536), (12345, 12345), (0, 16384),
                                   (0, 12288), (777, 30001), (0, 0), (65536, 65536), (16384, 49152)])
def test_the_kernels_evaluation_equals_the_plain_definition(lo, hi):
    rng = np.random.default_rng(lo + 3 * hi)
    X = _mixed_matrix(rng, 19, 37)
    assert np.array_equal(T.interval(X, lo, hi, seed=21, sliced=True), T.interval(X, lo, hi, seed=21))


def test_the_largest_count_by_both_evaluations():
    """2^24 trials, 2^18 words: under one plane and under sixteen."""
    K = T.keys(1, np.array([3]), np.array([4]))
    x = np.array([T.MAX_COUNT])
    for lo, hi in ((0, 32768), (1, 65536)):
        y = int(T.parts(K, x, lo, hi)[0])
        assert y == int(T.parts_sliced(K, x, lo, hi)[0])
        p = (hi - lo) / T.GRID
        assert abs(y - T.MAX_COUNT * p) <= 5.0 * np.sqrt(T.MAX_COUNT * p * (1 - p)) + 1
