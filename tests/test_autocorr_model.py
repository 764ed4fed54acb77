"""The model of the autocorrelation step (tests/autocorr_model.py) pinned against independent evaluations, and
``autocorr.statistics`` with it: the sums against rational arithmetic, the permutation moments against the enumeration of all
5 040 permutations of seven cells, the NaN rules, and a planted case.  No GPU."""
import numpy as np
import pytest

pytest.importorskip("torch")

import autocorr_model as am  # noqa: E402
from prosstt_amd import autocorr  # noqa: E402

PLANTED_SEED = 3                 # see planted_case


def _small(seed, N=40, G=5, symmetric=False):
    """(A float32, csr, mu): random entries with zeros among them; a graph of about five entries per row with a hub row, an
    empty row, a self-loop and a stored zero."""
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.uniform(0.3, 6.0, size=G)[None, :], size=(N, G))
    A = am.entries32(X, rng.uniform(0.5, 2.0, size=N))
    W = np.where(rng.random((N, N)) < 5.0 / N, rng.uniform(1e-3, 1.0, size=(N, N)), 0.0)
    W[3, :] = rng.uniform(0.1, 1.0, size=N)
    W[5, :] = 0.0
    W[7, 7] = 0.5
    if symmetric:
        W = W + W.T
    indptr, indices, data = am.csr_of(W)
    data[2] = 0.0
    mu = A.astype(np.float64).sum(0) / N
    return A, (indptr, indices, data), mu


@pytest.mark.parametrize("rpb", [1, 16, 64])
@pytest.mark.parametrize("symmetric", [False, True])
def test_sums_against_rational_arithmetic(symmetric, rpb):
    A, csr, mu = _small(11, symmetric=symmetric)
    got = am.sums(A, *csr, mu, rpb)
    values, masses, counts = am.exact_sums(A, *csr, mu)
    for name, s, want, mass, n in zip(("cross", "sqdiff", "m2", "m4"), got, values, masses, counts):
        for g in range(A.shape[1]):
            err = abs(am.Fraction(float(s[g])) - want[g])
            assert err <= (n + 4) * am.Fraction(2) ** -53 * mass[g], (name, g, float(err / mass[g]))


def test_smooth_against_a_dense_product():
    A, (indptr, indices, data), _ = _small(12)
    W = am.dense(indptr, indices, data)
    raw = am.smooth(A, indptr, indices, data, False)
    np.testing.assert_allclose(raw, W @ A.astype(np.float64), rtol=2e-7, atol=0)
    mean = am.smooth(A, indptr, indices, data, True)
    d = W.sum(1)
    assert d[5] == 0 and not mean[5].any() and raw.dtype == mean.dtype == np.float32
    keep = d > 0
    np.testing.assert_allclose(mean[keep], (W @ A.astype(np.float64))[keep] / d[keep, None], rtol=2e-7, atol=0)


def _graph_sums(A, csr, mu, rpb=16):
    cross, sqdiff, m2, m4 = am.sums(A, *csr, mu, rpb)
    w0, s1, s2 = autocorr.graph_constants(*csr)
    return autocorr.GraphSums(A.shape[0], w0, mu, cross, sqdiff, m2, m4, s1, s2)


@pytest.mark.parametrize("symmetric", [True, False])
def test_permutation_moments_against_full_enumeration(symmetric):
    """All 5 040 permutations of seven cells: the mean and variance of I and C, to 1e-10 relative."""
    rng = np.random.default_rng(5 + symmetric)
    N = 7
    W = np.where(rng.random((N, N)) < 0.6, rng.uniform(0.1, 1.0, size=(N, N)), 0.0)
    if symmetric:
        W = np.triu(W, 1) + np.triu(W, 1).T
    np.fill_diagonal(W, 0.0)
    assert symmetric == bool(np.array_equal(W, W.T))
    x = rng.gamma(1.5, 1.0, size=N)
    mean_i, var_i, mean_c, var_c = am.permutation_moments(x, W)
    w0, s1, s2 = am.graph_constants(W)
    got = autocorr.graph_constants(*am.csr_of(W))
    np.testing.assert_allclose(got, (w0, s1, s2), rtol=1e-14)
    z = x - x.mean()
    b2 = N * np.sum(z ** 4) / np.sum(z * z) ** 2
    ei, vi, vc = autocorr.permutation_moments(N, w0, s1, s2, np.array([b2]))
    for name, have, want in (("E(I)", ei, mean_i), ("Var(I)", vi[0], var_i), ("E(C)", 1.0, mean_c), ("Var(C)", vc[0], var_c)):
        print("%s: formula %.17g, enumeration %.17g, relative difference %.2e" % (name, have, want, abs(have - want) / abs(want)))
        assert abs(have - want) <= 1e-10 * abs(want), name


def test_statistics_against_the_model():
    A, csr, mu = _small(13, N=60, G=8)
    A[:, 2] = A[0, 2]                                   # a constant gene: m2 = 0
    mu = A.astype(np.float64).sum(0) / 60
    gs = _graph_sums(A, csr, mu)
    st = autocorr.statistics(gs)
    live = np.arange(8) != 2
    assert gs.m2[2] == 0 and all(np.isnan(a[2]) for a in (st.morans_i, st.gearys_c, st.z_i, st.z_c, st.pvals, st.pvals_adj))
    assert np.array_equal(st.morans_i[live], am.morans_i(gs.cross, gs.m2, 60, gs.w_total)[live])
    assert np.array_equal(st.gearys_c[live], am.gearys_c(gs.sqdiff, gs.m2, 60, gs.w_total)[live])
    assert st.expected_i == -1.0 / 59
    # the dense definitions
    W = am.dense(*csr)
    A64 = A.astype(np.float64)[:, live]
    Z = A64 - mu[live]
    np.testing.assert_allclose(st.morans_i[live], 60 / W.sum() * np.einsum("ig,ij,jg->g", Z, W, Z) / (Z * Z).sum(0), rtol=1e-12)
    D = A64[:, None, :] - A64[None, :, :]
    np.testing.assert_allclose(st.gearys_c[live], 59 / (2 * W.sum()) * np.einsum("ijg,ij->g", D * D, W) / (Z * Z).sum(0), rtol=1e-12)
    import scipy.stats
    np.testing.assert_allclose(st.pvals[live], scipy.stats.norm.sf(st.z_i[live]), rtol=1e-15)
    assert np.all(np.isfinite(st.z_c[live])) and np.all(st.pvals_adj[live] >= st.pvals[live])
    # order: z_i descending, ties to the lower index, NaN last
    want = sorted(range(8), key=lambda g: (np.isnan(st.z_i[g]), -st.z_i[g] if not np.isnan(st.z_i[g]) else 0.0, g))
    assert list(st.order) == want and st.order[-1] == 2 and st.order.dtype == np.int64
    assert list(autocorr.statistics(gs, 3).order) == want[:3]
    tied = gs._replace(cross=np.full(8, gs.cross[0]), m2=np.full(8, gs.m2[0]), m4=np.full(8, gs.m4[0]))
    assert list(autocorr.statistics(tied).order) == list(range(8))
    for bad in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match="n_genes"):
            autocorr.statistics(gs, bad)
    with pytest.raises(TypeError):
        autocorr.statistics((1, 2, 3))


def test_nan_rules():
    A, csr, mu = _small(14, N=40, G=4)
    gs = _graph_sums(A, csr, mu)
    none = autocorr.statistics(gs._replace(w_total=0.0))
    assert all(np.all(np.isnan(a)) for a in (none.morans_i, none.gearys_c, none.z_i, none.z_c, none.pvals, none.pvals_adj))
    assert list(none.order) == [0, 1, 2, 3]
    few = autocorr.statistics(gs._replace(n_cells=3))                  # fewer than four cells: no variance
    assert np.all(np.isfinite(few.morans_i)) and np.all(np.isnan(few.z_i)) and np.all(np.isnan(few.z_c)) and few.expected_i == -0.5
    assert np.all(np.isnan(few.pvals)) and np.all(np.isnan(few.pvals_adj))


def planted_case(seed=PLANTED_SEED):
    """(X int32 (N, 2 H), s, csr, planted gene indices): cells on a path with a few chords; gene h < H has counts that
    follow a smooth program along the path, gene H + h holds the same counts in shuffled cell order.

    PLANTED_SEED = 3 is a seed for which, in the model, every planted gene's z_i exceeds every twin's and every twin has
    |z_i| < 4 (test_planted_genes_in_the_model asserts it)."""
    rng = np.random.default_rng(seed)
    N, H = 200, 12
    t = np.linspace(0.0, 1.0, N)
    phase, period = rng.uniform(0, 2 * np.pi, size=H), rng.uniform(0.5, 1.5, size=H)
    rate = 3.0 * (1.0 + np.sin(2 * np.pi * t[:, None] / period[None, :] + phase[None, :])) + 0.2
    s = rng.uniform(0.7, 1.4, size=N)
    planted = rng.poisson(rate * s[:, None])
    twins = np.stack([planted[rng.permutation(N), h] for h in range(H)], axis=1)
    csr = am.path_graph(N, [(0, 100, 0.5), (20, 180, 0.25), (60, 61, 2.0), (150, 199, 1.0)])
    return np.concatenate([planted, twins], axis=1).astype(np.int32), s, csr, np.arange(H)


def test_planted_genes_in_the_model():
    X, s, csr, planted = planted_case()
    A = am.entries32(X, s)
    mu = A.astype(np.float64).sum(0) / len(s)
    st = autocorr.statistics(_graph_sums(A, csr, mu, am.default_rows_per_block(len(s))))
    H = len(planted)
    print("planted z_i: min %.2f; twins z_i: min %.2f max %.2f" % (st.z_i[:H].min(), st.z_i[H:].min(), st.z_i[H:].max()))
    assert st.z_i[:H].min() > st.z_i[H:].max() and np.all(np.abs(st.z_i[H:]) < 4)
    assert set(st.order[:H]) == set(planted) and np.all(st.pvals_adj[:H] < 1e-6)
    assert np.all(st.gearys_c[:H] < 0.7) and np.all(st.z_c[:H] < -4)
