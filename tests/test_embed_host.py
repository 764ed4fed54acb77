"""embed.pca's driver (prosstt_amd/embed.py: _randomized_pca) on a binary64 torch-CPU stand-in for the device operator,
against the exact SVD of the centred log1p(X / s); and the argument checks that refuse before any device use."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from prosstt_amd import device, embed  # noqa: E402


def synthetic(seed=20261016, N=3000, G=1500, rank=8):
    """NB counts around log-linear rank-8 means with lognormal size factors: (X int32, s)."""
    rng = np.random.default_rng(seed)
    s = rng.lognormal(0.0, 0.4, size=N)
    U = rng.normal(size=(N, rank))
    V = rng.normal(size=(rank, G)) * np.linspace(1.0, 0.3, rank)[:, None]
    log_mu = rng.normal(0.0, 1.0, size=G)[None, :] + 0.6 * (U @ V)
    mu = np.clip(s[:, None] * np.exp(log_mu), 1e-3, 1e4)
    r = 2.0
    X = rng.negative_binomial(r, r / (r + mu)).astype(np.int32)
    return X, s


class StandIn:
    """The operator's interface on a dense binary64 CPU matrix."""

    def __init__(self, A):
        self.A = torch.as_tensor(A, dtype=torch.float64)
        self.shape = tuple(A.shape)
        self.dtype = torch.float64
        self.device = torch.device("cpu")
        self.calls = []

    def matmul(self, W):
        assert W.dtype == self.dtype and W.shape == (self.shape[1], W.shape[1])
        self.calls.append(("matmul", W.clone()))
        return self.A @ W

    def rmatmul(self, Q):
        assert Q.dtype == self.dtype and Q.shape == (self.shape[0], Q.shape[1])
        self.calls.append(("rmatmul", None))
        return self.A.T @ Q

    def moments(self):
        return self.A.sum(dim=0).numpy(), (self.A * self.A).sum(dim=0).numpy()


@pytest.fixture(scope="module")
def problem():
    X, s = synthetic()
    A = np.log1p(X / s[:, None])
    Ac = A - A.mean(axis=0)
    U, S, Vt = np.linalg.svd(Ac, full_matrices=False)
    return dict(X=X, s=s, A=A, S=S, Vt=Vt, U=U)


def separated(S, k, l):
    """Indices i < k whose exact sigma is at least 2 sigma_{l+1} with 5 % relative gaps to both neighbours."""
    out = []
    for i in range(k):
        gap_lo = (S[i - 1] - S[i]) / S[i] if i > 0 else np.inf
        gap_hi = (S[i] - S[i + 1]) / S[i]
        if S[i] >= 2 * S[l] and gap_lo >= 0.05 and gap_hi >= 0.05:
            out.append(i)
    return out


def check_against_exact(p, ref, k, sv_tol, cos_tol, over_tol, evr_rtol=1e-9, mean_rtol=1e-12, min_separated=3,
                        captured=1 - 1e-3):
    """The checks shared with the device test: bounds on sigma, captured variance (unless ``captured`` is None: a flat
    noise floor past the leading components converges slowly), separated components, signs."""
    S, Vt = ref["S"], ref["Vt"]
    N = ref["A"].shape[0]
    l = min(k + 10, *ref["A"].shape)
    sv = p.singular_values
    assert sv.shape == (k,) and p.components.shape == (k, ref["A"].shape[1]) and p.scores.shape == (N, k)
    assert np.all(sv <= S[:k] * (1 + over_tol))
    if captured is not None:
        assert np.sum(sv ** 2) >= captured * np.sum(S[:k] ** 2)
    sep = separated(S, k, l)
    assert len(sep) >= min_separated, sep
    for i in sep:
        assert abs(sv[i] - S[i]) <= sv_tol * S[0], (i, sv[i], S[i])
        cos = abs(p.components[i] @ Vt[i])
        assert 1 - cos <= cos_tol, (i, 1 - cos)
    # sign convention: the loading of largest magnitude is positive; scores are flipped with their component
    top = np.argmax(np.abs(p.components), axis=1)
    assert np.all(p.components[np.arange(k), top] > 0)
    Ac = ref["A"] - ref["A"].mean(axis=0)
    for i in sep:
        np.testing.assert_allclose(p.scores[:, i], Ac @ p.components[i], rtol=0, atol=max(sv_tol, 1e-9) * 10 * S[0])
    # explained variance and its ratio by their definitions
    np.testing.assert_allclose(p.explained_variance, sv ** 2 / (N - 1), rtol=1e-15)
    total = np.sum(Ac * Ac) / (N - 1)
    np.testing.assert_allclose(p.explained_variance_ratio, p.explained_variance / total, rtol=evr_rtol)
    np.testing.assert_allclose(p.gene_mean, ref["A"].mean(axis=0), rtol=mean_rtol, atol=1e-15)
    return sep


def run(ref, k=30, n_iter=7, seed=0):
    op = StandIn(ref["A"])
    S1, S2 = op.moments()
    return embed._randomized_pca(op, S1, S2, k, n_iter, seed), op


def test_driver_matches_the_exact_svd(problem):
    p, op = run(problem)
    sep = check_against_exact(p, problem, 30, sv_tol=1e-9, cos_tol=1e-9, over_tol=1e-10)
    assert len(sep) >= 3
    # 2 n_iter + 2 products after the moments: the first product, 7 x 2 iterations, the final one
    assert [c for c, _ in op.calls] == ["matmul"] + ["rmatmul", "matmul"] * 7 + ["rmatmul"]


def test_explained_variance_ratio_from_the_moments(problem):
    p, op = run(problem, k=10, n_iter=4)
    S1, S2 = op.moments()
    N = problem["A"].shape[0]
    total = np.sum(S2 - N * (S1 / N) ** 2) / (N - 1)
    np.testing.assert_array_equal(p.explained_variance_ratio, p.explained_variance / total)
    assert 0 < p.explained_variance_ratio.sum() < 1


def test_seed_decides_the_test_matrix(problem):
    a, op_a = run(problem, k=12, n_iter=2, seed=5)
    b, _ = run(problem, k=12, n_iter=2, seed=5)
    c, op_c = run(problem, k=12, n_iter=2, seed=6)
    for f in embed.PCA._fields:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    G = problem["A"].shape[1]
    omega = np.random.default_rng(5).standard_normal((G, 22))
    np.testing.assert_array_equal(op_a.calls[0][1].numpy(), omega)
    assert not np.array_equal(op_c.calls[0][1].numpy(), omega)
    assert not np.array_equal(a.scores, c.scores)


def test_small_shapes_cap_the_panel():
    """l = min(k + 10, N, G): at k = N - 1 or k = G the panel is the whole small side."""
    rng = np.random.default_rng(3)
    A = np.log1p(rng.poisson(3.0, size=(40, 9)).astype(np.float64))
    op = StandIn(A)
    S1, S2 = op.moments()
    p = embed._randomized_pca(op, S1, S2, 9, 3, 0)
    assert op.calls[0][1].shape == (9, 9)
    Ac = A - A.mean(axis=0)
    S = np.linalg.svd(Ac, compute_uv=False)
    np.testing.assert_allclose(p.singular_values, S, rtol=1e-10, atol=1e-12 * S[0])


def test_host_arrays_are_refused():
    X, s = synthetic(N=20, G=10)
    with pytest.raises(TypeError):
        embed.pca(X, s)
    with pytest.raises(TypeError):
        embed.LogNormalized(X, s)
    with pytest.raises(TypeError):
        embed.pca(torch.as_tensor(X, dtype=torch.float32), s)
    with pytest.raises(ValueError, match="device"):
        embed.pca(torch.as_tensor(X), s, 5)                   # a CPU tensor
    with pytest.raises(ValueError, match="device"):
        embed.LogNormalized(torch.as_tensor(X), s)


def test_count_matrix_view_refusals():
    """device.CountMatrix, the checked view behind embed and summary: step 1 on any input, step 2 (on_device) after it."""
    X, _ = synthetic(N=20, G=10)
    with pytest.raises(TypeError, match="no CPU path"):
        device.CountMatrix(X, "caller")                                   # a host array
    with pytest.raises(TypeError, match="int32"):
        device.CountMatrix(torch.as_tensor(X, dtype=torch.int64), "caller")
    with pytest.raises(ValueError, match="dimensions"):
        device.CountMatrix(torch.as_tensor(X).reshape(4, 5, 10), "caller")
    with pytest.raises(TypeError):
        device.CountMatrix(device.PresentedCounts(X, np.arange(20)), "caller")
    order = np.arange(20)[::-1]
    for given, cell_of_row in ((torch.as_tensor(X), None), (device.PresentedCounts(torch.as_tensor(X), order), order)):
        m = device.CountMatrix(given, "caller")                           # step 1 accepts a CPU tensor
        assert (m.N, m.G) == (20, 10) and m.X.dtype == torch.int32
        assert m.cell_of_row is None if cell_of_row is None else np.array_equal(m.cell_of_row, cell_of_row)
        with pytest.raises(ValueError, match="caller needs a device tensor"):
            m.on_device()
    total = np.arange(20)
    assert device.to_plan_order(None, total)[0] is total
    got, = device.to_plan_order(order, total)
    assert np.array_equal(got, total[::-1]) and got is not total


@pytest.mark.parametrize("bad", ["short", "zero", "negative", "nan", "inf", "tiny", "below_domain", "domain_edge"])
def test_bad_size_factors_are_refused(bad):
    X, s = synthetic(N=20, G=10)
    s = s.copy()
    if bad == "domain_edge":                                 # s = 2^-94 (inv_size = 2^94) is the smallest accepted:
        s[3] = 2.0 ** -94                                    # refused only for the matrix being on the CPU
        with pytest.raises(ValueError, match="device") as e:
            embed.LogNormalized(torch.as_tensor(X), s)
        assert "size factor" not in str(e.value)
        assert embed._inverse_sizes(s, 20)[3] == np.float32(2.0 ** 94)
        with pytest.raises(ValueError, match="size factor"):
            embed._inverse_sizes(np.where(np.arange(20) == 3, 2.0 ** -94 * (1 - 2.0 ** -20), s), 20)
        return
    if bad == "short":
        s = s[:-1]
    elif bad == "zero":
        s[3] = 0.0
    elif bad == "negative":
        s[3] = -1.0
    elif bad == "nan":
        s[3] = np.nan
    elif bad == "inf":
        s[3] = np.inf
    elif bad == "below_domain":
        s[3] = 1e-30                                         # 1 / s is a finite float32 above 2^94: x / s can overflow
    else:
        s[3] = 1e-300                                        # 1 / s overflows float32
    with pytest.raises(ValueError, match="size factor"):
        embed.LogNormalized(torch.as_tensor(X), s)
    with pytest.raises(ValueError, match="size factor"):
        embed.pca(torch.as_tensor(X), s, 5)


@pytest.mark.parametrize("k", [0, -1, 11, 2.5])
def test_components_out_of_range(k):
    X, s = synthetic(N=20, G=10)                               # min(N, G, 118) = 10
    with pytest.raises(ValueError, match="n_components"):
        embed.pca(torch.as_tensor(X), s, k)


def test_components_cap_is_118():
    X = torch.zeros(200, 200, dtype=torch.int32)
    s = np.ones(200)
    with pytest.raises(ValueError, match="n_components"):
        embed.pca(X, s, 119)
    with pytest.raises(ValueError, match="n_iter"):
        embed.pca(X, s, 5, n_iter=-1)
    with pytest.raises(ValueError, match="two cells"):
        embed.pca(torch.zeros(1, 5, dtype=torch.int32), np.ones(1), 1)
    with pytest.raises(ValueError, match="device"):           # in range: refused only for being on the CPU
        embed.pca(X, s, 118)


@pytest.mark.parametrize("case", ["tall", "rank_deficient", "zero"])
def test_qr_factors(case):
    """embed._qr: Y = Q R with orthonormal Q for any condition, and Householder for a zero panel."""
    rng = np.random.default_rng(8)
    Y = rng.standard_normal((5000, 12)) * np.logspace(0, -6, 12)
    if case == "rank_deficient":
        Y[:, 7] = Y[:, 2] * 3.0
        Y[:, 11] = 0.0
    if case == "zero":
        Y[:] = 0.0
    Q, R = embed._qr(torch.as_tensor(Y))
    Q = Q.numpy()
    np.testing.assert_allclose(Q @ R, Y, rtol=0, atol=1e-13 * max(1.0, np.abs(Y).max()))
    if case == "tall":
        np.testing.assert_allclose(Q.T @ Q, np.eye(12), rtol=0, atol=1e-13)
