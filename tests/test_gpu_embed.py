"""-m gpu: the embed library (libprosstt_amd_embed.so through prosstt_amd/embed.py) against binary64 references: the
products A.W and A^T.Q and the gene moments over ragged, strided, unaligned and near-2^31 inputs and one matrix above
2^31 entries; bit-identical repeats on other streams; pca on a synthetic matrix and on the sampler's PresentedCounts
against the exact SVD; errors."""
import numpy as np
import pytest

from test_embed_host import check_against_exact, separated, synthetic

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 64, 65, 1000, 4097]
GS = [1, 3, 31, 32, 33, 1025, 5003]
LS = [1, 7, 32, 64, 100, 128]
KINDS = ["nb", "big", "zeros"]
# (N, G, l, pad, shift, kind): every N, G and l at least twice, pads and unaligned bases; the largest pairs kept few
CASES = [(NS[i % 7], GS[(3 * i + 1) % 7], LS[i % 6], (0, 1, 3, 64)[(i // 3) % 4], (i // 2) % 2, KINDS[i % 3])
         for i in range(21)] + [(4097, 5003, 64, 0, 0, "nb"), (1000, 1025, 128, 3, 1, "big"),
                                (1000, 1025, 65, 1, 0, "nb"), (65, 5003, 96, 3, 1, "big")]      # lp = 96: NT = 3


def _matrix(N, G, pad, shift, kind, seed):
    """(device view X, host int64 copy, size factors): a (N, G) column view of an (N, G + pad) tensor."""
    import torch
    rng = np.random.default_rng(seed)
    shift = shift if pad > 0 else 0
    width = G + pad
    if kind == "zeros":
        W = np.zeros((N, width), dtype=np.int32)
        W[rng.random((N, width)) < 0.01] = 1
    elif kind == "nb":
        W = rng.negative_binomial(0.7, 0.1, size=(N, width)).astype(np.int32)
    else:
        W = (2 ** 31 - 1 - rng.integers(0, 1000, size=(N, width))).astype(np.int32)
        W[rng.random((N, width)) < 0.2] = 0
        W[rng.random((N, width)) < 0.2] = 1
    s = rng.lognormal(0.0, 1.0, size=N)
    s[rng.random(N) < 0.05] = 1e4                                # tiny x / s: log1p's small-argument end
    D = torch.as_tensor(W).cuda()
    return D[:, shift:shift + G], W[:, shift:shift + G].astype(np.int64), s


def _assert_product(got, A, P, what):
    """|Y - Y64| <= 2^-14 sum |A||P| entrywise, with P the f32 panel's values."""
    P64 = P.astype(np.float64)
    want = A @ P64
    bound = np.abs(A) @ np.abs(P64) * 2.0 ** -14
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), (what, float(np.max(err - bound)))


@pytest.mark.parametrize("N,G,l,pad,shift,kind", CASES)
def test_products_and_moments(N, G, l, pad, shift, kind):
    import torch
    from prosstt_amd import embed
    X, host, s = _matrix(N, G, pad, shift, kind, N * 7919 + G * 13 + l)
    op = embed.LogNormalized(X, s)
    assert op.shape == (N, G)
    A = np.log1p(host / s[:, None])
    rng = np.random.default_rng(l)
    W = rng.standard_normal((G, l)).astype(np.float32)
    Q = rng.standard_normal((N, l)).astype(np.float32)
    Y = op.matmul(torch.as_tensor(W).cuda())
    Z = op.rmatmul(torch.as_tensor(Q).cuda())
    assert Y.shape == (N, l) and Z.shape == (G, l) and Y.dtype == Z.dtype == torch.float32
    _assert_product(Y.cpu().numpy(), A, W, "matmul")
    _assert_product(Z.cpu().numpy(), A.T, Q, "rmatmul")
    S1, S2 = op.gene_moments()
    R1, R2 = A.sum(axis=0), (A * A).sum(axis=0)
    assert np.all(np.abs(S1 - R1) <= 2.0 ** -19 * R1)
    assert np.all(np.abs(S2 - R2) <= 2.0 ** -18 * R2)


def test_repeats_and_streams_are_bit_identical():
    import torch
    from prosstt_amd import embed
    X, host, s = _matrix(4097, 1025, 3, 1, "nb", 11)
    op = embed.LogNormalized(X, s)
    rng = np.random.default_rng(2)
    W = torch.as_tensor(rng.standard_normal((1025, 50)).astype(np.float32)).cuda()
    Q = torch.as_tensor(rng.standard_normal((4097, 50)).astype(np.float32)).cuda()
    first = (op.matmul(W), op.rmatmul(Q), op.gene_moments())
    second = (op.matmul(W), op.rmatmul(Q), op.gene_moments())
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        third = (op.matmul(W), op.rmatmul(Q), op.gene_moments())
    st.synchronize()
    for other in (second, third):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
        for a, b in zip(first[2], other[2]):
            np.testing.assert_array_equal(a, b)


def test_above_2_to_the_31_entries():
    """110 000 x 20 000 (2.2e9 entries, 8.8 GB): byte and element offsets past 2^32 and 2^31; the reference is binary64
    on the device, chunk by chunk."""
    import torch
    from prosstt_amd import embed
    N, G, l = 110000, 20000, 8
    gen = torch.Generator(device="cuda").manual_seed(7)
    X = torch.randint(0, 6, (N, G), dtype=torch.int32, device="cuda", generator=gen)
    X[N - 3:, G - 5:] = 2 ** 31 - 2                              # the last entries, near 2^31
    s = np.random.default_rng(3).lognormal(0.0, 0.5, size=N)
    rng = np.random.default_rng(4)
    W = torch.as_tensor(rng.standard_normal((G, l)).astype(np.float32)).cuda()
    Q = torch.as_tensor(rng.standard_normal((N, l)).astype(np.float32)).cuda()
    op = embed.LogNormalized(X, s)
    Y, Z = op.matmul(W), op.rmatmul(Q)
    S1, S2 = op.gene_moments()
    sd = torch.as_tensor(s, device="cuda")
    W64, Q64 = W.double(), Q.double()
    Z64 = torch.zeros(G, l, dtype=torch.float64, device="cuda")
    Zb = torch.zeros_like(Z64)
    R1 = torch.zeros(G, dtype=torch.float64, device="cuda")
    R2 = torch.zeros_like(R1)
    for lo in range(0, N, 8192):
        hi = min(N, lo + 8192)
        A = torch.log1p(X[lo:hi].double() / sd[lo:hi, None])
        Yc = A @ W64
        bound = (A @ W64.abs()) * 2.0 ** -14
        assert bool(((Y[lo:hi].double() - Yc).abs() <= bound).all()), lo
        Z64 += A.T @ Q64[lo:hi]
        Zb += A.T @ Q64[lo:hi].abs()
        R1 += A.sum(dim=0)
        R2 += (A * A).sum(dim=0)
        del A
    assert bool(((Z.double() - Z64).abs() <= Zb * 2.0 ** -14).all())
    R1, R2 = R1.cpu().numpy(), R2.cpu().numpy()
    assert np.all(np.abs(S1 - R1) <= 2.0 ** -19 * R1)
    assert np.all(np.abs(S2 - R2) <= 2.0 ** -18 * R2)
    del X, op
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def problem():
    X, s = synthetic()
    A = np.log1p(X / s[:, None])
    U, S, Vt = np.linalg.svd(A - A.mean(axis=0), full_matrices=False)
    return dict(X=X, s=s, A=A, S=S, Vt=Vt, U=U)


def test_pca_of_the_synthetic_matrix(problem):
    import torch
    from prosstt_amd import embed
    X = torch.as_tensor(problem["X"]).cuda()
    p = embed.pca(X, problem["s"], 30, n_iter=7, seed=0)
    sep = check_against_exact(p, problem, 30, sv_tol=1e-5, cos_tol=1e-6, over_tol=1e-5, evr_rtol=1e-5,
                              mean_rtol=2.0 ** -19)
    assert len(sep) >= 3
    again = embed.pca(X, problem["s"], 30, n_iter=7, seed=0)
    for f in embed.PCA._fields:
        np.testing.assert_array_equal(getattr(p, f), getattr(again, f))


def test_pca_of_presented_counts():
    from prosstt_amd import device, workloads, simulation as sim, embed
    work = workloads.build("C2")
    np.random.seed(12)
    presented, pt, br, sc = sim.sample_density(work.tree, 3000, alpha=work.alpha, beta=work.beta, out="torch")
    assert isinstance(presented, device.PresentedCounts)
    assert not np.array_equal(presented.cell_of_row, np.arange(3000))
    sub = device.PresentedCounts(presented.counts[:, :1500], presented.cell_of_row)     # a strided view, rows permuted
    k = 20
    p = embed.pca(sub, sc, k)
    q = embed.pca(sub.in_plan_order(), sc, k)
    host = sub.to_host("numpy32")                                                        # plan order
    A = np.log1p(host / sc[:, None])
    U, S, Vt = np.linalg.svd(A - A.mean(axis=0), full_matrices=False)
    ref = dict(A=A, S=S, Vt=Vt, U=U)
    sep = separated(S, k, min(k + 10, *A.shape))
    assert len(sep) >= 1, S[:k + 11]
    check_against_exact(p, ref, k, sv_tol=1e-5, cos_tol=1e-6, over_tol=1e-5, evr_rtol=1e-5, mean_rtol=2.0 ** -19,
                        min_separated=1, captured=None)
    for i in sep:                                        # plan order: the same scores as from the plan-ordered matrix
        assert np.max(np.abs(p.scores[:, i] - q.scores[:, i])) <= 1e-5 * S[0]
        assert abs(p.singular_values[i] - q.singular_values[i]) <= 1e-5 * S[0]


def test_errors():
    import torch
    from prosstt_amd import embed
    X = torch.ones((64, 40), dtype=torch.int32, device="cuda")
    s = np.ones(64)
    bad = X.clone()
    bad[3, 7] = -1
    op = embed.LogNormalized(bad, s)
    W = torch.ones((40, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="negative"):
        op.matmul(W)
    with pytest.raises(ValueError, match="negative"):
        embed.LogNormalized(bad, s).rmatmul(torch.ones((64, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="negative"):
        embed.LogNormalized(bad, s).gene_moments()
    with pytest.raises(ValueError, match="negative"):
        embed.pca(bad, s, 3)
    with pytest.raises(ValueError, match="device"):
        embed.pca(X.cpu(), s, 3)
    good = embed.LogNormalized(X, s)
    np.testing.assert_allclose(good.matmul(W).cpu().numpy(), np.full((64, 4), 40 * np.log(2.0)), rtol=1e-6)
    for l in (0, 129):
        with pytest.raises(ValueError, match="l <="):
            good.matmul(torch.ones((40, l), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        good.matmul(torch.ones((41, 4), dtype=torch.float32, device="cuda"))
    with pytest.raises(TypeError):
        good.matmul(W.double())
    with pytest.raises(ValueError):
        good.matmul(W.cpu())
    with pytest.raises(TypeError):
        good.rmatmul(np.ones((64, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        embed.LogNormalized(X[:, ::2], s)
