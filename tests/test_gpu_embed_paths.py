"""-m gpu: the embed kernels (prosstt_amd/csrc/embed/embed.hip) entry by entry, on every instantiation and in the regimes
that tests/test_embed_paths.py proves the cases reach (several steps of the pipelined loop in a block, a ragged last
step, several slabs, full and partial strips).

A panel with exactly one 1.0 per column makes a product exact: Y[i, c] = A[i, g_c], every other term is a * 0 and every
slab sum adds zeros.  So ceil(G / l) matmul calls (or ceil(N / l) rmatmul calls) with shifted selection panels return
the whole float32 matrix A32 = log1p(X / s) as the device formed it, and since entry() is a pure function of (x, inv)
every kernel, NT and VEC must return the same bits.  The comparisons of this module are therefore BIT FOR BIT between
instantiations (int32 views, on the device), 2^-20 relative against binary64 log1p(X / s) (the documented contract of
entry()), and N 2^-52 sum |A32| for the binary64 moments against the sums of the extracted A32."""
import numpy as np
import pytest

from test_embed_paths import DEEP, DEEP_LS, DEEP_VIEWS, MATRICES, PRODUCTS, SMALL, SMALL_VIEWS, case_id

pytestmark = pytest.mark.gpu

ENTRY_BOUND = 2.0 ** -20        # include/prosstt_amd_embed.h, embed.py, DESIGN section 11
FILL = 12345                    # the columns of the wider tensor outside a view: a read past the view shows


def _draw(N, G):
    """(X int32 host, s): NB(0.7, 0.1) counts, 8 % zeros on top of the NB's own, 4 % large values up to 2^31 - 1;
    lognormal size factors with some rows at 1e4.  Every A value is 0 or a normal float32."""
    rng = np.random.default_rng(N * 7919 + G)
    X = rng.negative_binomial(0.7, 0.1, size=(N, G)).astype(np.int64)
    kind = rng.random((N, G))
    X[kind < 0.08] = 0
    big = kind > 0.96
    X[big] = rng.integers(1 << 16, 1 << 31, size=int(big.sum()))
    X[kind > 0.998] = 2 ** 31 - 1
    s = rng.lognormal(0.0, 1.0, size=N)
    s[rng.random(N) < 0.05] = 1e4
    return X.astype(np.int32), s


_drawn, _views, _first = {}, {}, {}


def _host(N, G):
    if (N, G) not in _drawn:
        _drawn[N, G] = _draw(N, G)
    return _drawn[N, G]


def _view(N, G, pad, shift):
    """The (N, G) device view of the drawn matrix inside an (N, G + pad) tensor, at the alignment its id names."""
    import torch
    key = (N, G, pad, shift)
    if key not in _views:
        wide = torch.full((N, G + pad), FILL, dtype=torch.int32, device="cuda")
        assert wide.data_ptr() % 16 == 0
        wide[:, shift:shift + G] = torch.as_tensor(_host(N, G)[0]).cuda()
        _views[key] = wide[:, shift:shift + G]
        assert _views[key].data_ptr() % 16 == (4 * shift) % 16
    return _views[key]


def _operator(N, G, pad, shift):
    from prosstt_amd import embed
    return embed.LogNormalized(_view(N, G, pad, shift), _host(N, G)[1])


def _extract(op, kernel, l):
    """A32 (N, G) through selection panels of width l; a last, narrower panel is padded with zero columns, which must
    come back as zeros."""
    import torch
    N, G = op.shape
    out = torch.empty(N, G, dtype=torch.float32, device="cuda")
    cols = torch.arange(l, device="cuda")
    total = G if kernel == "matmul" else N                     # the panel's rows: genes (matmul) or cells (rmatmul)
    for k0 in range(0, total, l):
        w = min(l, total - k0)
        P = torch.zeros(total, l, dtype=torch.float32, device="cuda")
        P[k0 + cols[:w], cols[:w]] = 1.0
        if kernel == "matmul":
            Y = op.matmul(P)                                   # Y[i, c] = A[i, k0 + c]
            out[:, k0:k0 + w] = Y[:, :w]
        else:
            Y = op.rmatmul(P)                                  # Z[g, c] = A[k0 + c, g]
            out[k0:k0 + w, :] = Y[:, :w].T
        assert not bool(Y[:, w:].any()), (kernel, l, k0)
    return out


def _a32(N, G):
    """The first extraction of a drawn matrix: what every other one is compared with, and itself with binary64."""
    if (N, G) not in _first:
        pad, shift = DEEP_VIEWS[0] if (N, G) == DEEP else SMALL_VIEWS[0]
        _first[N, G] = _extract(_operator(N, G, pad, shift), "matmul", 128 if (N, G) == DEEP else 127)
    return _first[N, G]


def _a64(X, s):
    """binary64 log1p(X / s) on the device; X int32 device (N, G), s host binary64."""
    import torch
    return torch.log1p(X.double() / torch.as_tensor(s, device="cuda")[:, None])


def _assert_bits(got, want, what):
    import torch
    same = got.view(torch.int32) == want.view(torch.int32)
    if not bool(same.all()):
        at = (~same).nonzero()
        i, j = (int(v) for v in at[0])
        raise AssertionError("%s: %d of %d entries differ, the first at (%d, %d): %r, not %r"
                             % (what, at.shape[0], same.numel(), i, j, float(got[i, j]), float(want[i, j])))


def _assert_entries(a32, a64, zero, what):
    """|a32 - a64| <= 2^-20 a64 for every entry, finite, zeros exactly zero; prints the largest relative error."""
    import torch
    assert bool(torch.isfinite(a32).all()), what
    assert not bool(a32[zero].any()), what
    err = (a32.double() - a64).abs()
    rel = float((err / a64.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.0
    print("%s: max |a32 - a64| / a64 = %.4g = 2^%.2f" % (what, rel, np.log2(rel) if rel > 0 else -np.inf))
    assert bool((err <= ENTRY_BOUND * a64).all()), (what, rel)


EXTRACTIONS = [(kernel,) + case for case in PRODUCTS for kernel in ("matmul", "rmatmul")]


@pytest.mark.parametrize("kernel,N,G,pad,shift,l", EXTRACTIONS, ids=[case_id(*c) for c in EXTRACTIONS])
def test_every_instantiation_returns_the_same_entries(kernel, N, G, pad, shift, l):
    """Bit for bit: the extraction through this kernel, view and panel width against the first one."""
    what = case_id(kernel, N, G, pad, shift, l)
    got = _extract(_operator(N, G, pad, shift), kernel, l)
    _assert_bits(got, _a32(N, G), what)


@pytest.mark.parametrize("N,G", [DEEP] + SMALL)
def test_entries_are_log1p_to_2_to_the_minus_20(N, G):
    import torch
    X, s = _host(N, G)
    Xd = torch.as_tensor(X).cuda()
    _assert_entries(_a32(N, G), _a64(Xd, s), Xd == 0, "%d x %d" % (N, G))


def _through_identity(X, s):
    """A32 of a (N, l) matrix through one matmul with W = I."""
    import torch
    from prosstt_amd import embed
    Xd = torch.as_tensor(X).cuda()
    l = X.shape[1]
    return Xd, embed.LogNormalized(Xd, s).matmul(torch.eye(l, dtype=torch.float32, device="cuda"))


def test_corners_of_the_domain():
    """Counts at the ends of the float32 integer range against size factors over the whole domain [2^-94, 2^126]."""
    rng = np.random.default_rng(20)
    N, l = 2048, 64
    corners = [0, 1, 2, 3, 7, 255, 256, 65535, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 31 - 2,
               2 ** 31 - 1]
    X = rng.integers(0, 1 << 31, size=(N, l))
    X[:, :len(corners)] = np.asarray(corners)[None, :]
    t = np.clip(np.linspace(-94.0, 126.0, N) + rng.uniform(-0.5, 0.5, size=N), -94.0, 126.0)
    s = 2.0 ** t                                               # log-spaced, random mantissas
    s[0], s[-1] = 2.0 ** -94, 2.0 ** 126                       # both ends of the domain exactly
    Xd, Y = _through_identity(X.astype(np.int32), s)
    _assert_entries(Y, _a64(Xd, s), Xd == 0, "corners")


def test_sweep_of_the_argument():
    """y = x / s log-uniform over [2^-30, 2^8]: the u == 1 branch (y <= 2^-24), the band above it where u - 1 = 2^-23,
    and up.  Column 0 holds x uniform in [1, 2^31) with s = x / y; the other columns of a row hold round(y' s), y'
    log-uniform over the part of [2^-30, 2^8] that an int32 count reaches with the row's s."""
    rng = np.random.default_rng(21)
    N, l = 4096, 128
    x0 = rng.integers(1, 1 << 31, size=N).astype(np.float64)
    s = x0 / 2.0 ** rng.uniform(-30.0, 8.0, size=N)
    keep = (s >= 2.0 ** -94) & (s <= 2.0 ** 126)               # (all of them: 2^-8 <= s < 2^61)
    x0, s = x0[keep], s[keep]
    lo = np.maximum(-30.0, np.log2(1.0 / s))[:, None]
    hi = np.maximum(lo, np.minimum(8.0, np.log2((2.0 ** 31 - 1) / s))[:, None])
    X = np.rint(2.0 ** rng.uniform(lo, hi, size=(len(s), l)) * s[:, None])
    X[:, 0] = x0
    X = np.clip(X, 1, 2 ** 31 - 1).astype(np.int32)
    Xd, Y = _through_identity(X, s)
    a64 = _a64(Xd, s)
    y = np.expm1(a64.cpu().numpy())
    assert np.sum(y <= 2.0 ** -24) > 10000 and np.sum((y > 2.0 ** -24) & (y < 2.0 ** -22)) > 10000
    _assert_entries(Y, a64, Xd == 0, "sweep")


def _assert_moments(S, A32, what):
    """|S1 - sum A32| <= N 2^-52 sum |A32| and the same for the squares: twice the bound of recursive summation at
    unit roundoff 2^-53, the spare factor for the reference's own sum.  A32^2 is exact in binary64."""
    N = A32.shape[0]
    A = A32.double()
    for got, terms in zip(S, (A, A * A)):
        want = terms.sum(dim=0).cpu().numpy()
        bound = N * 2.0 ** -52 * terms.abs().sum(dim=0).cpu().numpy()
        assert np.all(np.abs(got - want) <= bound), (what, float(np.max(np.abs(got - want) - bound)))


@pytest.mark.parametrize("N,G,pad,shift", MATRICES, ids=[case_id("moments", *m) for m in MATRICES])
def test_moments_are_the_sums_of_the_exact_entries(N, G, pad, shift):
    _assert_moments(_operator(N, G, pad, shift).gene_moments(), _a32(N, G), case_id("moments", N, G, pad, shift))


def _assert_dense(got, A64, P, what):
    """|Y - A32.P| <= 2^-14 sum |A32||P| entrywise in binary64, on the device."""
    P64 = P.double()
    err = (got.double() - A64 @ P64).abs()
    bound = (A64.abs() @ P64.abs()) * 2.0 ** -14
    assert bool((err <= bound).all()), (what, float((err - bound).max()))


@pytest.mark.parametrize("l", DEEP_LS)
@pytest.mark.parametrize("pad,shift", DEEP_VIEWS)
def test_dense_products_where_the_loop_is_deep(pad, shift, l):
    import torch
    N, G = DEEP
    gen = torch.Generator(device="cuda").manual_seed(l)
    W = torch.randn(G, l, dtype=torch.float32, device="cuda", generator=gen)
    Q = torch.randn(N, l, dtype=torch.float32, device="cuda", generator=gen)
    op = _operator(N, G, pad, shift)
    A64 = _a32(N, G).double()
    _assert_dense(op.matmul(W), A64, W, case_id("matmul", N, G, pad, shift, l))
    _assert_dense(op.rmatmul(Q), A64.T, Q, case_id("rmatmul", N, G, pad, shift, l))


@pytest.mark.parametrize("N,G,l", [(129, 257, 33), DEEP + (96,)])
def test_presented_counts_directly(N, G, l):
    """Rows permuted: matmul's rows do not depend on where they lie (bit for bit the plan-ordered call); rmatmul sums
    the rows in another order (the dense bound); the moments likewise (their bound)."""
    import torch
    from prosstt_amd import device, embed
    X, s = _host(N, G)
    cell_of_row = np.random.default_rng(N).permutation(N)
    assert not np.array_equal(cell_of_row, np.arange(N))
    presented = device.PresentedCounts(torch.as_tensor(X[cell_of_row]).cuda(), cell_of_row)
    op = embed.LogNormalized(presented, s)
    plain = embed.LogNormalized(torch.as_tensor(X).cuda(), s)
    gen = torch.Generator(device="cuda").manual_seed(l)
    W = torch.randn(G, l, dtype=torch.float32, device="cuda", generator=gen)
    Q = torch.randn(N, l, dtype=torch.float32, device="cuda", generator=gen)
    _assert_bits(op.matmul(W), plain.matmul(W), "matmul of presented counts")
    A32 = _a32(N, G)
    _assert_dense(op.rmatmul(Q), A32.double().T, Q, "rmatmul of presented counts")
    _assert_moments(op.gene_moments(), A32, "moments of presented counts")


def test_negative_entry_on_the_deep_paths():
    """One -1 at (last row, last gene): in the ragged last step of the last block of every kernel."""
    import torch
    from prosstt_amd import embed
    N, G = DEEP
    s = _host(N, G)[1]
    clean = _view(N, G, *DEEP_VIEWS[0])
    wide = torch.full((N, G + 1), FILL, dtype=torch.int32, device="cuda")
    wide[:, :G] = clean
    bad = wide[:, :G]
    bad[N - 1, G - 1] = -1
    gen = torch.Generator(device="cuda").manual_seed(1)
    W = torch.randn(G, 96, dtype=torch.float32, device="cuda", generator=gen)
    Q = torch.randn(N, 128, dtype=torch.float32, device="cuda", generator=gen)
    before = embed.LogNormalized(clean, s).matmul(W)
    with pytest.raises(ValueError, match="negative"):
        embed.LogNormalized(bad, s).matmul(W)
    with pytest.raises(ValueError, match="negative"):
        embed.LogNormalized(bad, s).rmatmul(Q)
    with pytest.raises(ValueError, match="negative"):
        embed.LogNormalized(bad, s).gene_moments()
    fresh = embed.LogNormalized(clean, s)
    _assert_bits(fresh.matmul(W), before, "matmul after a refused call")
    fresh.rmatmul(Q)
    fresh.gene_moments()
