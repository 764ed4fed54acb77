"""
-m gpu: every launch path of the lineage kernels (K2) bit for bit against the kernel-order model in
oracle/nb_model.c (prnb_lineage_attempt, prnb_lineage_commit; the model is checked against long double in
tests/test_lineage_model.py), plus gene_max, means_from_rel, the batched walk (K1), the host ports that use them, and
the device.Context wrappers' argument checks.

Which kernel a call reaches (prosstt_amd_lineage_attempt_batch / _lineage_commit in prosstt_amd.hip):
  attempt  "lds"   K <= 32 and max(T, 2 * common_j) * K <= 6144   (lineage_attempt_lds_kernel)
           "hreg"  K <= 32 otherwise                             (lineage_attempt_kernel<true>)
           "gmem"  K > 32                                        (lineage_attempt_kernel<false>)
  commit   "hreg"  K <= 32 (lineage_commit_kernel<true>),  "gmem"  K > 32 (<false>)
test_cases_reach_every_kernel keeps at least two cases on each.  NaN in the inputs is outside the contract (the kernels'
fmax drops a NaN where numpy's max would return it) and is not tested.
"""
import numpy as np
import pytest

from oracle import nb_model

pytestmark = pytest.mark.gpu

ATT_LDS_DOUBLES = 6144
FLT_MIN = np.float32(1.17549435e-38)
U = 2.0 ** -53
LD = np.longdouble


def attempt_kernel(T, K, sib_T):
    need = max([T] + [2 * min(T, s) for s in sib_T]) * K
    if K <= 32:
        return "lds" if need <= ATT_LDS_DOUBLES else "hreg"
    return "gmem"


def commit_kernel(K):
    return "hreg" if K <= 32 else "gmem"


@pytest.fixture(scope="module")
def ctx():
    from prosstt_amd import device
    return device.get_context()


def walk(rng, T, K):
    return rng.normal(0, 0.1, (T, K)).cumsum(axis=0) + np.log(rng.uniform(0.05, 1.5, K))


def coefficients(rng, K, G):
    H = rng.standard_gamma(0.05, (K, G))
    if G > 2:
        H[:, G // 2] = 0.0                       # a constant gene: r is NaN, never counted
    return H


def dev(ctx, a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=ctx.torch_device)


# B, T, K, G, sibling lengths (an int n: n siblings of random lengths 1..40)
ATTEMPT_CASES = [
    (1, 192, 32, 129, [50, 96]),           # T*K = 6144: the LDS kernel's bound, reached
    (1, 193, 32, 129, [50]),               # one step past it: <true>
    (3, 256, 24, 128, [128, 20]),          # 256*24 = 6144 and 2*128*24 = 6144: LDS
    (1, 257, 24, 4097, [3]),               # <true>
    (1, 150, 32, 1000, [96]),              # common = 96: 2*96*32 = 6144, LDS
    (1, 150, 32, 1000, [97]),              # common = 97: 6208, <true>
    (300, 5, 2, 65, [3, 9]),
    (1, 1, 1, 1, [1]),
    (3, 2, 31, 2, [5, 1]),
    (1, 300, 31, 63, [400, 2]),            # siblings longer than T: <true>
    (1, 3, 33, 127, [2, 10]),
    (3, 300, 64, 64, [150, 300, 1]),
    (1, 300, 1, 4097, [299, 301]),
    (1, 20, 5, 300, 64),                   # the 64-sibling limit
    (300, 3, 64, 129, [2]),
    (1, 300, 32, 4097, [200]),
    (3, 97, 33, 1000, [97, 96, 1]),
    (1, 2, 64, 65, [1, 2, 3]),
    (2, 1, 33, 128, [1, 5]),
    (1, 5, 2, 128, 64),
]


def sibling_lengths(rng, sib):
    return [int(n) for n in rng.integers(1, 41, sib)] if isinstance(sib, int) else list(sib)


def attempt_inputs(case):
    B, T, K, G, sib = case
    rng = np.random.default_rng(B * 1000003 + T * 1009 + K * 31 + G)
    P = np.stack([walk(rng, T, K) for _ in range(B)])
    H = coefficients(rng, K, G)
    sibs = [walk(rng, n, K) for n in sibling_lengths(rng, sib)]
    return P, H, sibs


def test_cases_reach_every_kernel():
    rng = np.random.default_rng(0)
    att = [attempt_kernel(c[1], c[2], sibling_lengths(rng, c[4])) for c in ATTEMPT_CASES]
    assert all(att.count(k) >= 2 for k in ("lds", "hreg", "gmem")), att
    com = [commit_kernel(c[1]) for c in COMMIT_CASES]
    assert all(com.count(k) >= 2 for k in ("hreg", "gmem")), com


@pytest.mark.parametrize("case", ATTEMPT_CASES, ids=lambda c: "B%d-T%d-K%d-G%d" % c[:4])
def test_attempt_matches_model(ctx, case):
    P, H, sibs = attempt_inputs(case)
    top, counts = ctx.lineage_attempt_batch(P, dev(ctx, H), sibs)
    want_top, want_counts = nb_model.lineage_attempt(P, H, sibs)
    np.testing.assert_array_equal(top, want_top)
    np.testing.assert_array_equal(counts, want_counts)


@pytest.mark.parametrize("T,K,sib_T", [(60, 8, [30, 70]), (193, 32, [10]), (40, 40, [40])])
def test_batch_equals_single_attempts(ctx, T, K, sib_T):
    rng = np.random.default_rng(T + K)
    P = np.stack([walk(rng, T, K) for _ in range(3)])
    H = coefficients(rng, K, 300)
    sibs = [walk(rng, n, K) for n in sib_T]
    Hd = dev(ctx, H)
    top, counts = ctx.lineage_attempt_batch(P, Hd, sibs)
    for b in range(3):
        mx, c = ctx.lineage_attempt(P[b], Hd, sibs)
        assert mx == top[b] and c == [int(x) for x in counts[b]]


def test_max_and_counts_do_not_depend_on_the_kernel(ctx):
    """Same (P, H): the LDS kernel with sibling S1, <true> with [S1, S_long] (common 130: 2*130*32 > 6144), and
    <false> with a zero program column and a zero row of H added (fma(0, 0, acc) == acc, centred 0 stays 0)."""
    rng = np.random.default_rng(11)
    T, K, G = 150, 32, 1000
    P = np.stack([walk(rng, T, K) for _ in range(2)])
    H = coefficients(rng, K, G)
    S1, S_long = walk(rng, 90, K), walk(rng, 130, K)
    assert attempt_kernel(T, K, [90]) == "lds" and attempt_kernel(T, K, [90, 130]) == "hreg"
    Hd = dev(ctx, H)
    top_lds, c_lds = ctx.lineage_attempt_batch(P, Hd, [S1])
    top_hreg, c_hreg = ctx.lineage_attempt_batch(P, Hd, [S1, S_long])
    np.testing.assert_array_equal(top_lds, top_hreg)
    np.testing.assert_array_equal(c_lds[:, 0], c_hreg[:, 0])
    pad = lambda a: np.concatenate([a, np.zeros(a.shape[:-1] + (1,))], axis=-1)
    H33 = np.concatenate([H, np.zeros((1, G))])
    assert attempt_kernel(T, K + 1, [90, 130]) == "gmem"
    top_g, c_g = ctx.lineage_attempt_batch(pad(P), dev(ctx, H33), [pad(S1), pad(S_long)])
    np.testing.assert_array_equal(top_g, top_hreg)
    np.testing.assert_array_equal(c_g, c_hreg)
    want_top, want_counts = nb_model.lineage_attempt(P, H, [S1, S_long])
    np.testing.assert_array_equal(top_hreg, want_top)
    np.testing.assert_array_equal(c_hreg, want_counts)


# T, K, G: K = 1024 leaves one step per LDS range; (2049, 64, 1000) has its ranges cut short by the 2048-double bound
COMMIT_CASES = [(1, 1, 5), (2, 32, 129), (63, 1, 20001), (63, 33, 1000), (65, 64, 4097), (2049, 33, 70),
                (2049, 64, 1000), (65, 1024, 100), (2, 1024, 3)]


def mixed_prior(rng, rel):
    """-inf, values above every row (they must survive) and values inside the rows' range, gene by gene."""
    G = rel.shape[1]
    prior = np.empty(G)
    prior[0::3] = -np.inf
    prior[1::3] = rel.max(axis=0)[1::3] + 1.0
    prior[2::3] = np.median(rel, axis=0)[2::3]
    return prior


@pytest.mark.parametrize("mode", ["both", "rel", "max"])
@pytest.mark.parametrize("T,K,G", COMMIT_CASES)
def test_commit_matches_model(ctx, T, K, G, mode):
    import torch
    rng = np.random.default_rng(T * 7 + K * 3 + G)
    P = walk(rng, T, K)
    H = coefficients(rng, K, G)
    want_rel, _ = nb_model.lineage_commit(P, H)
    prior = mixed_prior(rng, want_rel)
    _, want_max = nb_model.lineage_commit(P, H, prior)
    sentinel = -12345.5
    big = torch.full((T + 5, G), sentinel, dtype=torch.float64, device=ctx.torch_device)
    gmax = dev(ctx, prior) if mode != "rel" else None
    ctx.lineage_commit(P, dev(ctx, H), big[2:2 + T] if mode != "max" else None, gmax)
    big = big.cpu().numpy()
    assert np.all(big[:2] == sentinel) and np.all(big[2 + T:] == sentinel)   # outside the row slice: untouched
    if mode == "max":
        assert np.all(big == sentinel)
    else:
        np.testing.assert_array_equal(big[2:2 + T], want_rel)
    if gmax is not None:
        np.testing.assert_array_equal(gmax.cpu().numpy(), want_max)


def test_commit_prior_kinds_and_refusal(ctx):
    import torch
    from prosstt_amd import _native
    rng = np.random.default_rng(2)
    T, K, G = 65, 40, 777
    P, H = walk(rng, T, K), coefficients(rng, K, G)
    Hd = dev(ctx, H)
    rel, _ = nb_model.lineage_commit(P, H)
    for prior in (np.full(G, -np.inf), rel.max(axis=0) + 0.5, np.full(G, np.inf)):
        gmax = dev(ctx, prior)
        ctx.lineage_commit(P, Hd, None, gmax)
        np.testing.assert_array_equal(gmax.cpu().numpy(), np.maximum(prior, rel.max(axis=0)))
    # 1025 programs: the library refuses (2 * K doubles per step exceed the LDS range) and writes nothing
    K = 1025
    P, H = walk(rng, 3, K), coefficients(rng, K, 64)
    out = torch.full((3, 64), 7.0, dtype=torch.float64, device=ctx.torch_device)
    gmax = torch.full((64,), -3.0, dtype=torch.float64, device=ctx.torch_device)
    with pytest.raises(_native.NativeError):
        ctx.lineage_commit(P, dev(ctx, H), out, gmax)
    assert bool((out == 7.0).all()) and bool((gmax == -3.0).all())


@pytest.mark.parametrize("G", [0, 1, 63, 64, 65, 20001])
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 5, 15, 16, 17, 1000, 4099])
def test_gene_max_kernel(ctx, rows, G):
    import torch
    rng = np.random.default_rng(rows * 100 + G)
    if rows * G > 3e7:                      # (4099 x 20001: 656 MB for nothing the smaller ones do not test)
        G = 4097
    rel = rng.normal(0, 5, (rows, G))
    if rows > 2:
        rel[rows // 2] = -np.inf            # a row of -inf
        rel[:, ::5] = -np.abs(rel[:, ::5]) - 1.0     # all-negative genes
    if rows and G > 1:
        rel[:, 1] = -np.inf                 # a gene that is -inf in every row
    prior = np.full(G, -np.inf)
    if rows and G:
        prior = mixed_prior(rng, np.where(np.isinf(rel), -50.0, rel))
    gmax = dev(ctx, prior) if G else torch.empty(0, dtype=torch.float64, device=ctx.torch_device)
    out = ctx.gene_max(dev(ctx, rel) if rel.size else torch.empty((rows, G), dtype=torch.float64, device=ctx.torch_device), gmax)
    assert out is gmax
    want = np.maximum(prior, rel.max(axis=0)) if rows else prior
    np.testing.assert_array_equal(gmax.cpu().numpy(), want)


def correctly_rounded_f32(exact):
    """(r, far): r = the binary32 nearest to the long double ``exact`` wherever far is True, i.e. where ``exact`` lies
    more than 8 * 2^-53 (relative) from a binary32 rounding boundary.  The device's binary64 exp(rel) * base is within
    3 * 2^-53 of exact (an exp within one ulp, one product rounding), so there its one conversion must give r.  Rounding
    through binary64 first moves a value by at most 2^-53: it cannot cross a boundary that is farther away."""
    r = exact.astype(np.float64).astype(np.float32)
    lo, hi = np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(np.inf))
    mid_lo = (r.astype(LD) + lo.astype(LD)) / 2
    mid_hi = (r.astype(LD) + hi.astype(LD)) / 2
    d = np.minimum(np.abs(exact - mid_lo), np.abs(exact - mid_hi)) / exact
    return r, d > 8 * U


@pytest.mark.parametrize("rows,G,lo,hi", [(7, 129, -60.0, 60.0), (300, 20001, -40.0, 40.0), (33, 65, -120.0, -80.0)])
def test_means_from_rel_one_rounding(ctx, rows, G, lo, hi):
    """300 x 20001 runs past the kernel's 2,097,152-thread grid (grid-stride loop, i % G); the last case crosses
    binary32's smallest normal, below which a positive mean is stored as FLT_MIN."""
    rng = np.random.default_rng(rows + G)
    rel = rng.uniform(lo, hi, (rows, G))
    base = np.exp(rng.normal(0.0, 2.0, G))
    got = ctx.means_from_rel(dev(ctx, rel), dev(ctx, base)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (rows, G)
    exact = np.exp(rel.astype(LD)) * base.astype(LD)[None, :]
    r, far = correctly_rounded_f32(exact)
    tiny = exact < LD(1.17549435e-38)
    far &= np.abs(exact / LD(1.17549435e-38) - 1) > 8 * U       # (the clamp's own threshold, in binary64)
    want = np.where(tiny, FLT_MIN, r)
    assert far.mean() > 0.99
    np.testing.assert_array_equal(got[far], want[far])
    near = ~far
    assert np.all((got[near] == want[near]) | (got[near] == np.nextafter(want[near], np.float32(0)))
                  | (got[near] == np.nextafter(want[near], np.float32(np.inf))))
    if lo < -87:
        assert tiny.any() and (~tiny).any()


def test_means_from_rel_zero_and_clamp(ctx):
    rel = np.array([[-800.0, -100.0, -87.0, 0.0, 3.0]])
    base = np.array([1.0, 1.0, 1.0, 0.0, 2.0])
    got = ctx.means_from_rel(dev(ctx, rel), dev(ctx, base)).cpu().numpy()[0]
    assert got[0] == 0.0 and not np.signbit(got[0])     # binary64 zero: stays zero
    assert got[1] == FLT_MIN                            # positive below FLT_MIN
    assert got[2] == np.float32(np.exp(-87.0)) and got[2] > FLT_MIN
    assert got[3] == 0.0 and got[4] == np.float32(2.0 * np.exp(3.0))


@pytest.mark.parametrize("T", [1, 2, 3, 100])
@pytest.mark.parametrize("K", [2, 64, 65, 200])
def test_walk_batches_match_model(ctx, T, K):
    seed = 2 ** 64 - 1
    first = (5 << 32) | 0xFFFFFFFE                     # the batch crosses the carry into the high word
    ids = [first + i for i in range(4)]
    got = ctx.lineage_walks(seed, ids, T, K)
    assert got.shape == (4, T, K)
    for i, sid in enumerate(ids):
        np.testing.assert_array_equal(got[i], nb_model.lineage_walk(seed, sid, T, K))
    scattered = [first + 3, 7, first, 2 ** 64 - 1]     # not consecutive: one launch each
    got = ctx.lineage_walks(seed, scattered, T, K)
    for i, sid in enumerate(scattered):
        np.testing.assert_array_equal(got[i], nb_model.lineage_walk(seed, sid, T, K))


def test_calc_relat_means_matches_model_and_reference(golden):
    from conftest import tree_spec
    from prosstt_amd import sim_utils as sut
    from prosstt_amd.tree import Tree
    g = golden("g3_lineage_unequal_gamma")
    spec = tree_spec(g)
    t = Tree(topology=spec["topology"], time=spec["time"], num_branches=len(spec["time"]),
             branch_points=spec["branch_points"], modules=spec["modules"], G=spec["G"])
    H = g["H"]
    K = H.shape[0]
    progs = {b: g["prog_%s" % b] for b in t.branches}
    rel = sut.calc_relat_means(t, progs, H)
    gamma_k = K * U / (1 - K * U)
    for b in t.branches:
        want, _ = nb_model.lineage_commit(progs[b], H)
        np.testing.assert_array_equal(rel[b], want)
        # the reference's numpy product and the kernel are each within gamma(K) * |P| @ |H| of the exact value
        mag = np.abs(progs[b]) @ np.abs(H)
        assert np.all(np.abs(rel[b] - g["rel_%s" % b]) <= 2 * gamma_k * mag * (1 + 4 * U))


def test_max_relat_exp(ctx):
    from prosstt_amd import simulation as sim, sim_utils as sut
    from prosstt_amd.tree import Tree
    np.random.seed(21)
    t = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 30, "B": 17, "C": 45}, num_branches=3,
             branch_points=1, modules=7, G=203)
    rel, _, _ = sim.simulate_lineage(t, a=0.05, intra_branch_tol=0)
    want = np.stack([np.max(np.exp(np.asarray(rel[b])), axis=0) for b in t.branches], axis=1)
    got = sut.max_relat_exp(t, rel)                          # the device tensor simulate_lineage kept
    assert got.shape == (203, 3)
    np.testing.assert_array_equal(got, want)
    fresh = {b: np.array(rel[b], copy=True) for b in t.branches}
    np.testing.assert_array_equal(sut.max_relat_exp(t, fresh), want)   # from the host arrays


def test_wrappers_take_strided_coefficients(ctx):
    """A column slice or a transposed H gives what its contiguous copy gives (the kernels index H + k*G + g)."""
    import torch
    rng = np.random.default_rng(4)
    T, K, G = 40, 6, 300
    P = np.stack([walk(rng, T, K) for _ in range(2)])
    sibs = [walk(rng, 25, K)]
    wide = coefficients(rng, K, G + 50)
    H = np.ascontiguousarray(wide[:, 20:20 + G])
    sliced = dev(ctx, wide)[:, 20:20 + G]
    transposed = dev(ctx, H.T).t()
    assert not sliced.is_contiguous() and not transposed.is_contiguous()
    want_top, want_counts = nb_model.lineage_attempt(P, H, sibs)
    want_rel, want_max = nb_model.lineage_commit(P[0], H)
    for Hd in (sliced, transposed):
        top, counts = ctx.lineage_attempt_batch(P, Hd, sibs)
        np.testing.assert_array_equal(top, want_top)
        np.testing.assert_array_equal(counts, want_counts)
        rel = torch.empty((T, G), dtype=torch.float64, device=ctx.torch_device)
        gmax = torch.full((G,), -np.inf, dtype=torch.float64, device=ctx.torch_device)
        ctx.lineage_commit(P[0], Hd, rel, gmax)
        np.testing.assert_array_equal(rel.cpu().numpy(), want_rel)
        np.testing.assert_array_equal(gmax.cpu().numpy(), want_max)


def test_wrappers_refuse_bad_outputs(ctx):
    """Outputs the kernels would write past or misread are refused on the host, before any launch."""
    import torch
    rng = np.random.default_rng(6)
    T, K, G = 10, 4, 100
    P, Hd = walk(rng, T, K), dev(ctx, coefficients(rng, K, G))
    gmax32 = torch.full((G,), -1.0, dtype=torch.float32, device=ctx.torch_device)
    with pytest.raises((TypeError, ValueError)):
        ctx.lineage_commit(P, Hd, None, gmax32)
    assert bool((gmax32 == -1.0).all())
    rel_cpu = torch.full((T, G), 5.0, dtype=torch.float64)
    with pytest.raises((TypeError, ValueError)):
        ctx.lineage_commit(P, Hd, rel_cpu, None)
    assert bool((rel_cpu == 5.0).all())
    rel = dev(ctx, rng.normal(size=(T, G)))
    with pytest.raises((TypeError, ValueError)):
        ctx.gene_max(rel, gmax32)
    assert bool((gmax32 == -1.0).all())
    short = torch.full((T - 1, G), 3.0, dtype=torch.float32, device=ctx.torch_device)
    with pytest.raises((TypeError, ValueError)):
        ctx.means_from_rel(rel, dev(ctx, np.ones(G)), out=short)
    assert bool((short == 3.0).all())
    strided = torch.full((T, 2 * G), 3.0, dtype=torch.float32, device=ctx.torch_device)[:, ::2]
    with pytest.raises((TypeError, ValueError)):
        ctx.means_from_rel(rel, dev(ctx, np.ones(G)), out=strided)
    torch.cuda.synchronize()
