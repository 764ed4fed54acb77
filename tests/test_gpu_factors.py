"""-m gpu: prosstt_amd/factors.py and libprosstt_amd_factors.so against the numpy model (tests/factors_model.py).

Bit for bit.  With coef = 0, s = 1, alpha = 0, beta = 1, loadings in {0, +-1, +-2} and counts below 64 every product and sum
of U and I is an integer below 2^53 (mu = d = w = 1, u = x - 1), so the device must return the model's bits whatever the order
of the sums; Q (logarithms) is left out there.

Tolerance of the real-valued sums.  |device - model| <= c 2^-53 S per output, S the model's sum of the magnitudes of the
parts of the terms (tests/factors_model.py).  c = C_TERM + 2 (genes per block + blocks of genes): DESIGN section 31 derives
C_TERM = 48 from the roundings of the definition and the documented 1 ulp of HIP's and of numpy's exp, log1p and log, and the
definition here is that one with the roles swapped; each of the two sides adds its terms one after the other, one rounding per
addition.  The largest ratio measured on an MI355X is in DESIGN section 35; c is not fitted to it.

Tolerance of a half's coefficients.  The device's half and the model's take the same penalised step from a common state on
sums that differ by at most dU = c 2^-53 S_U and dI = c 2^-53 S_I: the new coefficients differ by cov dU + cov dI step,
cov = (I + penalty)^-1.  The common state is the model's after four rounds, where a step is small beside 1, so the second part
is below the first; regress's radius COEF_FACTOR lambda_max(cov) c 2^-53 |S_U| with COEF_FACTOR = 4 covers both (DESIGN
section 31 has it for a whole fit, a geometric sum of such steps), norms Euclidean over a unit's coefficients.  It holds for
the genes and cells that took the same number of halvings in both; the others stood on the threshold of the halving rule, and
must be few (at most 1 in 100)."""
import ctypes
import functools

import numpy as np
import pytest

import factors_model as M

pytestmark = pytest.mark.gpu

C_TERM = 48.0
U53 = 2.0 ** -53
COEF_FACTOR = 4.0
T = 32                                      # PROSSTT_AMD_FACTORS_TILE_GENES (tests/test_factors_host.py reads it from the header)

NS = [1, 63, 255, 256, 257, 513, 700]
GS = [1, T - 1, T, T + 1, 2 * T + 1, 257, 513]
PS = [1, 3, 4, 5, 8, 9, 16]                # 2 | 9, 14 | 20 | 44, 54 | 152 sums: both sides of the splits 8, 16 and 32
LAYOUTS = ["plain", "wide", "shifted", "padded"]      # row stride G, G + 1, G + 3 from one element in, G rounded up to 4 and 4 more
SPLITS = [0, 8, 16, 32]
BLOCKINGS = [0, T, 4 * T]
# (N, G, p, layout, split, genes_per_block, use): a sweep that meets every value of every list
CASES = [(NS[i % 7], GS[(3 * i + i // 7) % 7], PS[(5 * i + 2 * (i // 7)) % 7], LAYOUTS[(i + i // 4) % 4], SPLITS[(i + i // 5) % 4],
          BLOCKINGS[(i + i // 3) % 3], bool((i // 2) % 2)) for i in range(35)]
# whole tiles under the 16-byte loads with several blocks of genes, the mixed slices, and the largest of everything
CASES += [(700, 513, 16, "padded", 0, 0, True), (257, 2 * T + 1, 9, "padded", 8, T, False), (513, 257, 5, "padded", 32, 4 * T, True),
          (256, 2 * T + 1, 8, "wide", 16, T, True), (513, 513, 3, "padded", 8, 4 * T, False)]


def test_the_cases_cover_every_listed_value():
    for column, values in enumerate((NS, GS, PS, LAYOUTS, SPLITS, BLOCKINGS, [False, True])):
        assert {case[column] for case in CASES} == set(values), column
    from prosstt_amd import factors
    assert factors.gene_blocks(257, 513)[1] > 1 and factors.gene_blocks(700, 513, T)[1] == 17


def _view(W, G, layout):
    """The device view of the host matrix W (N, G) in a layout."""
    import torch
    N = W.shape[0]
    if layout == "plain":
        return torch.as_tensor(W).cuda()
    ld, shift = {"wide": (G + 1, 0), "shifted": (G + 3, 1), "padded": (-(-G // 4) * 4 + 4, 0)}[layout]
    wide = torch.full((N, ld), 12345, dtype=torch.int32, device="cuda")
    wide[:, shift:shift + G] = torch.as_tensor(W).cuda()
    return wide[:, shift:shift + G]


def _exact_inputs(N, G, p, use, rng):
    X = rng.integers(0, 64, size=(N, G)).astype(np.int32)
    L = rng.integers(-2, 3, size=(G, p)).astype(np.float64)
    left_out = None
    if use:
        left_out = np.where(rng.random(G) < 0.2, -1, rng.integers(0, 5, size=G))
        if G > 1:
            left_out[0] = -1
    return X, L, left_out


@pytest.mark.parametrize("N,G,p,layout,split,per,use", CASES)
def test_exact_sums_bit_for_bit(N, G, p, layout, split, per, use):
    from prosstt_amd import factors
    rng = np.random.default_rng(N * 100003 + G * 7 + 31 * p + len(layout))
    X, L, left_out = _exact_inputs(N, G, p, use, rng)
    zero = np.zeros((N, p))
    got = factors.cell_equations(_view(X, G, layout), np.ones(N), L, zero, 0.0, 1.0, use=left_out, split=split, genes_per_block=per)
    want = M.cell_equations(X, np.ones(N), L, zero, 0.0, 1.0, left_out, per).eq
    assert got.score.shape == (N, p) and got.information.shape == (N, p * (p + 1) // 2) and got.n_genes == G
    assert got.score.tobytes() == want.score.tobytes()
    assert got.information.tobytes() == want.information.tobytes()
    assert np.array_equal(got.used, want.used) and np.all(np.isfinite(got.q))
    assert np.all(got.used == (G if left_out is None else int((left_out >= 0).sum())))


# ----------------------------------------------------------------------------------------------- real-valued inputs

@functools.lru_cache(maxsize=None)
def _real():
    """257 cells x 513 genes of negative-binomial counts by numpy from a rank-6 log-bilinear model, per-gene alpha and beta
    (some 0 and some 1), loadings with a column of intercepts (p = 7), the true coefficients and perturbed ones."""
    rng = np.random.default_rng(2025)
    N, G, k = 257, 513, 6
    L = np.concatenate([rng.normal(0.5, 0.8, size=(G, 1)), rng.normal(0.0, 0.4, size=(G, k))], axis=1)
    C = np.concatenate([np.ones((N, 1)), rng.normal(0.0, 0.7, size=(N, k))], axis=1)
    alpha, beta = rng.uniform(0.05, 0.6, size=G), rng.uniform(1.0, 3.0, size=G)
    alpha[::7], beta[::5] = 0.0, 1.0
    sc = rng.lognormal(0.0, 0.4, size=N)
    X = _draw(rng, sc[:, None] * np.exp(C @ L.T), alpha, beta)
    perturbed = C + rng.normal(0.0, 0.3, size=C.shape)
    return X, sc, L, alpha, beta, C, perturbed


def _draw(rng, mu, alpha, beta):
    var = alpha * mu * mu + beta * mu
    with np.errstate(divide="ignore", invalid="ignore"):
        size_nb, prob = mu * mu / (var - mu), mu / var
    poisson = ~(var > mu)
    X = np.where(poisson, rng.poisson(mu), rng.negative_binomial(np.where(poisson, 1.0, size_nb), np.where(poisson, 0.5, prob)))
    return X.astype(np.int32)


def _c(N, G, per=0):
    from prosstt_amd import factors
    genes, blocks = factors.gene_blocks(N, G, per)
    return C_TERM + 2.0 * (genes + blocks)


def _ratios(got, want):
    """The largest |device - model| / S over the outputs of U, of I and of Q."""
    out = []
    for dev, model, S in ((got.score, want.eq.score, want.s_score), (got.information, want.eq.information, want.s_information),
                          (got.q, want.eq.q, want.s_q)):
        assert np.all(np.isfinite(dev))
        diff = np.abs(dev - model)
        assert np.all(diff[S == 0] == 0)
        out.append(float((diff[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0)
    assert np.array_equal(got.used, want.eq.used)
    return out


@pytest.mark.parametrize("which", ["true", "perturbed"])
@pytest.mark.parametrize("layout,per", [("plain", 0), ("shifted", 0), ("padded", 4 * T), ("plain", 544)])
def test_real_valued_sums_against_the_model(which, layout, per):
    from prosstt_amd import factors
    X, sc, L, alpha, beta, C, perturbed = _real()
    coef = C if which == "true" else perturbed
    got = factors.cell_equations(_view(X, X.shape[1], layout), sc, L, coef, alpha, beta, genes_per_block=per)
    want = M.cell_equations(X, sc, L, coef, alpha, beta, None, per)
    assert want.status == 0
    r = _ratios(got, want)
    bound = _c(*X.shape, per) * U53
    print("factors ratio %s %s genes_per_block=%d: U %.3g I %.3g Q %.3g of 2^-53 (bound %.3g)" % (which, layout, per, r[0] / U53,
                                                                                              r[1] / U53, r[2] / U53, bound / U53))
    assert max(r) <= bound


def _bytes(a):
    return np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.cpu().numpy()).tobytes()


def _same(a, b):
    return (_bytes(a.score) == _bytes(b.score) and _bytes(a.information) == _bytes(b.information) and _bytes(a.q) == _bytes(b.q)
            and np.array_equal(a.used, b.used))


def test_equal_bits_for_every_split_and_stream_and_for_a_cell_alone_or_among_others():
    import torch
    from prosstt_amd import factors
    X, sc, L, alpha, beta, coef, _ = _real()
    view = torch.as_tensor(X).cuda()
    first = factors.cell_equations(view, sc, L, coef, alpha, beta)
    assert _same(first, factors.cell_equations(view, sc, L, coef, alpha, beta))
    with torch.cuda.stream(torch.cuda.Stream()):
        assert _same(first, factors.cell_equations(view, sc, L, coef, alpha, beta))
    for split in (8, 16, 32):
        assert _same(first, factors.cell_equations(view, sc, L, coef, alpha, beta, split=split)), split
    # the unaligned kernel, and a wider row stride
    for layout in ("shifted", "wide", "padded"):
        assert _same(first, factors.cell_equations(_view(X, 513, layout), sc, L, coef, alpha, beta)), layout
    # a cell alone against the same cell among 256 others, and chunks of cells, at equal genes_per_block
    per = factors.gene_blocks(257, 513)[0]
    assert per == factors.gene_blocking(257, 513) and factors.gene_blocks(257, 513)[1] > 1
    assert factors.gene_blocks(1, 513) == factors.gene_blocks(257, 513)       # (one block of cells either way)
    for per in (per, 4 * T):
        whole = factors.cell_equations(view, sc, L, coef, alpha, beta, genes_per_block=per)
        for cell in (0, 100, 256):
            alone = factors.cell_equations(view[cell:cell + 1], sc[cell:cell + 1], L, coef[cell:cell + 1], alpha, beta, genes_per_block=per)
            assert _bytes(alone.score) == _bytes(whole.score[cell:cell + 1]) and _bytes(alone.q) == _bytes(whole.q[cell:cell + 1])
            assert _bytes(alone.information) == _bytes(whole.information[cell:cell + 1])
        parts = [factors.cell_equations(view[lo:hi], sc[lo:hi], L, coef[lo:hi], alpha, beta, genes_per_block=per)
                 for lo, hi in ((0, 100), (100, 257))]
        assert _same(factors.CellEquations.concat(parts), whole)
    # device-resident inputs and device outputs
    on = lambda a: torch.as_tensor(a).cuda()                     # noqa: E731
    dev = factors.cell_equations(view, on(sc), on(L), on(coef), on(alpha), on(beta), out="torch")
    assert isinstance(dev.score, torch.Tensor) and dev.score.is_cuda and dev.information.is_cuda and dev.q.is_cuda
    assert tuple(dev.information.shape) == (257, 28) and dev.score.dtype == torch.float64 and tuple(dev.symmetric().shape) == (257, 7, 7)
    assert _same(dev, first)
    both = factors.CellEquations.concat([dev, dev])
    assert isinstance(both.score, torch.Tensor) and both.n_cells == 514


def test_presented_counts_are_read_in_place():
    """Row i of a ``device.PresentedCounts`` is cell ``cell_of_row[i]``: the size factors and coefficients are given in plan
    order and permuted to the rows, the results come back in plan order.  Rows are independent: the same bits."""
    import torch
    from prosstt_amd import device, factors
    X, sc, L, alpha, beta, coef, _ = _real()
    perm = np.random.default_rng(41).permutation(257)
    presented = device.PresentedCounts(torch.as_tensor(np.ascontiguousarray(X[perm])).cuda(), perm)
    got = factors.cell_equations(presented, sc, L, coef, alpha, beta)
    assert _same(got, factors.cell_equations(torch.as_tensor(X).cuda(), sc, L, coef, alpha, beta))
    dev = factors.cell_equations(presented, sc, L, coef, alpha, beta, out="torch")
    assert _same(dev, got)


# ------------------------------------------------------------------------------------------------------- status bits

def _raises_bit(name, X=((3,),), sc=(1.5,), L=((0.4,),), coef=((0.7,),), alpha=0.2, beta=2.0, use=None):
    """The smallest problem, N = G = 1 unless the arguments say otherwise: this bit and no other, for every split."""
    import torch
    from prosstt_amd import factors
    X = torch.as_tensor(np.asarray(X, dtype=np.int32)).cuda()
    args = (np.asarray(sc, dtype=np.float64), np.asarray(L, dtype=np.float64), np.asarray(coef, dtype=np.float64), alpha, beta)
    for split in (0, 8, 16, 32):
        with pytest.raises(ValueError) as err:
            factors.cell_equations(X, *args, use=use, split=split)
        assert str(err.value).startswith("status bit %s " % name) and "; " not in str(err.value), split
    assert getattr(factors, name) & M.cell_equations(X.cpu().numpy(), args[0], args[1], args[2], alpha, beta, use).status
    clean = factors.cell_equations(torch.tensor([[3]], dtype=torch.int32).cuda(), [1.5], [[0.4]], [[0.7]], 0.2, 2.0)
    assert np.isfinite(clean.q).all()                            # nothing is left behind: the next call is clean


def test_status_bit_of_a_negative_count():
    _raises_bit("NEGATIVE", X=[[-1]])
    _raises_bit("NEGATIVE", X=[[3, 4], [5, -7]], sc=[1.0, 2.0], L=[[0.4], [0.1]], coef=[[0.7], [0.2]])


def test_a_negative_count_of_a_gene_that_is_left_out_or_of_a_cell_that_is_skipped_sets_nothing():
    import torch
    from prosstt_amd import factors
    X = torch.tensor([[3, -4], [5, 7]], dtype=torch.int32).cuda()
    got = factors.cell_equations(X, [1.0, 2.0], [[0.4], [np.nan]], [[0.7], [0.2]], 0.2, [2.0, 0.5], use=[0, -1])
    assert got.used.tolist() == [1, 1]


def test_status_bit_of_a_bad_size_factor():
    for bad in (0.0, -1.0, 1e151, np.inf, np.nan):
        _raises_bit("SIZE", sc=[bad])


def test_status_bit_of_inadmissible_parameters():
    _raises_bit("PARAMETER", beta=0.5)
    _raises_bit("PARAMETER", alpha=-1e-18)
    _raises_bit("PARAMETER", alpha=np.inf)
    _raises_bit("PARAMETER", beta=np.nan)


def test_status_bit_of_a_coefficient_or_a_loading_that_is_not_finite():
    _raises_bit("COEFFICIENT", coef=[[np.nan]])
    _raises_bit("COEFFICIENT", L=[[np.inf]])
    # the second of two loadings, which only the information's products read besides the loadings' table
    _raises_bit("COEFFICIENT", L=[[0.4, np.nan]], coef=[[0.7, 0.1]])


def test_status_bit_of_a_linear_predictor_beyond_700_or_a_mean_that_overflows():
    _raises_bit("ETA", L=[[1.0]], coef=[[701.0]])
    _raises_bit("ETA", L=[[-1.0]], coef=[[701.0]])
    _raises_bit("ETA", sc=[1e150], L=[[1.0]], coef=[[690.0]], alpha=0.0, beta=1.0)


def test_one_past_sixteen_coefficients_is_refused_through_the_abi():
    import torch
    from prosstt_amd import _native
    lib = _native.load("factors")
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")      # noqa: E731
    X = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    need = ctypes.c_uint64(0)
    assert lib.prosstt_amd_factors_workspace_bytes(2, 3, 16, 0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.prosstt_amd_factors_workspace_bytes(2, 3, 17, 0, ctypes.byref(need)) == _native.EINVAL
    ws = torch.zeros(int(need.value), dtype=torch.uint8, device="cuda")
    size, L, coef, par, sums = t(2) + 1.0, t(3, 17), t(17, 2), t(2, 3) + 1.0, t(17 + 153 + 1, 2)
    used, status = torch.full((2,), 77, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda a: ctypes.c_void_p(a.data_ptr())                # noqa: E731

    def call(p):
        return lib.prosstt_amd_factors_cell_equations(None, ptr(X), 2, 3, 3, ptr(size), None, ptr(L), 17, p, ptr(coef), ptr(par[0]),
                                                      ptr(par[1]), 0, 0, ptr(ws), ws.numel(), ptr(sums), ptr(sums[17:]), ptr(sums[170]),
                                                      ptr(used), ptr(status))
    assert call(17) == _native.EINVAL
    assert b"1 <= p <= 16" in lib.prosstt_amd_factors_last_error()
    torch.cuda.synchronize()
    assert used.tolist() == [77, 77] and int(status.item()) == 0              # nothing was enqueued
    assert call(16) == 0
    torch.cuda.synchronize()
    assert used.tolist() == [3, 3] and int(status.item()) == 0


# ---------------------------------------------------------------------------------------------- the halves and the loop

PENALTY, TOL, K = 1.0, 1e-8, 3


@functools.lru_cache(maxsize=None)
def _bilinear():
    """300 cells x 257 genes from a rank-3 log-bilinear model, alpha = 0.2, beta = 2; the random start of the scores; the
    model's loop in both summation orders, 8 rounds each and 4 rounds for the common state of the half-round test."""
    rng = np.random.default_rng(7)
    N, G = 300, 257
    U, V, b = rng.normal(0.0, 1.0, size=(N, K)), rng.normal(0.0, 0.4, size=(G, K)), rng.normal(1.5, 0.6, size=G)
    sc = rng.lognormal(0.0, 0.3, size=N)
    X = _draw(rng, sc[:, None] * np.exp(b[None, :] + U @ V.T), np.full(G, 0.2), np.full(G, 2.0))
    X[:, 11] = 0                                                  # a gene without counts
    start = 0.1 * rng.standard_normal((N, K))
    histories = [], []
    fits = [M.glmpca(X, sc, start, 0.2, 2.0, ordered=o, rotated=False, history=h, penalty=PENALTY, tol=TOL, max_rounds=8)
            for o, h in zip((True, False), histories)]
    state = M.glmpca(X, sc, start, 0.2, 2.0, rotated=False, penalty=PENALTY, tol=TOL, max_rounds=4)
    return X, sc, start, fits, histories, state, b[None, :] + U @ V.T


def test_the_models_two_summation_orders_agree_on_this_input():
    """What the two tests below rest on, checked on the CPU: every halving of the two model loops is the same, and their
    objectives stay within the stopping rule's resolution of each other."""
    X, sc, start, fits, histories, state, _ = _bilinear()
    ordered, plain = fits
    assert len(ordered.objective) == len(plain.objective) == 8
    assert np.all(np.abs(ordered.objective - plain.objective) <= TOL * (np.abs(ordered.objective) + 1.0))
    for a, b in zip(*histories):
        assert np.array_equal(a.gene_halvings, b.gene_halvings) and np.array_equal(a.cell_halvings, b.cell_halvings)
    assert ordered.no_counts[11] and ordered.no_counts.sum() == 1


def _device_evaluators(X, sc, no_counts):
    import torch
    from prosstt_amd import factors, regress
    view = torch.as_tensor(X).cuda()
    N = X.shape[0]
    use = np.where(no_counts, -1, 0)
    genes = regress._Pass(view, sc, np.arange(N), np.ones((N, K + 1)), "test")

    def gene_evaluate(scores, coef):
        genes.set_design(np.concatenate([np.ones((N, 1)), scores], axis=1))
        return genes(coef, 0.2, 2.0)

    def cell_evaluate(L, coef):
        return factors.cell_equations(view, sc, L, coef, 0.2, 2.0, use=use)

    return gene_evaluate, cell_evaluate


def test_one_half_round_from_a_common_state():
    from prosstt_amd import factors, regress
    import regress_model
    X, sc, start, fits, histories, state, _ = _bilinear()
    N, G = X.shape
    no_counts = state.no_counts
    dev = _device_evaluators(X, sc, no_counts)
    mod = M.evaluators(X, sc, 0.2, 2.0, no_counts)
    common = (state.scores, state.loadings, state.intercept, no_counts, PENALTY, TOL)
    got_b, got_l, got_h, _q = factors.half_round(*dev, *common, "genes")
    want_b, want_l, want_h, _q = factors.half_round(*mod, *common, "genes")
    design = np.concatenate([np.ones((N, 1)), state.scores], axis=1)
    coef = np.concatenate([state.intercept[:, None], state.loadings], axis=1)
    at = regress_model.normal_equations(X, sc, np.arange(N), design, coef, 0.2, 2.0)
    rows, blocks = regress.row_blocks(N, G)
    figures = _within_the_radius(np.concatenate([got_b[:, None], got_l], axis=1), np.concatenate([want_b[:, None], want_l], axis=1),
                                 got_h, want_h, at.ne.information + np.diag([0.0] + [PENALTY] * K), at.s_score,
                                 C_TERM + 2.0 * (rows + blocks), ~no_counts)
    print("gene half: %d genes, %d with equal halvings; |coef - model| at most %.3g, %.3g of the radius" % figures)
    assert np.array_equal(got_l[no_counts], want_l[no_counts]) and np.array_equal(got_b[no_counts], want_b[no_counts])
    got_s, got_h, _q = factors.half_round(*dev, *common, "cells")
    want_s, want_h, _q = factors.half_round(*mod, *common, "cells")
    L = np.concatenate([state.intercept[:, None], state.loadings], axis=1)
    at = M.cell_equations(X, sc, L, np.concatenate([np.ones((N, 1)), state.scores], axis=1), 0.2, 2.0, np.where(no_counts, -1, 0))
    figures = _within_the_radius(got_s, want_s, got_h, want_h, at.eq.symmetric()[:, 1:, 1:] + PENALTY * np.eye(K), at.s_score[:, 1:],
                                 _c(N, G), np.ones(N, dtype=bool))
    print("cell half: %d cells, %d with equal halvings; |coef - model| at most %.3g, %.3g of the radius" % figures)


def _within_the_radius(got, want, got_h, want_h, matrix, s_score, c, keep):
    """The module docstring's tolerance of a half's coefficients, unit by unit; returns the figures for the test's print."""
    lam = 1.0 / np.linalg.eigvalsh(matrix[keep])[:, 0]                       # lambda_max of the inverse
    allowed = COEF_FACTOR * lam * c * U53 * np.linalg.norm(s_score[keep], axis=1)
    diff = np.linalg.norm(got[keep] - want[keep], axis=1)
    same = got_h[keep] == want_h[keep]
    assert (~same).sum() <= keep.sum() // 100, (int((~same).sum()), int(keep.sum()))
    assert np.all(diff[same] <= allowed[same]), float((diff[same] / allowed[same]).max())
    return int(keep.sum()), int(same.sum()), float(diff.max()), float((diff[same] / allowed[same]).max())


@functools.lru_cache(maxsize=None)
def _device_fit():
    import torch
    from prosstt_amd import factors
    X, sc, start, fits, histories, state, _ = _bilinear()
    return factors.glmpca(torch.as_tensor(X).cuda(), sc, K, alpha=0.2, beta=2.0, penalty=PENALTY, init=start, max_rounds=8, tol=TOL)


def test_the_loop_follows_the_models_objective():
    X, sc, start, fits, histories, state, truth = _bilinear()
    f = _device_fit()
    want = fits[0]
    assert f.rounds == 8 == len(f.objective) and not f.converged and f.no_counts.tolist() == want.no_counts.tolist()
    falls = f.objective[:-1] - f.objective[1:]
    assert np.all(falls <= TOL * (np.abs(f.objective[:-1]) + 1.0)), falls.max()
    gap = np.abs(f.objective - want.objective)
    print("glmpca objective: %s; largest |device - model| %.3g of tol (|Q| + 1); rms of the linear predictor against the truth %.4f"
          % (np.array2string(f.objective, precision=3), float((gap / (TOL * (np.abs(want.objective) + 1.0))).max()),
             float(np.sqrt(np.mean((f.linear_predictor() - truth)[:, ~f.no_counts] ** 2)))))
    assert np.all(gap <= TOL * (np.abs(want.objective) + 1.0))


def test_the_rotation_invariants():
    from prosstt_amd import factors
    X, sc, start, fits, histories, state, _ = _bilinear()
    f = _device_fit()
    assert f.scores.shape == (300, K) and f.loadings.shape == (257, K) and f.intercept.shape == (257,)
    np.testing.assert_allclose(f.loadings.T @ f.loadings, np.eye(K), rtol=0, atol=1e-12)
    gram = f.scores.T @ f.scores
    norms = np.sqrt(np.diag(gram))
    assert np.all(np.abs(gram - np.diag(np.diag(gram))) <= 1e-12 * norms[:, None] * norms[None, :]) and np.all(np.diff(norms) <= 0)
    assert np.all(np.abs(f.scores.mean(axis=0)) <= 1e-12 * norms)
    top = np.argmax(np.abs(f.loadings), axis=0)
    assert np.all(f.loadings[top, np.arange(K)] > 0)
    assert np.all(f.loadings[f.no_counts] == 0) and np.allclose(f.intercept[f.no_counts], np.log(0.5 / sc.sum()), rtol=1e-12)
    # the rotation changes no linear predictor: rotate the model's state by the same function and compare with its own
    # (``rotate`` is host code that both loops share; the device fit's own predictor is covered by the round trip through
    # ``raw()`` in the project test below, which must return it to 1e-12)
    want = fits[0]
    rotated = factors.rotate(want.scores, want.loadings, want.intercept)
    before = want.intercept[None, :] + want.scores @ want.loadings.T
    after = rotated[2][None, :] + rotated[0] @ rotated[1].T
    assert np.abs(after - before).max() <= 1e-12
    assert f.fitted() is f.fitted() and np.allclose(np.log(f.fitted()), f.linear_predictor(), rtol=0, atol=1e-12)


def test_project_of_the_training_cells_is_one_more_cell_half():
    import torch
    from prosstt_amd import factors
    X, sc, start, fits, histories, state, _ = _bilinear()
    f = _device_fit()
    N, G = X.shape
    history = []
    got = f.project(torch.as_tensor(X).cuda(), sc, start=f.scores, max_rounds=1, history=history)
    assert len(history) == 1 and got.tobytes() == f.rotated_scores(history[0].after).tobytes()
    # the half is taken in the loop's own coordinates, the penalty's: the model takes it from the very state the device took
    # it from (``before``: the fit's scores through ``raw_scores``), and the two are compared there, halvings and all
    _, loadings, intercept = f.raw()
    scores = history[0].before
    assert np.abs(scores - f.raw()[0]).max() == 0
    assert np.abs(intercept[None, :] + scores @ loadings.T - f.linear_predictor()).max() <= 1e-12
    mod = M.evaluators(X, sc, 0.2, 2.0, f.no_counts)
    want, want_h, _q = factors.half_round(*mod, scores, loadings, intercept, f.no_counts, PENALTY, TOL, "cells")
    L = np.concatenate([intercept[:, None], loadings], axis=1)
    at = M.cell_equations(X, sc, L, np.concatenate([np.ones((N, 1)), scores], axis=1), 0.2, 2.0, np.where(f.no_counts, -1, 0))
    figures = _within_the_radius(history[0].after, want, history[0].halvings, want_h, at.eq.symmetric()[:, 1:, 1:] + PENALTY * np.eye(K),
                                 at.s_score[:, 1:], _c(N, G), np.ones(N, dtype=bool))
    print("project: %d cells, %d with equal halvings; |scores - model| at most %.3g, %.3g of the radius" % figures)
    # chunks of cells, and from zero to the cells' own maxima: a concave problem per cell
    halves = [f.project(torch.as_tensor(X[lo:hi]).cuda(), sc[lo:hi]) for lo, hi in ((0, 120), (120, 300))]
    whole = f.project(torch.as_tensor(X).cuda(), sc)
    assert np.allclose(np.concatenate(halves), whole, rtol=0, atol=1e-9)
    # (where the loop stopped, a cell's penalised Q is no lower than after the one half from the fit, up to the halving rule's
    # own allowance; the model evaluates both)
    def penalised(rotated):
        raw = f.raw_scores(rotated)
        q = M.cell_equations(X, sc, L, np.concatenate([np.ones((N, 1)), raw], axis=1), 0.2, 2.0, np.where(f.no_counts, -1, 0)).eq.q
        return q - 0.5 * PENALTY * np.sum(raw ** 2, axis=1)
    at_whole, at_got = penalised(whole), penalised(got)
    assert np.all(at_whole >= at_got - TOL * (np.abs(at_got) + 1.0))
