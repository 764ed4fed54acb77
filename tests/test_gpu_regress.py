"""-m gpu: prosstt_amd/regress.py and libprosstt_amd_regress.so against the numpy model (tests/regress_model.py).

Bit for bit.  With coef = 0, s = 1, alpha = 0, beta = 1, design entries in {0, +-1, +-2} and counts below 64 every product and
sum of U, I and M is an integer below 2^53 (mu = d = w = 1, u = x - 1), so the device must return the model's bits whatever
the order of the sums; Q (logarithms) is left out there.

Tolerance of the real-valued sums.  |device - model| <= c 2^-53 S per output, S the model's sum of the magnitudes of the
parts of the terms (tests/regress_model.py).  c = C_TERM + 2 (rows per block + blocks of rows): DESIGN section 31 derives
C_TERM = 48 from the roundings of the definition and the documented 1 ulp of HIP's and of numpy's exp, log1p and log; each of
the two sides adds its terms one after the other, one rounding per addition.  The largest ratio measured on an MI355X is in
DESIGN section 31; c is not fitted to it.

Tolerance of the coefficients.  The device's loop and the model's run the same scoring on sums that differ by at most
dU = c 2^-53 S_U and dI = c 2^-53 S_I.  One round maps the coefficients to coef + I^-1 U; near the maximum that map moves
an error e of the coefficients to (1 - I^-1 J) e, J the observed information, plus what the round's own sums add,
cov dU + cov dI cov U.  At the last round U is a step's worth of nothing, so the second part is below the first, and the
errors of the earlier rounds are contracted (1 - I^-1 J is the relative gap between the observed and the expected
information, well below 1/2 at 50 cells and more per knot): a geometric sum below 2.  Hence for a gene that took the same
number of rounds in both loops |coef - model| <= COEF_FACTOR lambda_max(cov) c 2^-53 |S_U|, COEF_FACTOR = 4 (2 for the
geometric sum, 2 for the part of dI), norms Euclidean over the p coefficients.  A gene whose round counts differ stopped on
another side of the stopping rule's threshold; both loops are then within sqrt(2 tol (|Q| + 1) lambda_max(cov)) of the
maximiser, and such genes must be few (at most 1 in 100)."""
import functools

import numpy as np
import pytest

import regress_model as M

pytestmark = pytest.mark.gpu

C_TERM = 48.0
U53 = 2.0 ** -53
COEF_FACTOR = 4.0

NS = [1, 7, 8, 9, 63, 65, 133, 700]
GS = [1, 255, 256, 257, 513]
PS = [1, 2, 3, 4, 5, 6, 7, 8, 16]          # 5 | 9, 14 | 20, 27 | 35 sums: both sides of the splits 8, 16 and 32
KS = ["1", "60", "N"]
LAYOUTS = ["plain", "wide", "shifted", "padded"]      # row stride G, G + 1, G + 3 from one element in, G rounded up to 4
SPLITS = [0, 8, 16, 32]
# (N, G, p, K, layout, meat, split): a sweep that meets every value of every list
CASES = [(NS[i % 8], GS[(i + i // 8) % 5], PS[(2 * i + i // 9) % 9], KS[(i + i // 3) % 3], LAYOUTS[(i + i // 4) % 4], bool((i // 2) % 2),
          SPLITS[(i + i // 5) % 4]) for i in range(36)]
# the staged loads with whole strips, and the largest of everything
CASES += [(700, 513, 16, "60", "padded", False, 0), (133, 256, 7, "N", "plain", True, 8), (65, 513, 5, "60", "padded", True, 32),
          (700, 257, 8, "N", "wide", False, 16)]


def test_the_cases_cover_every_listed_value():
    for column, values in enumerate((NS, GS, PS, KS, LAYOUTS, [False, True], SPLITS)):
        assert {case[column] for case in CASES} == set(values), column
    from prosstt_amd import regress
    assert regress.row_blocks(700, 256)[1] > 1 and regress.row_blocks(133, 513)[1] > 1


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


def _exact_inputs(N, G, p, K, rng):
    K = {"1": 1, "60": 60, "N": N}[K]
    X = rng.integers(0, 64, size=(N, G)).astype(np.int32)
    D = rng.integers(-2, 3, size=(K, p)).astype(np.float64)
    labels = np.arange(N) if K == N else rng.integers(0, K, size=N)
    labels = np.where(rng.random(N) < 0.15, -1, labels)
    if N > 1:
        labels[0] = max(labels[0], 0)
    return X, D, labels


@pytest.mark.parametrize("N,G,p,K,layout,meat,split", CASES)
def test_exact_sums_bit_for_bit(N, G, p, K, layout, meat, split):
    from prosstt_amd import regress
    rng = np.random.default_rng(N * 100003 + G * 7 + 31 * p + len(layout))
    X, D, labels = _exact_inputs(N, G, p, K, rng)
    zero = np.zeros((G, p))
    got = regress.normal_equations(_view(X, G, layout), np.ones(N), labels, D, zero, 0.0, 1.0, meat=meat, split=split)
    want = M.normal_equations(X, np.ones(N), labels, D, zero, 0.0, 1.0, meat).ne
    assert got.score.shape == (G, p) and got.information.shape == (G, p, p) and got.n_cells == N
    assert got.score.tobytes() == want.score.tobytes()
    assert got.information.tobytes() == want.information.tobytes()
    assert np.array_equal(got.used, want.used) and np.all(np.isfinite(got.q))


# ----------------------------------------------------------------------------------------------- real-valued inputs

@functools.lru_cache(maxsize=None)
def _tree():
    """smoke()'s tree: 3 branches x 20 steps, 300 genes."""
    import test_gpu_fit
    return test_gpu_fit._tree()


@functools.lru_cache(maxsize=None)
def _walk():
    """Log-means walking along three branches of 20 nodes (the two children start where the parent ends), 257 genes, 300
    cells at random nodes with negative-binomial counts by numpy, per-gene alpha and beta, the tree design with one inner
    knot, and two sets of coefficients: the model's fit and a perturbed one."""
    from prosstt_amd import regress
    rng = np.random.default_rng(2024)
    G, N = 257, 300
    steps = rng.normal(0.0, 0.08, size=(3, 20, G))
    a_path = 1.0 + np.cumsum(steps[0], axis=0)
    logm = np.concatenate([a_path, a_path[-1] + np.cumsum(steps[1], axis=0), a_path[-1] + np.cumsum(steps[2], axis=0)])
    alpha, beta = rng.uniform(0.05, 0.6, size=G), rng.uniform(1.0, 3.0, size=G)
    alpha[::7], beta[::5] = 0.0, 1.0
    labels = rng.integers(0, 60, size=N)
    labels[rng.random(N) < 0.1] = -1
    sc = rng.lognormal(0.0, 0.4, size=N)
    mu = sc[:, None] * np.exp(logm[np.maximum(labels, 0)])
    var = alpha * mu * mu + beta * mu
    with np.errstate(divide="ignore", invalid="ignore"):
        size_nb, prob = mu * mu / (var - mu), mu / var
    poisson = ~(var > mu)
    X = np.where(poisson, rng.poisson(mu), rng.negative_binomial(np.where(poisson, 1.0, size_nb), np.where(poisson, 0.5, prob)))
    X = X.astype(np.int32)
    design = regress.tree_design(_tree(), 1)
    fit = M.regression(X, sc, labels, design, alpha, beta)
    assert fit.converged.all()
    perturbed = fit.coef + rng.normal(0.0, 0.3, size=fit.coef.shape)
    return X, sc, labels, design.matrix, alpha, beta, fit.coef, perturbed


def _bound(N, G):
    from prosstt_amd import regress
    rows, blocks = regress.row_blocks(N, G)
    return (C_TERM + 2.0 * (rows + blocks)) * U53


def _assert_coefficients(r, want, X, sc, labels, D, alpha, beta, tol=1e-8):
    """The module docstring's tolerance of the coefficients, gene by gene; returns the figures for the test's print."""
    assert np.array_equal(r.no_counts, want.no_counts) and np.array_equal(r.converged, want.converged)
    keep = want.converged
    at = M.normal_equations(X, sc, labels, D, np.where(np.isnan(want.coef), 0.0, want.coef), alpha, beta)
    lam = np.linalg.eigvalsh(want.cov[keep])[:, -1]
    allowed = COEF_FACTOR * lam * _bound(*X.shape) * np.linalg.norm(at.s_score[keep], axis=1)
    diff = np.linalg.norm(r.coef[keep] - want.coef[keep], axis=1)
    same = r.rounds[keep] == want.rounds[keep]
    assert (~same).sum() <= keep.sum() // 100, (int((~same).sum()), int(keep.sum()))
    assert np.all(diff[same] <= allowed[same]), float((diff[same] / allowed[same]).max())
    radius = np.sqrt(2.0 * tol * (np.abs(want.q[keep]) + 1.0) * lam)
    assert np.all(diff[~same] <= 2.0 * radius[~same])
    return int(keep.sum()), int(same.sum()), float(diff.max()), float((diff[same] / allowed[same]).max()), float(allowed.min())


def _ratios(got, want):
    """The largest |device - model| / S over the outputs of U, of I (or M) and of Q."""
    out = []
    for dev, model, S in ((got.score, want.ne.score, want.s_score), (got.information, want.ne.information, want.s_information),
                          (got.q, want.ne.q, want.s_q)):
        assert np.all(np.isfinite(dev))
        diff = np.abs(dev - model)
        assert np.all(diff[S == 0] == 0)
        out.append(float((diff[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0)
    assert np.array_equal(got.used, want.ne.used)
    return out


@pytest.mark.parametrize("which", ["fit", "perturbed"])
@pytest.mark.parametrize("meat", [False, True])
@pytest.mark.parametrize("layout", ["plain", "shifted"])
def test_real_valued_sums_against_the_model(which, meat, layout):
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, fitted, perturbed = _walk()
    coef = fitted if which == "fit" else perturbed
    got = regress.normal_equations(_view(X, X.shape[1], layout), sc, labels, D, coef, alpha, beta, meat=meat)
    want = M.normal_equations(X, sc, labels, D, coef, alpha, beta, meat)
    assert want.status == 0
    r = _ratios(got, want)
    bound = _bound(*X.shape)
    print("regress ratio %s meat=%s %s: U %.3g I %.3g Q %.3g of 2^-53 (bound %.3g)" % (which, meat, layout, r[0] / U53, r[1] / U53,
                                                                                   r[2] / U53, bound / U53))
    assert max(r) <= bound


def _same(a, b):
    return (_bytes(a.score) == _bytes(b.score) and _bytes(a.information) == _bytes(b.information) and _bytes(a.q) == _bytes(b.q)
            and np.array_equal(a.used, b.used))


def _bytes(a):
    return np.ascontiguousarray(a if isinstance(a, np.ndarray) else a.cpu().numpy()).tobytes()


def test_equal_bits_twice_on_a_second_stream_over_halves_of_the_genes_and_for_every_split():
    import torch
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, coef, _ = _walk()
    view = torch.as_tensor(X).cuda()
    for meat in (False, True):
        first = regress.normal_equations(view, sc, labels, D, coef, alpha, beta, meat=meat)
        assert _same(first, regress.normal_equations(view, sc, labels, D, coef, alpha, beta, meat=meat))
        with torch.cuda.stream(torch.cuda.Stream()):
            assert _same(first, regress.normal_equations(view, sc, labels, D, coef, alpha, beta, meat=meat))
        for split in (8, 16, 32):
            assert _same(first, regress.normal_equations(view, sc, labels, D, coef, alpha, beta, meat=meat, split=split)), split
        # the unaligned kernel
        assert _same(first, regress.normal_equations(_view(X, 257, "shifted"), sc, labels, D, coef, alpha, beta, meat=meat))
        # 257 genes are two strips and 128 / 129 genes one, all with five blocks of rows (300 cells, 64 at the least per block)
        assert regress.row_blocks(300, 257) == regress.row_blocks(300, 128) == regress.row_blocks(300, 129)
        halves = [regress.normal_equations(view[:, lo:hi], sc, labels, D, coef[lo:hi], alpha[lo:hi], beta[lo:hi], meat=meat)
                  for lo, hi in ((0, 128), (128, 257))]
        assert np.concatenate([h.score for h in halves]).tobytes() == first.score.tobytes()
        assert np.concatenate([h.information for h in halves]).tobytes() == first.information.tobytes()
        assert np.concatenate([h.q for h in halves]).tobytes() == first.q.tobytes()
    # device-resident inputs and device outputs
    on = lambda a: torch.as_tensor(a).cuda()                     # noqa: E731
    dev = regress.normal_equations(view, on(sc), on(labels), on(D), on(coef), on(alpha), on(beta), meat=True, out="torch")
    assert isinstance(dev.score, torch.Tensor) and dev.score.is_cuda and dev.information.is_cuda and dev.q.is_cuda
    assert tuple(dev.information.shape) == (257, 7, 7) and dev.score.dtype == torch.float64
    assert _same(dev, first)
    both = regress.NormalEquations.concat([dev, dev])
    assert isinstance(both.score, torch.Tensor) and both.n_cells == 600 and both.meat


def test_presented_counts_are_read_in_place():
    """Row i of a ``device.PresentedCounts`` is cell ``cell_of_row[i]``: labels and size factors are given in plan order and
    permuted to the rows, never the matrix.  The same rows as a plain matrix give the same bits; against ``in_plan_order()``
    the rows are added in another order, so the bits are equal where every sum is exact and within the bound otherwise."""
    import torch
    from prosstt_amd import device, regress
    X, sc, labels, D, alpha, beta, coef, _ = _walk()
    perm = np.random.default_rng(41).permutation(300)
    presented = device.PresentedCounts(torch.as_tensor(np.ascontiguousarray(X[perm])).cuda(), perm)
    got = regress.normal_equations(presented, sc, labels, D, coef, alpha, beta)
    rows = regress.normal_equations(presented.counts, sc[perm], labels[perm], D, coef, alpha, beta)
    assert _same(got, rows)
    assert max(_ratios(got, M.normal_equations(X, sc, labels, D, coef, alpha, beta))) <= _bound(300, 257)
    rng = np.random.default_rng(5)
    Xe, De, le = _exact_inputs(300, 257, 5, "60", rng)
    presented = device.PresentedCounts(torch.as_tensor(np.ascontiguousarray(Xe[perm])).cuda(), perm)
    zero, one = np.zeros((257, 5)), np.ones(300)
    a = regress.normal_equations(presented, one, le, De, zero, 0.0, 1.0)
    b = regress.normal_equations(presented.in_plan_order(), one, le, De, zero, 0.0, 1.0)
    assert torch.equal(presented.in_plan_order().cpu(), torch.as_tensor(Xe))
    assert a.score.tobytes() == b.score.tobytes() and a.information.tobytes() == b.information.tobytes()
    assert np.array_equal(a.used, b.used)


def test_concat_of_two_chunks_of_rows_is_the_model_of_the_chunks():
    import torch
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, coef, _ = _walk()
    view = torch.as_tensor(X).cuda()
    cuts = ((0, 100), (100, 300))
    parts = [regress.normal_equations(view[lo:hi], sc[lo:hi], labels[lo:hi], D, coef, alpha, beta) for lo, hi in cuts]
    whole = regress.NormalEquations.concat(parts)
    assert whole.n_cells == 300
    models = [M.normal_equations(X[lo:hi], sc[lo:hi], labels[lo:hi], D, coef, alpha, beta) for lo, hi in cuts]
    want = M.Sums(regress.NormalEquations.concat([m.ne for m in models]), models[0].s_score + models[1].s_score,
                  models[0].s_information + models[1].s_information, models[0].s_q + models[1].s_q, 0)
    assert max(_ratios(whole, want)) <= _bound(200, 257) + U53
    # where every sum is exact the chunks add up to the bits of the whole
    Xe, De, le = _exact_inputs(300, 257, 5, "60", np.random.default_rng(6))
    ve, zero, one = torch.as_tensor(Xe).cuda(), np.zeros((257, 5)), np.ones(300)
    parts = [regress.normal_equations(ve[lo:hi], one[lo:hi], le[lo:hi], De, zero, 0.0, 1.0) for lo, hi in cuts]
    whole = regress.NormalEquations.concat(parts)
    model = regress.NormalEquations.concat([M.normal_equations(Xe[lo:hi], one[lo:hi], le[lo:hi], De, zero, 0.0, 1.0).ne
                                            for lo, hi in cuts])
    assert whole.score.tobytes() == model.score.tobytes() and whole.information.tobytes() == model.information.tobytes()
    assert np.array_equal(whole.used, model.used)


# ------------------------------------------------------------------------------------------------------- status bits

def _raises_bit(name, **changed):
    import torch
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, coef, _ = _walk()
    args = dict(X=torch.as_tensor(X).cuda(), sc=sc, labels=labels, D=D, coef=coef, alpha=alpha, beta=beta)
    args.update(changed)
    call = lambda a: regress.normal_equations(a["X"], a["sc"], a["labels"], a["D"], a["coef"], a["alpha"], a["beta"])    # noqa: E731
    with pytest.raises(ValueError) as err:
        call(args)
    assert str(err.value).startswith("status bit %s " % name) and "; " not in str(err.value)      # this bit and no other
    clean = dict(args, X=torch.as_tensor(X).cuda(), sc=sc, labels=labels, D=D, coef=coef, alpha=alpha, beta=beta)
    call(clean)                                                  # nothing is left behind: the next call is clean


def test_status_bit_of_a_negative_count():
    import torch
    X = _walk()[0].copy()
    row = int(np.flatnonzero(_walk()[2] >= 0)[3])
    X[row, 200] = -1
    _raises_bit("NEGATIVE", X=torch.as_tensor(X).cuda())


def test_status_bit_of_a_label_beyond_the_design():
    labels = _walk()[2].copy()
    labels[299] = 60
    _raises_bit("LABEL", labels=labels)


def test_status_bit_of_a_bad_size_factor():
    sc, labels = _walk()[1].copy(), _walk()[2]
    sc[int(np.flatnonzero(labels >= 0)[-1])] = 0.0
    _raises_bit("SIZE", sc=sc)
    sc = _walk()[1].copy()
    sc[int(np.flatnonzero(labels >= 0)[0])] = 1e151
    _raises_bit("SIZE", sc=sc)


def test_status_bit_of_inadmissible_parameters():
    beta = _walk()[5].copy()
    beta[256] = 0.5
    _raises_bit("PARAMETER", beta=beta)
    alpha = _walk()[4].copy()
    alpha[3] = -1e-18
    _raises_bit("PARAMETER", alpha=alpha)
    alpha = _walk()[4].copy()
    alpha[0] = np.inf
    _raises_bit("PARAMETER", alpha=alpha)


def test_status_bit_of_a_nan_coefficient():
    coef = _walk()[6].copy()
    coef[130, 6] = np.nan
    _raises_bit("COEFFICIENT", coef=coef)


def test_status_bit_of_a_linear_predictor_beyond_700():
    coef = _walk()[6].copy()
    coef[17] = 701.0                                             # the design's rows sum to 1: eta = 701
    _raises_bit("ETA", coef=coef)
    coef[17] = -701.0
    _raises_bit("ETA", coef=coef)


def test_status_bit_of_a_squared_residual_that_overflows_with_the_meat_alone():
    """alpha = 0 and a mean of 1e165: u is about -1e165 and finite, u u is not.  The information's pass is clean; the meat's
    names the bit for every split, also where the sums of U share a block with sums of M (0 times infinity there)."""
    import torch
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, coef, _ = _walk()
    assert alpha[7] == 0.0
    sc, coef = sc.copy(), coef.copy()
    sc[int(np.flatnonzero(labels >= 0)[5])] = 1e100
    coef[7] = 150.0                                              # the design's rows sum to 1: eta = 150
    view = torch.as_tensor(X).cuda()
    clean = regress.normal_equations(view, sc, labels, D, coef, alpha, beta)
    assert np.all(np.isfinite(clean.score)) and np.all(np.isfinite(clean.information))
    assert M.normal_equations(X, sc, labels, D, coef, alpha, beta, True).status == regress.ETA
    for split in (0, 8, 16, 32):
        with pytest.raises(ValueError) as err:
            regress.normal_equations(view, sc, labels, D, coef, alpha, beta, meat=True, split=split)
        assert str(err.value).startswith("status bit ETA ") and "; " not in str(err.value)


# -------------------------------------------------------------------------------------------------------- end to end

@functools.lru_cache(maxsize=None)
def _sampled(flat):
    """3 000 cells of ``sample_density`` on smoke()'s tree (alpha = 0.2, beta = 2), or on the tree with every gene's means
    flattened to their average over the nodes: (X device, rows, sc, tree)."""
    from prosstt_amd import simulation as sim
    from prosstt_amd.tree import Tree
    t = _tree()
    if flat:
        means = t.means
        level = np.concatenate([means[b] for b in t.branches]).mean(axis=0)
        t = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1,
                 modules=5, G=300)
        t.add_genes({b: np.repeat(level[None, :], 20, axis=0) for b in t.branches})
    np.random.seed(1234)
    X, pt, br, sc = sim.sample_density(t, 3000, alpha=np.full(300, 0.2), beta=np.full(300, 2.0), seed=11, out="torch")
    return X, sim.cell_rows(t, pt, br), np.asarray(sc, dtype=np.float64), t


def _host_matrix(X):
    from prosstt_amd import device
    return (X.in_plan_order() if isinstance(X, device.PresentedCounts) else X).cpu().numpy()


def test_regression_end_to_end_on_the_smoke_tree():
    from prosstt_amd import fit, mapping, markers, regress
    X, rows, sc, t = _sampled(False)
    design = regress.tree_design(t, 1)
    assert design.matrix.shape == (60, 7)
    r = regress.regression(X, sc, rows, design, alpha=0.2, beta=2.0, robust=True)
    assert np.all(r.converged | r.no_counts) and r.converged.sum() >= 290 and not r.separated.any()
    want = M.regression(_host_matrix(X), sc, rows, design, 0.2, 2.0, robust=True)
    figures = _assert_coefficients(r, want, _host_matrix(X), sc, rows, design.matrix, 0.2, 2.0)
    keep = r.converged
    print("regression: %d genes, %d with equal rounds (%d .. %d); |coef - model| at most %.3g, %.3g of what the sums' bound "
          "allows (the smallest allowance %.3g)" % (figures[0], figures[1], r.rounds[keep].min(), r.rounds[keep].max(), figures[2],
                                                   figures[3], figures[4]))
    assert np.allclose(r.se[keep], want.se[keep], rtol=1e-9)
    # the fitted means are what the rest of the package takes
    fitted = r.fitted()
    assert fitted.shape == (60, 300)
    ok = ~r.no_counts
    f = fit.count_model(X, sc, rows, np.where(ok[None, :], fitted, 1.0), max_rounds=4)
    assert f.alpha.shape == (300,)
    table = mapping.node_table(t)
    from prosstt_amd.tree import Tree
    t2 = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1, modules=5, G=300)
    t2.add_genes({b: np.where(ok[None, :], fitted, 1.0)[table.offsets[i]:table.offsets[i + 1]] for i, b in enumerate(table.names)})
    assert t2.means["B"].shape == (20, 300)
    # the one-hot design at alpha = 0, beta = 1 is the groups' pseudobulk
    groups = table.branch_code[rows]
    g = regress.regression(X, sc, groups, regress.group_design(3), alpha=0.0, beta=1.0, tol=1e-12)
    bulk = markers.group_moments(X, sc, groups).pseudobulk(sc)
    has = ~g.no_counts
    assert g.converged[has].all()
    seen = bulk[:, has] > 0                                      # (a group without a count of a gene: its coefficient is stopped)
    np.testing.assert_allclose(g.fitted()[:, has][seen], bulk[:, has][seen], rtol=1e-4)


def test_regression_with_cells_left_out():
    """Cells with a negative label take no part, whatever their size factor is (0 here, which the header admits for them);
    with no cell left the call is refused by name."""
    import torch
    from prosstt_amd import regress
    X, sc, labels, D, alpha, beta, _, _ = _walk()
    out = np.flatnonzero(labels < 0)
    assert out.size >= 10
    sc = sc.copy()
    sc[out[:3]] = 0.0
    r = regress.regression(torch.as_tensor(X).cuda(), sc, labels, D, alpha=alpha, beta=beta)
    want = M.regression(X, sc, labels, D, alpha, beta)
    assert want.converged.all()
    figures = _assert_coefficients(r, want, X, sc, labels, D, alpha, beta)
    print("regression, cells left out: %d genes, %d with equal rounds; |coef - model| at most %.3g, %.3g of the allowance"
          % figures[:4])
    with pytest.raises(ValueError, match="at least one cell with a label >= 0"):
        regress.regression(torch.as_tensor(X).cuda(), sc, np.full(300, -1), D, alpha=alpha, beta=beta)


# The numpy model on numpy's negative binomial from the flattened tree's means, these cells' sizes and labels, 24 seeds
# (tools/regress_calibration.py writes these lines; DESIGN section 31 holds them too): the mean of the Wald statistic of "all
# knots equal" over the genes and the share of genes above the chi-square 95 % point of 6 degrees of freedom, each with its
# standard deviation over the seeds; and on the tree as it is, where the genes do change, the share of rejections with its.
# The device on the sampler's own counts gave mean 6.2579 and share 0.0433 on the flattened tree, and 0.4033 on the tree as it is.
NULL_MEAN, NULL_MEAN_SD = 5.9884, 0.1900
NULL_SHARE, NULL_SHARE_SD = 0.0492, 0.0078
CHANGING_SHARE, CHANGING_SHARE_SD = 0.4104, 0.0146
CHANGING_MARGIN = CHANGING_SHARE - 5.0 * CHANGING_SHARE_SD - NULL_SHARE      # 0.2882: the model's margin at its 5 sd low end


def test_calibration_of_the_wald_statistic():
    import scipy.stats
    from prosstt_amd import regress
    point = scipy.stats.chi2.ppf(0.95, 6)
    X, rows, sc, t = _sampled(True)
    design = regress.tree_design(t, 1)
    r = regress.regression(X, sc, rows, design, alpha=0.2, beta=2.0)
    w = r.wald(design.constant())
    have = np.isfinite(w.statistic)
    assert have.sum() >= 290 and np.all(w.df == 6)
    mean, share = float(w.statistic[have].mean()), float((w.statistic[have] > point).mean())
    print("calibration, flat tree: mean %.4f, share above %.3f: %.4f, %d genes" % (mean, point, share, have.sum()))
    assert abs(mean - NULL_MEAN) <= 5.0 * NULL_MEAN_SD
    assert abs(share - NULL_SHARE) <= 5.0 * NULL_SHARE_SD
    X, rows, sc, t = _sampled(False)
    r = regress.regression(X, sc, rows, design, alpha=0.2, beta=2.0)
    w = r.wald(design.constant())
    have = np.isfinite(w.statistic)
    changing = float((w.statistic[have] > point).mean())
    print("calibration, smoke()'s tree: share above %.3f: %.4f, adjusted below 0.05: %.4f" % (
        point, changing, float((w.pvals_adj[have] < 0.05).mean())))
    assert changing - NULL_SHARE >= CHANGING_MARGIN
