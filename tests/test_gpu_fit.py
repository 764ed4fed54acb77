"""-m gpu: prosstt_amd/fit.py and libprosstt_amd_fit.so against the numpy model (tests/fit_model.py): the sums of the
pass on ragged shapes, strided and unaligned views, every regime of the term and both ends of the parameter box; equal bits
across streams, views and slices of the genes; one test per status bit; ``LogLik.concat``; ``count_model`` end to end against
the model; and the test the feature exists for: a simulation refitted against its true means has chi-square likelihood
ratios.

Tolerance of the sums.  |ll_device - ll_model| <= EPS * S[c][g], S the model's sum of |lgd| + r L1 + x |log theta - L1|
over the entries; base likewise relative to itself.  The largest ratio measured over the cases of this file on an MI355X
was 1.9e-15 for ll and 2.6e-15 for base; EPS is 8 times the larger (the margin covers another ROCm's log and a
different blocking of the rows) and may never exceed 2^-40.

The refits measured there: 2 (l_hat - l_truth) had mean 1.99, largest 10.4, 4.3 % above 5.99 with both parameters free
(299 of 300 genes converged within 60 rounds, 9 on the box), and mean 1.04, largest 6.9 with alpha alone."""
import functools

import numpy as np
import pytest

import fit_model as M

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
EPS = 8 * 2.6e-15               # 8 x the largest |device - model| / S measured (see above)
assert EPS <= 2.0 ** -40

NS = [1, 2, 63, 64, 65, 257]
GS = [1, 3, 63, 64, 65, 257, 1025]
KS = [1, 2, 7, 300]
CS = [1, 2, 9, 16]
PADS = [0, 1, 3, 64]
KINDS = ["zeros", "nb", "big"]
# (N, G, K, C, pad, kind, shift): a sweep that meets every value of every list, then the rows that must start on 16 bytes
# with full and partial strips of 256 genes (the staged loads), with each kind
CASES = [(NS[i % 6], GS[(3 * i + i // 7) % 7], KS[(i + i // 4) % 4], CS[(i // 2 + i // 8) % 4], PADS[(i // 2) % 4],
          KINDS[i % 3], (i // 5) % 2) for i in range(28)]
CASES += [(257, 1025, 7, 9, 3, "big", 0), (65, 257, 300, 16, 3, "nb", 0), (257, 64, 2, 1, 64, "big", 0),
          (64, 1025, 1, 2, 3, "zeros", 0), (63, 257, 7, 16, 3, "big", 0)]


def test_the_cases_cover_every_listed_value():
    for column, values in enumerate((NS, GS, KS, CS, PADS, KINDS)):
        assert {case[column] for case in CASES} == set(values)
    assert any(shift for *_, shift in CASES)
    staged = [c for c in CASES if (c[1] + c[4]) % 4 == 0 and c[6] == 0 and c[1] >= 256]
    assert {c[5] for c in staged} == set(KINDS)


def _matrix(N, G, pad, kind, shift, rng):
    """(host matrix, device view of it): G columns from column ``shift`` of a tensor of row stride G + pad
    (tests/test_gpu_hvg.py's pattern)."""
    import torch
    shift = shift if pad > 0 else 0
    width = G + pad
    if kind == "zeros":
        W = np.zeros((N, width), dtype=np.int32)
    else:
        W = rng.negative_binomial(0.5, 0.1, size=(N, width)).astype(np.int32)
        if kind == "big":
            special = np.array([INT_MAX, 33047, 12, 13, 14, 1, 0], dtype=np.int32)
            pick = rng.random((N, width)) < 0.5
            W[pick] = special[rng.integers(0, special.size, size=int(pick.sum()))]
    D = torch.as_tensor(W).cuda()
    return W[:, shift:shift + G], D[:, shift:shift + G]


def _inputs(N, G, K, C, rng):
    """(size, labels, means, alpha, beta): some labels negative, exact zeros among the means, candidates over the whole box
    with both corners, and genes at b = 1 and at a = 0."""
    sc = rng.lognormal(0.0, 0.35, size=N)
    labels = rng.integers(-1, K, size=N)
    means = rng.lognormal(0.5, 1.2, size=(K, G))
    means[rng.random((K, G)) < 0.1] = 0.0
    u = rng.uniform(-12.0, 4.0, size=(C, G))
    v = rng.uniform(-12.0, 4.0, size=(C, G))
    u[0], v[0] = -12.0, 4.0
    u[C - 1, G // 2:], v[C - 1, G // 2:] = 4.0, -12.0
    alpha, beta = np.exp(u), 1.0 + np.exp(v)
    beta[:, 0::5] = 1.0                                # the textbook negative binomial
    alpha[:, 1::5] = 0.0                               # the quasi-Poisson end
    return sc, labels, means, alpha, beta


def _ratios(got, want):
    ll, base, bad, S = want
    assert np.array_equal(got.bad, bad)
    assert np.all(np.isfinite(got.values)) and np.all(np.isfinite(got.base))
    with np.errstate(invalid="ignore", divide="ignore"):
        r_ll = np.where(S > 0, np.abs(got.values - ll) / S, np.abs(got.values - ll))
        r_base = np.where(base > 0, np.abs(got.base - base) / base, np.abs(got.base - base))
    return float(r_ll.max()), float(r_base.max())


@pytest.mark.parametrize("N,G,K,C,pad,kind,shift", CASES)
def test_loglik_against_the_model(N, G, K, C, pad, kind, shift):
    from prosstt_amd import fit
    rng = np.random.default_rng(N * 100003 + G * 7 + pad + 31 * C + K)
    X, view = _matrix(N, G, pad, kind, shift, rng)
    sc, labels, means, alpha, beta = _inputs(N, G, K, C, rng)
    got = fit.loglik(view, sc, labels, means, alpha, beta)
    assert got.values.shape == (C, G) and got.base.shape == (G,) and got.n_cells == N
    want = M.loglik(X, sc, labels, means, alpha, beta)
    r_ll, r_base = _ratios(got, want)
    print("fit ratio %s: ll %.3g base %.3g bad %d" % ((N, G, K, C, pad, kind, shift), r_ll, r_base, int(want[2].sum())))
    assert r_ll <= EPS and r_base <= EPS
    if kind != "zeros" and N >= 63 and G >= 63:
        assert want[2].sum() > 0                       # counts at a mean of 0 were met
    if kind == "zeros":
        assert not got.bad.any() and not got.base.any()


@functools.lru_cache(maxsize=None)
def _shared():
    """One matrix with its inputs and the model's sums, for the tests that need no shape of their own."""
    rng = np.random.default_rng(77)
    N, G, K, C = 257, 257, 7, 9
    X, view = _matrix(N, G, 0, "big", 0, rng)
    sc, labels, means, alpha, beta = _inputs(N, G, K, C, rng)
    return X, view, sc, labels, means, alpha, beta, M.loglik(X, sc, labels, means, alpha, beta)


def _same(a, b):
    return (a.values.tobytes() == b.values.tobytes() and a.base.tobytes() == b.base.tobytes()
            and np.array_equal(a.bad, b.bad))


def test_equal_bits_on_a_second_stream_through_a_view_and_over_halves_of_the_genes():
    import torch
    from prosstt_amd import fit
    X, view, sc, labels, means, alpha, beta, _ = _shared()
    first = fit.loglik(view, sc, labels, means, alpha, beta)
    with torch.cuda.stream(torch.cuda.Stream()):
        other = fit.loglik(view, sc, labels, means, alpha, beta)
    assert _same(first, other)
    wide = torch.zeros((257, 257 + 7), dtype=torch.int32, device="cuda")
    wide[:, 3:260] = view                              # row stride 264, the base 12 bytes off: the unaligned kernel
    assert _same(first, fit.loglik(wide[:, 3:260], sc, labels, means, alpha, beta))
    # 257 genes are two strips and 128 / 129 genes one, all with five blocks of rows (257 cells, 64 at the least per block)
    halves = [fit.loglik(view[:, lo:hi], sc, labels, means[:, lo:hi], alpha[:, lo:hi], beta[:, lo:hi])
              for lo, hi in ((0, 128), (128, 257))]
    assert np.concatenate([h.values for h in halves], axis=1).tobytes() == first.values.tobytes()
    assert np.concatenate([h.base for h in halves]).tobytes() == first.base.tobytes()
    assert np.array_equal(np.concatenate([h.bad for h in halves]), first.bad)
    # a candidate's sums do not depend on the other candidates of the call
    alone = fit.loglik(view, sc, labels, means, alpha[5], beta[5])
    assert alone.values[0].tobytes() == first.values[5].tobytes()


def _raises_bit(name, **changed):
    from prosstt_amd import fit
    X, view, sc, labels, means, alpha, beta, _ = _shared()
    args = dict(X=view, sc=sc, labels=labels, means=means, alpha=alpha, beta=beta)
    args.update(changed)
    with pytest.raises(ValueError, match="status bit %s " % name):
        fit.loglik(args["X"], args["sc"], args["labels"], args["means"], args["alpha"], args["beta"])


def test_status_bit_of_a_negative_count():
    view = _shared()[1].clone()
    view[100, 200] = -1
    _raises_bit("NEGATIVE", X=view)


def test_status_bit_of_a_label_beyond_the_means():
    labels = _shared()[3].copy()
    labels[256] = 7
    _raises_bit("LABEL", labels=labels)


def test_status_bit_of_beta_below_one():
    beta = _shared()[6].copy()
    beta[8, 256] = 0.5
    _raises_bit("PARAMETER", beta=beta)


def test_status_bit_of_parameters_a_rounding_slip_outside_the_domain():
    """beta = 1 - 1e-12 with alpha = 0, and alpha = -1e-18 with beta = 1: theta would be a tiny negative number and r an
    enormous negative one.  The kernel judges the pair before it computes with it (and runs on (0, 2) in its place), so the
    call takes the time of any other and names the bit."""
    import time
    alpha, beta = _shared()[5].copy(), _shared()[6].copy()
    alpha[2, 7], beta[2, 7] = 0.0, 1.0 - 1e-12
    t0 = time.perf_counter()
    _raises_bit("PARAMETER", alpha=alpha, beta=beta)
    alpha, beta = _shared()[5].copy(), _shared()[6].copy()
    alpha[8, 200], beta[8, 200] = -1e-18, 1.0
    _raises_bit("PARAMETER", alpha=alpha, beta=beta)
    assert time.perf_counter() - t0 < 5.0


def test_status_bit_of_a_nan_parameter():
    alpha = _shared()[5].copy()
    alpha[0, 0] = np.nan
    _raises_bit("PARAMETER", alpha=alpha)


def test_status_bit_of_a_size_factor_of_zero():
    sc, labels = _shared()[2].copy(), _shared()[3]
    sc[int(np.flatnonzero(labels >= 0)[-1])] = 0.0
    _raises_bit("SIZE", sc=sc)


def test_status_bit_of_a_negative_mean_and_status_is_left_clean():
    from prosstt_amd import fit
    X, view, sc, labels, means, alpha, beta, want = _shared()
    bad = means.copy()
    bad[int(labels.max()), 130] = -1.0
    _raises_bit("MEAN", means=bad)
    assert _ratios(fit.loglik(view, sc, labels, means, alpha, beta), want)[0] <= EPS     # nothing left behind


def test_concat_over_chunks_of_cells_is_the_model_of_the_whole_matrix():
    from prosstt_amd import fit
    X, view, sc, labels, means, alpha, beta, want = _shared()
    parts = [fit.loglik(view[lo:hi], sc[lo:hi], labels[lo:hi], means, alpha, beta) for lo, hi in ((0, 100), (100, 257))]
    whole = fit.LogLik.concat(parts)
    assert whole.n_cells == 257
    r_ll, r_base = _ratios(whole, want)
    assert r_ll <= EPS and r_base <= EPS


def test_presented_counts_are_read_in_place_and_torch_outputs_stay_on_the_device():
    """Row i of a ``device.PresentedCounts`` is cell ``cell_of_row[i]``: labels and size factors are given in plan order and
    permuted to the rows, never the matrix.  The sums are those of the model on the plan-ordered matrix within EPS (the
    rows are added in another order), ``bad`` exactly; ``out="torch"`` returns the same bits as device tensors."""
    import torch
    from prosstt_amd import device, fit
    X, view, sc, labels, means, alpha, beta, want = _shared()
    perm = np.random.default_rng(41).permutation(257)
    presented = device.PresentedCounts(torch.as_tensor(np.ascontiguousarray(X[perm])).cuda(), perm)     # row i is cell perm[i]
    got = fit.loglik(presented, sc, labels, means, alpha, beta)
    r_ll, r_base = _ratios(got, want)
    assert r_ll <= EPS and r_base <= EPS
    rows = fit.loglik(presented.counts, sc[perm], labels[perm], means, alpha, beta)      # the same rows as a plain matrix
    assert _same(got, rows)
    on_device = fit.loglik(presented, sc, labels, torch.as_tensor(means).cuda(), alpha, beta, out="torch")
    assert isinstance(on_device.values, torch.Tensor) and on_device.values.is_cuda and on_device.base.is_cuda
    assert on_device.values.dtype == torch.float64 and tuple(on_device.values.shape) == (9, 257)
    assert on_device.values.cpu().numpy().tobytes() == got.values.tobytes()
    assert on_device.base.cpu().numpy().tobytes() == got.base.tobytes() and np.array_equal(on_device.bad, got.bad)
    whole = fit.LogLik.concat([on_device, on_device])
    assert isinstance(whole.values, torch.Tensor) and whole.n_cells == 514


def test_count_model_end_to_end_against_the_model():
    import torch
    from prosstt_amd import fit
    rng = np.random.default_rng(9)
    N, G, K = 257, 65, 7
    labels = rng.integers(0, K, size=N)
    sc = rng.lognormal(0.0, 0.35, size=N)
    mu = sc[:, None] * rng.lognormal(1.5, 0.8, size=(K, G))[labels]
    theta = 0.3 * mu + 1.0
    X = rng.negative_binomial(mu / theta, 1.0 / (1.0 + theta)).astype(np.int32)
    X[:, 11] = 0                                       # a gene without counts
    got = fit.count_model(torch.as_tensor(X).cuda(), sc, labels)
    want = M.count_model(X, sc, labels)
    np.testing.assert_allclose(got.means, want.means, rtol=1e-13)
    assert np.array_equal(got.converged, want.converged) and np.array_equal(got.at_bound, want.at_bound)
    assert not got.converged[11] and np.isnan(got.alpha[11]) and got.converged.sum() >= 60
    keep = want.converged
    assert np.all(np.abs(got.loglik[keep] - want.loglik[keep]) <= M.OPTIMISER_BOUND)
    assert np.array_equal(np.isnan(got.loglik), np.isnan(want.loglik))


# ------------------------------------------------------------------------------------------ the refit of a simulation

@functools.lru_cache(maxsize=None)
def _tree():
    """smoke()'s tree: 3 branches x 20 steps, 300 genes."""
    from prosstt_amd import simulation as sim, sim_utils as sut
    from prosstt_amd.tree import Tree
    np.random.seed(92)
    t = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1,
             modules=5, G=300)
    rel, _, _ = sim.simulate_lineage(t, a=0.05, intra_branch_tol=0)
    t.add_genes(rel, sut.simulate_base_gene_exp(t, rel))
    return t


def _refit(alpha, beta, **options):
    """(2 (l_hat - l_truth) over the genes kept, the share of genes left out) of 3 000 cells sampled from the tree."""
    from prosstt_amd import fit, simulation as sim
    t = _tree()
    np.random.seed(1234)
    X, pt, br, sc = sim.sample_density(t, 3000, alpha=np.full(300, alpha), beta=np.full(300, beta), seed=11, out="torch")
    rows, means = sim.cell_rows(t, pt, br), fit.simulation_means(t)
    assert means.shape == (60, 300) and means.dtype == np.float64
    f = fit.count_model(X, sc, rows, means, **options)
    truth = fit.loglik(X, sc, rows, means, np.full(300, alpha), np.full(300, beta))
    assert not f.bad.any()
    keep = ~np.isnan(f.loglik)                         # (a gene without any count is left out)
    assert not f.converged[~keep].any()
    return 2.0 * (f.loglik[keep] - (truth.values[0] - truth.base)[keep]), 1.0 - keep.mean(), f


def test_refit_of_a_simulation_has_chi_square_likelihood_ratios():
    from prosstt_amd import fit
    lr, left_out, f = _refit(0.2, 2.0)
    print("refit: mean %.4f, max %.3f, min %.3g, above 5.99: %.3f, left out %.3f" % (lr.mean(), lr.max(), lr.min(),
                                                                                   (lr > 5.99).mean(), left_out))
    assert left_out <= 0.02
    assert lr.min() >= -1e-6 and lr.max() <= 30.0      # P(chi2_2 > 30) = 3e-7
    assert abs(lr.mean() - 2.0) <= 5.0 * 2.0 / np.sqrt(300)
    hp = fit.hyperparameters(f)
    print("refit: %r, %d converged, %d at the box" % (hp, f.converged.sum(), f.at_bound.sum()))
    assert hp.n_genes == int((f.converged & ~f.at_bound).sum()) and np.isfinite(hp.log_alpha_std)


def test_refit_of_a_simulation_with_alpha_alone():
    lr, left_out, f = _refit(0.3, 1.0, free=("alpha",))
    print("refit, alpha alone: mean %.4f, max %.3f, min %.3g, left out %.3f" % (lr.mean(), lr.max(), lr.min(), left_out))
    assert left_out <= 0.02
    assert lr.min() >= -1e-6 and lr.max() <= 30.0
    assert abs(lr.mean() - 1.0) <= 5.0 * np.sqrt(2.0) / np.sqrt(lr.size)
    assert np.all(f.beta[f.converged] == 1.0) and np.all(np.isnan(f.se_log_beta_minus_1))
