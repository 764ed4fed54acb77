"""-m gpu: prosstt_amd.trends on the device.  The integer sums bit for bit against tests/trends_model.py on every path of the
pass (aligned rows, a view one column off, a row stride above G; strips whole and ragged; nodes of none, one and several
chunks); the largest admissible sums; the same bytes for every entries_per_block, stream, column slice and presentation;
cross-checks with markers and count_summary; each status bit alone; stale memory; rows 2^24 + 4 elements apart; and the whole
loop from a simulation's counts back to a tree that simulates again."""
import functools

import numpy as np
import pytest

import trends_model as tm

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
NS = (1, 2, 7, 161, 300)
GS = (1, 3, 255, 256, 257, 1023, 1024, 1025, 1029, 2051)
RS = (1, 5, 40)
LAYOUTS = ("aligned", "shifted", "wide")


def _counts(N, G, kind, rng):
    """About two thirds zeros; "big" holds INT_MAX in every row and column it can."""
    X = rng.poisson(3.0, size=(N, G)).astype(np.int64) * (rng.random((N, G)) < 1 / 3)
    if kind == "big":
        X[rng.random((N, G)) < 0.05] = INT_MAX
        X[rng.random((N, G)) < 0.05] = 65537
        X[0, 0] = X[N - 1, G - 1] = INT_MAX
    return X.astype(np.int32)


def _view(host, layout):
    """The host matrix on the device: "aligned" (base on 16 bytes, a row stride that is a multiple of 4: the 16-byte loads),
    "shifted" (the view starts one column in: the 4-byte loads), "wide" (a row stride of G + 7 behind an aligned base)."""
    import torch
    N, G = host.shape
    ld, shift = {"aligned": (-(-G // 4) * 4, 0), "shifted": (G + 4, 1), "wide": (G + 7, 0)}[layout]
    wide = torch.full((N, ld), 12345, dtype=torch.int32, device="cuda")
    wide[:, shift:shift + G] = torch.from_numpy(host).cuda()
    view = wide[:, shift:shift + G]
    assert view.data_ptr() % 16 == 4 * shift
    return view


def _csr(R, N, rng, longest=None):
    """Random rows: empty ones, one entry, a few, and up to ``longest`` entries, with repeated cells and weights 0 .. 4096
    (zeros and 4096 among them)."""
    longest = 2 * N + 3 if longest is None else longest
    lengths = rng.choice([0, 1, 3, 4, 5, longest // 2, longest], size=R)
    if R >= 5:
        lengths[[0, 2]] = [longest, 0]
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, N, nnz).astype(np.int32)
    weights = rng.integers(0, 4097, nnz).astype(np.int32)
    weights[rng.random(nnz) < 0.1] = 0
    weights[rng.random(nnz) < 0.1] = 4096
    return indptr, indices, weights


def _expected(X, csr):
    S1, S2 = tm.node_sums(X, *csr)
    return tm.as_int64(S1), tm.words(S2)


def _weights(csr, N):
    from prosstt_amd import trends
    return trends.NodeWeights(csr[0], csr[1], csr[2], N)


@pytest.mark.parametrize("kind", ["small", "big"])
@pytest.mark.parametrize("G", GS)
def test_sums_bit_for_bit_against_the_model(G, kind):
    from prosstt_amd import trends
    rng = np.random.default_rng(1000 * G + (kind == "big"))
    big_s2 = 0
    for N in NS:
        X = _counts(N, G, kind, rng)
        views = {layout: _view(X, layout) for layout in LAYOUTS}
        for R in RS:
            csr = _csr(R, N, rng)
            s1, s2 = _expected(X, csr)
            big_s2 += int(np.count_nonzero(s2[..., 1]))
            for layout in LAYOUTS:
                got = trends.node_sums(views[layout], _weights(csr, N))
                assert got.s1.dtype == np.int64 and got.s2_words.dtype == np.uint64
                assert np.array_equal(got.s1, s1), (N, R, layout)
                assert np.array_equal(got.s2_words, s2), (N, R, layout)
    assert (big_s2 > 0) == (kind == "big")           # sums of squares above 2^64 among them


def test_the_largest_admissible_sums():
    """One node of 2^20 - 1 entries, every count 2^31 - 1, every weight 4096: S1 is just below 2^63 and every accumulator of the
    pass just below 2^64."""
    import torch
    from prosstt_amd import trends
    n = trends.MAX_ROW_ENTRIES
    rng = np.random.default_rng(20)
    X = torch.full((3, 5), INT_MAX, dtype=torch.int32, device="cuda")
    w = trends.NodeWeights(np.array([0, n], dtype=np.int64), rng.integers(0, 3, n).astype(np.int32),
                           np.full(n, 4096, dtype=np.int32), 3)
    want1, want2 = n * 4096 * INT_MAX, n * 4096 * INT_MAX * INT_MAX
    assert 2 ** 62 < want1 < 2 ** 63 and want2 >> 64
    for epb in (0, 1 << 20, 4096):
        got = trends.node_sums(X, w, entries_per_block=epb)
        assert got.s1.tolist() == [[want1] * 5]
        assert got.s2().tolist() == [[want2] * 5]
        assert got.s2_words[0, 0].tolist() == [want2 & (2 ** 64 - 1), want2 >> 64]


@functools.lru_cache(maxsize=None)
def _case():
    """N = 161, G = 1029 (one whole strip and a remainder), five nodes of 0 to 325 entries, "big" counts."""
    rng = np.random.default_rng(161 * 1029)
    X = _counts(161, 1029, "big", rng)
    csr = _csr(5, 161, rng)
    X.setflags(write=False)
    return X, csr, _expected(X, csr)


def _bytes(sums):
    import torch
    out = []
    for a in (sums.s1, sums.s2_words):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        out.append(np.ascontiguousarray(a).tobytes())
    return out


def test_the_same_bytes_for_every_entries_per_block_stream_slice_and_presentation():
    import torch
    from prosstt_amd import device, trends
    X, csr, (s1, s2) = _case()
    w = _weights(csr, 161)
    view = _view(np.array(X), "aligned")
    base = trends.node_sums(view, w)
    assert np.array_equal(base.s1, s1) and np.array_equal(base.s2_words, s2)
    for epb in (1, 7, 64, 4096):
        assert _bytes(trends.node_sums(view, w, entries_per_block=epb)) == _bytes(base), epb
        assert _bytes(trends.node_sums(_view(np.array(X), "shifted"), w, entries_per_block=epb)) == _bytes(base), epb
    assert _bytes(trends.node_sums(view, w, out="torch")) == _bytes(base)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = trends.node_sums(view, w, entries_per_block=7)
    stream.synchronize()
    assert _bytes(other) == _bytes(base)
    # a column slice against the full call
    for lo, hi in ((0, 1024), (3, 1029), (500, 501)):
        part = trends.node_sums(view[:, lo:hi], w)
        assert np.array_equal(part.s1, s1[:, lo:hi]) and np.array_equal(part.s2_words, s2[:, lo:hi]), (lo, hi)
    # a presented matrix against its plan-order matrix: row i holds cell perm[i]
    perm = np.random.default_rng(5).permutation(161)
    presented = device.PresentedCounts(_view(np.ascontiguousarray(np.array(X)[perm]), "aligned"), perm)
    assert _bytes(trends.node_sums(presented, w)) == _bytes(base)
    on_device = trends.NodeWeights(*(torch.from_numpy(a).cuda() for a in csr), 161)
    assert _bytes(trends.node_sums(presented, on_device, entries_per_block=64)) == _bytes(base)
    assert _bytes(trends.node_sums(view, on_device)) == _bytes(base)


# ------------------------------------------------------------------------------------------------ what exists already

@functools.lru_cache(maxsize=None)
def _simulation():
    """smoke()'s tree, and 3 000 cells of ``sample_density`` from it: alpha = 0.2, beta = 2, library sizes scaled."""
    import torch
    from prosstt_amd import simulation as sim, sim_utils as sut
    from prosstt_amd.tree import Tree
    state = np.random.get_state()
    np.random.seed(92)
    t = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3, branch_points=1, modules=5,
             G=300)
    rel, _, _ = sim.simulate_lineage(t, a=0.05, intra_branch_tol=0)
    t.add_genes(rel, sut.simulate_base_gene_exp(t, rel))
    X, pt, br, sc = sim.sample_density(t, 3000, alpha=0.2, beta=2.0, seed=11, out="torch", order="plan")
    np.random.set_state(state)
    torch.cuda.synchronize()
    return t, X, np.asarray(pt), np.asarray(br), np.asarray(sc)


def test_nearest_is_markers_count_sum():
    from prosstt_amd import markers, trends
    t, X, pt, br, sc = _simulation()
    w = trends.node_weights(t, pt, br, kernel="nearest")
    got = trends.node_sums(X, w)
    gm = markers.group_moments(X, sc, w.labels)
    assert got.s1.shape == (60, 300) and len(gm.groups) == 60
    assert np.array_equal(got.s1, 4096 * np.asarray(gm.count_sum))
    tr = trends.expression_trends(X, sc, t, pt, br, kernel="nearest")
    np.testing.assert_allclose(tr.means, gm.pseudobulk(sc), rtol=1e-6)     # (exposure sums float32 size factors)
    assert abs(tr.density.sum() - 1.0) < 1e-12


def test_one_node_of_all_cells_is_count_summary():
    from prosstt_amd import summary, trends
    X, _, _ = _case()
    view = _view(np.array(X), "shifted")
    w = trends.NodeWeights(np.array([0, 161], dtype=np.int64), np.arange(161, dtype=np.int32),
                           np.full(161, 4096, dtype=np.int32), 161)
    got = trends.node_sums(view, w)
    cs = summary.count_summary(view)
    assert np.array_equal(got.s1[0], 4096 * cs.gene_sum)
    assert got.s2()[0].tolist() == [4096 * int(v) for v in cs.gene_sumsq]
    assert max(int(v) for v in cs.gene_sumsq) >= 1 << 64


# ------------------------------------------------------------------------------------------------------ status bits

def test_each_status_bit_alone_and_a_skipped_entry_leaves_the_rest_exact():
    import torch
    from prosstt_amd import trends
    X, csr, _ = _case()
    X = np.array(X)
    view = _view(X, "aligned")
    indptr, indices, weights = (a.copy() for a in csr)
    e = int(indptr[1]) - 2                            # in the tail of the first node's entries
    f = 1                                             # inside its first batch of four

    def device_weights(ind, wts):
        return trends.NodeWeights(torch.from_numpy(indptr).cuda(), torch.from_numpy(ind).cuda(), torch.from_numpy(wts).cuda(),
                                  161)

    def without(*entries):                            # the model without the skipped entries: weight 0
        wts = weights.copy()
        wts[list(entries)] = 0
        return _expected(X, (indptr, indices, wts))

    for bit, name, bad_index, bad_weight in ((2, "INDEX_RANGE", 161, None), (2, "INDEX_RANGE", -1, None),
                                             (2, "INDEX_RANGE", INT_MAX, None), (4, "WEIGHT_RANGE", None, 4097),
                                             (4, "WEIGHT_RANGE", None, -1)):
        ind, wts = indices.copy(), weights.copy()
        for at in (e, f):
            if bad_index is not None:
                ind[at] = bad_index
            else:
                wts[at] = bad_weight
        for epb in (0, 7):
            sums, bits = trends._node_sums(view, device_weights(ind, wts), epb)
            assert bits == bit, (name, bits)
            s1, s2 = without(e, f)
            assert np.array_equal(sums.s1, s1) and np.array_equal(sums.s2_words, s2), name
        with pytest.raises(ValueError, match=r"status bit %s \(%d\)" % (name, bit)) as err:
            trends.node_sums(view, device_weights(ind, wts))
        assert str(err.value).count("status bit") == 1
    # a negative count
    neg = X.copy()
    neg[int(indices[0]), 1028] = -5
    sums, bits = trends._node_sums(_view(neg, "aligned"), device_weights(indices, weights))
    assert bits == 1
    with pytest.raises(ValueError, match=r"status bit NEGATIVE \(1\): the count matrix has a negative entry"):
        trends.node_sums(_view(neg, "shifted"), _weights(csr, 161))
    # offsets that do not ascend, through device tensors: reported, nothing read out of bounds
    crooked = indptr.copy()
    crooked[2] = crooked[1] - 1
    w = trends.NodeWeights(torch.from_numpy(crooked).cuda(), torch.from_numpy(indices).cuda(),
                           torch.from_numpy(weights).cuda(), 161)
    assert trends._node_sums(view, w)[1] == 8


# ----------------------------------------------------------------------------------------------------- stale memory

def calls_trends(place=lambda value: value):
    """The library's label and its calls over ``_case`` and ``_simulation``; ``place`` puts the device inputs
    (tests/test_gpu_stale_memory.py)."""
    from prosstt_amd import trends
    X, csr, _ = _case()
    shifted, aligned = place(_view(np.array(X), "shifted")), place(_view(np.array(X), "aligned"))
    w = _weights(csr, 161)
    t, Xs, pt, br, sc = _simulation()
    part = place(Xs[:, :257])

    def whole():
        tr = trends.expression_trends(part, sc, t, pt, br, bandwidth=3.0)
        return (tr.means, tr.variances, tr.density, tr.labels, tr.weight, tr.exposure, tr.effective_cells, tr.empty,
                tr.sums.s1, tr.sums.s2_words)

    return "trends", {
        "node_sums": lambda: trends.node_sums(shifted, w),
        "node_sums in chunks of 7, out='torch'": lambda: trends.node_sums(aligned, w, entries_per_block=7, out="torch"),
        "expression_trends": whole,
    }


def test_no_result_depends_on_stale_memory():
    from test_gpu_stale_memory import _thrice
    _thrice(*calls_trends())


# ------------------------------------------------------------------------------------------------------ far offsets

from test_gpu_far_offsets import arena  # noqa: E402,F401  (the 19 GiB buffer, allocated for this module's one case)


def test_rows_2_to_the_24_plus_4_elements_apart(arena):  # noqa: F811
    import test_gpu_far_offsets as far
    from prosstt_amd import trends
    X = far._inputs()["X"]                            # 161 x 1029, INT_MAX among the counts
    stride, near_stride, shift = far.PATHS["vector"]
    rng = np.random.default_rng(24)
    csr = _csr(5, far.N, rng)
    csr[1][:8] = np.arange(153, 161)                  # rows beyond element 2^31 in the first batches
    s1, s2 = _expected(np.array(X), csr)
    w = _weights(csr, far.N)
    near = trends.node_sums(far._near(X, near_stride, shift), w)
    assert np.array_equal(near.s1, s1) and np.array_equal(near.s2_words, s2)
    got = trends.node_sums(far._far(arena, X, stride, shift), w)
    assert _bytes(got) == _bytes(near)


# ---------------------------------------------------------------------------------------------------------- the loop

# The statistics of z under the sampler's law, measured without the code under test: 24 seeds of numpy's negative binomial
# (n = mu / (alpha mu + beta - 1), p = 1 / (alpha mu + beta)) from the same means, size factors, pseudotimes and branches as
# _simulation(), the sums by tests/trends_model.py, bandwidth 3 (14 828 entries, at most 365 per node); as (mean, standard
# deviation over the seeds, ddof 1).  The windows overlap, so neighbouring nodes share cells and the spread is wider than
# that of 18 000 independent values.  DESIGN.md, section 25, has the same figures.
MEAN_Z = (9.78e-05, 0.014835)            # the device's own matrix gave 0.0334, its re-simulation -0.0109
MEAN_Z2 = (1.003331, 0.022584)           # the device's own matrix gave 1.0175, its re-simulation 1.0029
SIGMAS = 5.0


def z_statistics(s1, weights, sc, rows, M, alpha, beta):
    """(mean of z, mean of z^2) of the module docstring of the loop: z = (S1 - E) / sqrt(Var) over the nodes and genes with
    Var > 0, E = sum_e q_e s_e M[row(c_e)][g], Var = sum_e q_e^2 (alpha mu^2 + beta mu), mu = s_e M[row(c_e)][g]."""
    import scipy.sparse as sparse
    R, N = len(weights.indptr) - 1, weights.n_cells
    Q = sparse.csr_matrix((weights.weights.astype(np.float64), weights.indices, weights.indptr), shape=(R, N))
    mu = np.asarray(sc, dtype=np.float64)[:, None] * M[rows]
    E = Q @ mu
    V = Q.multiply(Q) @ (alpha * mu * mu + beta * mu)
    keep = V > 0
    z = (np.asarray(s1, dtype=np.float64)[keep] - E[keep]) / np.sqrt(V[keep])
    return float(z.mean()), float((z * z).mean())


def _assert_z(stats, what):
    print("%s: mean z %.5f, mean z^2 %.5f" % ((what,) + stats))
    assert abs(stats[0] - MEAN_Z[0]) <= SIGMAS * MEAN_Z[1], what
    assert abs(stats[1] - MEAN_Z2[0]) <= SIGMAS * MEAN_Z2[1], what


def test_the_loop_from_counts_back_to_a_tree_that_simulates_again():
    import torch
    from prosstt_amd import fit, simulation as sim, trends
    t, X, pt, br, sc = _simulation()
    rows = sim.cell_rows(t, pt, br)
    tr = trends.expression_trends(X, sc, t, pt, br, bandwidth=3.0)
    assert tr.means.shape == (60, 300) and len(tr.empty) == 0 and np.array_equal(tr.labels, rows)
    _assert_z(z_statistics(tr.sums.s1, tr.node_weights, sc, rows, fit.simulation_means(t), 0.2, 2.0), "the simulation")
    # the fit takes the node means as they are
    f = fit.count_model(X, sc, tr.labels, tr.means)
    has_counts = X.sum(dim=0).cpu().numpy() > 0
    assert has_counts.sum() > 250
    assert np.all(np.isfinite(f.alpha[has_counts])) and np.all(np.isfinite(f.beta[has_counts]))
    print("fitted alpha: median %.4f, beta: median %.4f" % (np.median(f.alpha[has_counts]), np.median(f.beta[has_counts])))
    # the learned tree simulates again (sample_density raises where the sampler's domain check fails)
    new = tr.to_tree()
    alpha = np.where(np.isfinite(f.alpha), f.alpha, 0.2)
    beta = np.where(np.isfinite(f.beta), f.beta, 2.0)
    state = np.random.get_state()
    np.random.seed(93)
    X2, pt2, br2, sc2 = sim.sample_density(new, 3000, alpha=alpha, beta=beta, seed=12, out="torch", order="plan")
    np.random.set_state(state)
    torch.cuda.synchronize()
    pt2, br2, sc2 = np.asarray(pt2), np.asarray(br2), np.asarray(sc2)
    tr2 = trends.expression_trends(X2, sc2, new, pt2, br2, bandwidth=3.0)
    _assert_z(z_statistics(tr2.sums.s1, tr2.node_weights, sc2, sim.cell_rows(new, pt2, br2), fit.simulation_means(new), alpha[None, :],
                           beta[None, :]), "the simulation of the learned tree")
