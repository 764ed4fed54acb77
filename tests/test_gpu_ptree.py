"""-m gpu: prosstt_amd.ptree on the device against tests/ptree_model.py.  Bit for bit where the definition is IEEE: best and
d2min, the projection's edge, t and q, the hard pass's gamma and sums (the model adds in the header's order), on every shape
class, a row stride of d + 1 and a view one element off, with ties, a zero-length edge and weights that underflow; the soft
pass within the bound derived in DESIGN section 28, and bit for bit where every d2 is equal; the same bits twice, on a second
stream, with and without resp, for device inputs, over stale memory, for subsets and permutations of the rows and for rows
2^24 + 4 elements apart; the fit step by step against the model; and the loop from a bare count matrix to a tree, trends, a
fit and a second simulation."""
import numpy as np
import pytest

import ptree_model as pm

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257, 1030)
RS = (1, 2, 63, 64, 65, 130, 400)
DS = (1, 2, 3, 9, 15, 17, 32, 33, 50, 65, 128)      # every Q of ptree_sums_kernel<Q, HARD> and both sides of each boundary:
#                                                    d = 1 .. 8 -> Q = 1, 9 .. 16 -> 2, 17 .. 32 -> 4, 33 .. 64 -> 8, 65 .. 128 -> 16
LAYOUTS = ("aligned", "wide", "shifted")


def _view(host, layout):
    """The host panel on the device: "aligned" (dense), "wide" (a row stride of d + 1), "shifted" (the view starts one element
    in, rows d + 4 apart)."""
    import torch
    N, d = host.shape
    ld, shift = {"aligned": (d, 0), "wide": (d + 1, 0), "shifted": (d + 4, 1)}[layout]
    wide = torch.full((N, ld), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, shift:shift + d] = torch.from_numpy(np.array(host)).cuda()
    view = wide[:, shift:shift + d]
    assert N == 1 or view.stride(0) == ld
    return view


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _bytes(result):
    import torch
    out = []
    for a in result:
        if a is not None:
            a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
            out.append(np.ascontiguousarray(a).tobytes())
    return out


def _assert_hard(got, want, what):
    assert got.best.dtype == np.int32 and got.sq_distance.dtype == np.float32
    assert np.array_equal(got.best, want.best), what
    assert _same_bits(got.sq_distance, want.sq_distance), what
    assert _same_bits(got.free_energy, want.free_energy), what
    assert _same_bits(got.gamma, want.gamma), what
    assert _same_bits(got.sums, want.sums), what


def _assert_soft(got, want, Y, C, sigma, what):
    """The per-cell argmin bit for bit, the rest within the derived bound."""
    assert np.array_equal(got.best, want.best), what
    assert _same_bits(got.sq_distance, want.sq_distance), what
    f, r, g, s = pm.soft_bound(Y, C, sigma, want)
    worst = {}
    for name, a, b, bound in (("free_energy", got.free_energy, want.free_energy, f), ("resp", got.resp, want.resp, r),
                              ("gamma", got.gamma, want.gamma, g), ("sums", got.sums, want.sums, s)):
        if a is None:
            continue
        err = np.abs(a - b)
        worst[name] = float(np.max(err / bound))
        assert np.all(err <= bound), (what, name, worst[name])
    return worst


# ------------------------------------------------------------------------------------------------------ every shape

@pytest.mark.parametrize("d", DS)
def test_hard_pass_and_projection_bit_for_bit_on_every_shape(d):
    from prosstt_amd import ptree
    rng = np.random.default_rng(4100 + d)
    turn = 0
    for R in RS:
        for N in NS:
            for kind in ("eighths", "gaussian"):
                if kind == "eighths":
                    Y, C = pm.eighths(N, d, int(rng.integers(1 << 30))), pm.eighths(R, d, int(rng.integers(1 << 30)))
                else:
                    Y = rng.standard_normal((N, d)).astype(np.float32)
                    C = rng.standard_normal((R, d)).astype(np.float32)
                layout = LAYOUTS[turn % 3]
                turn += 1
                want = pm.assign(Y, C, 0.0)
                got = ptree.assign(_view(Y, layout), _view(C, LAYOUTS[(turn // 3) % 3]), 0.0, responsibilities=True)
                _assert_hard(got, want, (N, R, d, kind, layout))
                assert _same_bits(got.resp, want.resp)
                if kind == "eighths":
                    assert np.array_equal(got.gamma, np.bincount(want.best, minlength=R).astype(np.float64))
            if R >= 2:
                edges = np.stack([rng.integers(0, R, size=R + 3), rng.integers(0, R, size=R + 3)], axis=1).astype(np.int32)
                edges[0] = (1, 1)                                            # an edge of zero length
                want = pm.project(Y, C, edges)
                got = ptree.project(_view(Y, layout), C, edges)
                assert got.edge.dtype == np.int32 and np.array_equal(got.edge, want.edge), (N, R, d)
                assert _same_bits(got.t, want.t) and _same_bits(got.sq_distance, want.sq_distance), (N, R, d)


def test_ties_go_to_the_lower_index_and_far_centres_underflow():
    from prosstt_amd import ptree
    rng = np.random.default_rng(5)
    N, R, d = 130, 70, 3
    C = pm.eighths(R, d, 1, span=4)
    C[40:] = C[:30]                                                          # duplicate centres
    Y = pm.eighths(N, d, 2, span=4)
    Y[:35] = C[rng.integers(0, R, size=35)]                                  # cells that lie on a centre
    want = pm.assign(Y, C, 0.0)
    got = ptree.assign(Y, C, 0.0)
    _assert_hard(got, want, "ties")
    assert np.all(got.best[:35] < 40) and np.all(got.sq_distance[:35] == 0)
    d2 = pm.d2(Y, C)
    assert np.all(got.best == np.argmin(d2, axis=1))                          # (numpy's argmin takes the first of equals)
    # a zero-length edge beside a duplicate of it: the lower edge wins, t = 0
    edges = np.array([[3, 3], [3, 43], [5, 6], [5, 6]], dtype=np.int32)
    p, w = ptree.project(Y, C, edges), pm.project(Y, C, edges)
    assert np.array_equal(p.edge, w.edge) and _same_bits(p.t, w.t) and _same_bits(p.sq_distance, w.sq_distance)
    assert not np.any(p.edge == 3) and np.all(p.t[p.edge == 0] == 0)
    # centres 1e4 apart at sigma = 1: every weight but the best underflows to 0
    far = (np.arange(R, dtype=np.float32)[:, None] * 1e4 * np.ones((1, d), dtype=np.float32)).astype(np.float32)
    cells = (far[rng.integers(0, R, size=N)] + rng.standard_normal((N, d)).astype(np.float32)).astype(np.float32)
    soft, model = ptree.assign(cells, far, 1.0, responsibilities=True), pm.assign(cells, far, 1.0)
    assert np.array_equal(np.sort(soft.resp, axis=1)[:, :-1], np.zeros((N, R - 1)))
    assert np.array_equal(soft.resp.max(axis=1), np.ones(N)) and _same_bits(soft.free_energy, model.free_energy)
    assert _same_bits(soft.gamma, model.gamma) and _same_bits(soft.sums, model.sums)


# ------------------------------------------------------------------------------------------------------ the soft pass

@pytest.mark.parametrize("d", (1, 3, 17, 50, 128))
def test_soft_pass_within_the_derived_bound(d):
    from prosstt_amd import ptree
    rng = np.random.default_rng(4200 + d)
    for N, R in ((1, 1), (65, 2), (257, 63), (64, 64), (1030, 65), (63, 130), (257, 400)):
        Y = rng.standard_normal((N, d)).astype(np.float32)
        C = rng.standard_normal((R, d)).astype(np.float32)
        hard = pm.assign(Y, C, 0.0)
        for sigma in (max(float(hard.sq_distance.mean()), 1e-3), 0.05 * d):
            want = pm.assign(Y, C, sigma)
            got = ptree.assign(_view(Y, "wide"), _view(C, "shifted"), sigma, responsibilities=True)
            worst = _assert_soft(got, want, Y, C, sigma, (N, R, d, sigma))
            assert np.all(got.resp.sum(axis=1) >= 1 - 1e-12) and np.all(np.isfinite(got.free_energy))
    print("soft pass, d = %d: the largest error over its bound %s" % (d, worst))


@pytest.mark.parametrize("R", (1, 2, 64, 128, 256))
def test_equal_distances_give_the_soft_sums_bit_for_bit(R):
    """Every centre is the same point: w = exp(-0) = 1, Z = R, r = 1 / R exactly."""
    from prosstt_amd import ptree
    rng = np.random.default_rng(R)
    N, d = 300, 7
    Y = rng.standard_normal((N, d)).astype(np.float32)
    C = np.repeat(rng.standard_normal((1, d)).astype(np.float32), R, axis=0)
    want, got = pm.assign(Y, C, 0.7), ptree.assign(Y, C, 0.7, responsibilities=True)
    assert np.all(got.resp == 1.0 / R) and not got.best.any()
    assert _same_bits(got.resp, want.resp) and _same_bits(got.gamma, want.gamma) and _same_bits(got.sums, want.sums)
    assert np.all(got.gamma == N / R)
    assert np.all(np.abs(got.free_energy - want.free_energy) <= pm.soft_bound(Y, C, 0.7, want)[0])


@pytest.mark.parametrize("d", (8, 9, 17, 32, 33, 65))
def test_equal_distances_give_the_soft_sums_bit_for_bit_for_every_q(d):
    """The same for every ptree_sums_kernel<Q, false>: d = 8 -> Q = 1, 9 -> 2, 17 and 32 -> 4, 33 -> 8, 65 -> 16 (the hard pass
    reaches every <Q, true> through DS above); two chunks of cells and a ragged one, two blocks of nodes; R is a power of two,
    so that every product r * y is exact and the sums are IEEE in the header's order."""
    from prosstt_amd import ptree
    rng = np.random.default_rng(900 + d)
    N, R = 300, 64
    Y = rng.standard_normal((N, d)).astype(np.float32)
    C = np.repeat(rng.standard_normal((1, d)).astype(np.float32), R, axis=0)
    want, got = pm.assign(Y, C, 0.7), ptree.assign(_view(Y, "shifted"), C, 0.7, responsibilities=True)
    assert np.all(got.resp == 1.0 / R) and not got.best.any()
    assert _same_bits(got.resp, want.resp) and _same_bits(got.gamma, want.gamma) and _same_bits(got.sums, want.sums)


# ------------------------------------------------------------------------------------------------------ the same bits

def _fixed_inputs():
    rng = np.random.default_rng(77)
    N, R, d = 777, 130, 15
    return rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((R, d)).astype(np.float32)


def test_same_bits_twice_on_a_second_stream_with_and_without_resp_and_for_device_inputs():
    import torch
    from prosstt_amd import ptree
    Y, C = _fixed_inputs()
    edges = ptree.spanning_tree(C)
    for sigma in (0.0, 9.0):
        base = ptree.assign(Y, C, sigma, responsibilities=True)
        assert _bytes(ptree.assign(Y, C, sigma, responsibilities=True)) == _bytes(base)
        bare = ptree.assign(Y, C, sigma)
        assert bare.resp is None and _bytes(bare) == _bytes(base[:5])
        Yd, Cd = torch.from_numpy(Y).cuda(), torch.from_numpy(C).cuda()
        on_device = ptree.assign(Yd, Cd, sigma, responsibilities=True, out="torch")
        assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in on_device)
        assert _bytes(on_device) == _bytes(base)
        assert _bytes(ptree.assign(Yd.double(), Cd.double(), sigma, responsibilities=True)) == _bytes(base)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            other = ptree.assign(Yd, Cd, sigma, responsibilities=True)
        stream.synchronize()
        assert _bytes(other) == _bytes(base)
    p = ptree.project(Y, C, edges)
    with torch.cuda.stream(stream):
        q = ptree.project(Yd, Cd, edges, out="torch")
    stream.synchronize()
    assert _bytes(q) == _bytes(p) == _bytes(ptree.project(Y, C, edges))


def calls_ptree(place=lambda value: value):
    """The library's label and its calls over ``_fixed_inputs``: the host arrays, and device views that ``place`` puts
    (tests/test_gpu_stale_memory.py)."""
    from prosstt_amd import ptree
    Y, C = _fixed_inputs()
    edges = ptree.spanning_tree(C)
    Yv, Cv = place(_view(Y, "shifted")), place(_view(C, "wide"))
    return "ptree", {
        "assign, hard": lambda: ptree.assign(Y, C, 0.0, responsibilities=True),
        "assign, soft": lambda: ptree.assign(Y, C, 9.0, responsibilities=True),
        "project": lambda: ptree.project(Y, C, edges),
        "assign, hard, device views": lambda: ptree.assign(Yv, Cv, 0.0, responsibilities=True, out="torch"),
        "assign, soft, device views": lambda: ptree.assign(Yv, Cv, 9.0),
        "project, device views": lambda: ptree.project(Yv, Cv, edges),
    }


def test_same_bits_over_stale_memory():
    import stale
    _, calls = calls_ptree()
    base = [_bytes(call()) for call in calls.values()]
    assert base[3] == base[0] and base[4] == base[1][:5] and base[5] == base[2]
    for byte in stale.BYTES:
        with stale.poisoned(byte) as state:
            got = [_bytes(call()) for call in calls.values()]
        assert got == base and state.fills > 0, byte


def test_per_cell_outputs_of_any_subset_or_permutation_of_the_rows():
    from prosstt_amd import ptree
    Y, C = _fixed_inputs()
    rng = np.random.default_rng(3)
    edges = ptree.spanning_tree(C)
    for sigma in (0.0, 9.0):
        whole = ptree.assign(Y, C, sigma, responsibilities=True)
        for rows in (rng.permutation(len(Y)), np.sort(rng.choice(len(Y), size=129, replace=False)), np.array([5]),
                     np.arange(100, 400)):
            part = ptree.assign(Y[rows], C, sigma, responsibilities=True)
            for a, b in ((part.best, whole.best), (part.sq_distance, whole.sq_distance),
                         (part.free_energy, whole.free_energy), (part.resp, whole.resp)):
                assert _same_bits(a, b[rows]), (sigma, len(rows))
        chunks = ptree.Assignment.concat(ptree.assign(Y[lo:lo + 300], C, sigma, responsibilities=True)
                                         for lo in range(0, len(Y), 300))
        assert _bytes(chunks[:3]) == _bytes(whole[:3]) and _same_bits(chunks.resp, whole.resp)
        np.testing.assert_allclose(chunks.gamma, whole.gamma, rtol=1e-12)
        np.testing.assert_allclose(chunks.sums, whole.sums, rtol=0, atol=1e-10)
    whole = ptree.project(Y, C, edges)
    rows = rng.permutation(len(Y))[:300]
    assert _bytes(ptree.project(Y[rows], C, edges)) == _bytes([a[rows] for a in whole])


def test_status_word_names_a_non_finite_value_in_a_device_tensor():
    import torch
    from prosstt_amd import ptree
    Y, C = _fixed_inputs()
    Yd, Cd = torch.from_numpy(Y).cuda(), torch.from_numpy(C).cuda()
    edges = ptree.spanning_tree(C)
    for row, col, value in ((0, 0, float("nan")), (776, 14, float("inf")), (300, 7, float("-inf"))):
        bad = Yd.clone()
        bad[row, col] = value
        for sigma in (0.0, 2.0):
            with pytest.raises(ValueError, match="NONFINITE"):
                ptree.assign(bad, Cd, sigma)
        with pytest.raises(ValueError, match="NONFINITE"):
            ptree.project(bad, Cd, edges)
    bad = Cd.clone()
    bad[129, 14] = float("nan")
    with pytest.raises(ValueError, match="NONFINITE"):
        ptree.assign(Yd, bad, 0.0)
    with pytest.raises(ValueError, match="NONFINITE"):
        ptree.project(Yd, bad, edges)


from test_gpu_far_offsets import arena  # noqa: E402,F401  (the 19 GiB buffer, allocated for this module's one case)


def test_rows_2_to_the_24_plus_4_elements_apart(arena):  # noqa: F811
    import test_gpu_far_offsets as far
    from prosstt_amd import ptree
    rng = np.random.default_rng(31)
    N, d, R = far.N, 50, 65
    Y = rng.standard_normal((N, d)).astype(np.float32)
    C = rng.standard_normal((R, d)).astype(np.float32)
    edges = ptree.spanning_tree(C)
    for name, (stride, _, shift) in sorted(far.PATHS.items()):
        view = far._far(arena, Y, stride, shift)
        for sigma in (0.0, 40.0):
            near = ptree.assign(_view(Y, "wide"), C, sigma, responsibilities=True)
            assert _bytes(ptree.assign(view, C, sigma, responsibilities=True)) == _bytes(near), (name, sigma)
        _assert_hard(ptree.assign(view, C, 0.0), pm.assign(Y, C, 0.0), name)
        assert _bytes(ptree.project(view, C, edges)) == _bytes(pm.project(Y, C, edges)), name


# ------------------------------------------------------------------------------------------------------ step by step

def test_the_fit_step_by_step_against_the_model():
    """512 cells on three branches in 10 dimensions, 30 nodes: in every iteration the device pass is fed the model's centres of
    the iteration before; it meets the bound, and its centre step gives the model's spanning tree wherever that tree is clear
    of the difference between the two distance matrices."""
    from prosstt_amd import ptree
    Y, _, _ = pm.three_branches(512, 10, 12)
    N, R = 512, 30
    C = ptree.lloyd(Y, pm.initial_centres(Y, R, 0), lambda c: pm.assign(Y, c, 0.0, False), ptree.KMEANS_ITER).centres
    sigma = float(np.mean(pm.assign(Y, C, 0.0, False).sq_distance.astype(np.float64)))
    lam = ptree.LAM * N / R
    clear = 0
    for it in range(12):
        want = pm.assign(Y, C, sigma)
        got = ptree.assign(Y, C, sigma, responsibilities=True)
        _assert_soft(got, want, Y, C, sigma, it)
        edges = ptree.spanning_tree(C)
        e_model, e_device = ptree.energy(want.free_energy, C, edges, lam), ptree.energy(got.free_energy, C, edges, lam)
        assert abs(e_model - e_device) <= pm.soft_bound(Y, C, sigma, want)[0].sum() * (1 + 1e-9)
        C_model = ptree.centre_step(want.gamma, want.sums, edges, lam, C)
        C_device = ptree.centre_step(got.gamma, got.sums, edges, lam, C)
        D_model, D_device = ptree.centre_distances(C_model), ptree.centre_distances(C_device)
        if pm.prim_margin(D_model) > 2 * np.max(np.abs(D_model - D_device)):
            clear += 1
            assert np.array_equal(ptree.prim(D_device), ptree.prim(D_model)), it
        C = C_model
    assert clear >= 10                                                       # (the rule was not vacuous)
    print("spanning tree clear of the bound in %d of 12 iterations" % clear)


def test_kmeans_gives_the_models_labels_in_each_iteration():
    from prosstt_amd import ptree
    Y, _, _ = pm.three_branches(512, 10, 13)
    C = pm.initial_centres(Y, 30, 4)
    for it in range(8):
        want, got = pm.assign(Y, C, 0.0, False), ptree.assign(Y, C, 0.0)
        _assert_hard(got, want, it)
        new = C.copy()
        full = want.gamma > 0
        new[full] = (want.sums[full] / want.gamma[full, None]).astype(np.float32)
        C = new
    for n_iter in (0, 1, 5, 100):
        km, model = ptree.kmeans(Y, 30, n_iter=n_iter, seed=4), pm.kmeans(Y, 30, n_iter=n_iter, seed=4)
        assert np.array_equal(km.labels, model.labels) and _same_bits(km.centres, model.centres)
        assert km.inertia == model.inertia and km.n_iter == model.n_iter and km.converged == model.converged
    assert km.converged and km.labels.dtype == np.int32
    fit, model = ptree.principal_tree(Y, 30, seed=4, n_iter=5), pm.principal_tree(Y, 30, seed=4, n_iter=5)
    assert fit.n_iter == 5 and fit.energy.shape == (6,) and fit.edges.shape == (29, 2)
    np.testing.assert_allclose(fit.energy, model[2], rtol=1e-9)
    assert fit.responsibilities().shape == (512, 30) and fit.project().edge.shape == (512,)


# ---------------------------------------------------------------------------------------------------------- the loop

# What the numpy model reaches on numpy-drawn matrices, measured without the code under test (DESIGN section 28 has the
# protocol and the same figures beside the device's): as (mean, standard deviation over the seeds, ddof 1).  The floor of the
# test is the mean minus SIGMAS standard deviations.
from ptree_quality import BRANCH_ACCURACY, N_COMPONENTS, SPEARMAN, branch_accuracy, spearman  # noqa: E402

SIGMAS = 5.0


def test_the_loop_from_a_bare_count_matrix_to_a_tree_and_a_second_simulation():
    from test_gpu_trends import _simulation
    from prosstt_amd import embed, fit, ptree, simulation as sim, trends
    t, X, pt, br, sc = _simulation()
    p = embed.pca(X, sc, N_COMPONENTS)
    tree = ptree.principal_tree(p.scores)
    assert tree.centres.shape == (ptree.N_NODES, N_COMPONENTS) and tree.best.shape == (3000,)
    assert np.all(np.diff(tree.energy) <= 1e-6 * np.abs(tree.energy[1:]))
    lf = tree.to_tree(root=int(np.argmin(pt)), G=300)
    new = lf.tree
    new._check_topology()
    children = {}
    for parent, child in new.topology:
        children.setdefault(parent, []).append(child)
    assert len(new.branches) == 3 and list(children) == [new.root] and len(children[new.root]) == 2, new.topology
    # the fields fit the tree and the libraries downstream
    bt = new.branch_times()
    first = np.array([bt[b][0] for b in lf.branches])
    last = np.array([bt[b][1] for b in lf.branches])
    assert np.all((lf.pseudotime >= first) & (lf.pseudotime <= last)) and lf.pseudotime.dtype == np.int64
    assert np.array_equal(sim.cell_rows(new, lf.pseudotime, lf.branches), lf.node) and lf.node.dtype == np.int32
    assert abs(sum(float(np.sum(new.density[b])) for b in new.branches) - 1.0) <= 1e-12
    accuracy, rho = branch_accuracy(lf.branches, br), spearman(lf.position, pt)
    print("principal_tree on smoke()'s tree: %d of %d nodes kept, times %s, branch accuracy %.4f, Spearman %.4f"
          % (len(lf.kept), ptree.N_NODES, dict(new.time), accuracy, rho))
    tr = trends.expression_trends(X, sc, new, lf.pseudotime, lf.branches, bandwidth=3.0)
    assert np.array_equal(tr.labels, lf.node) and tr.means.shape == (len(lf.kept), 300)
    f = fit.count_model(X, sc, lf.node, tr.means)
    host = X.cpu().numpy()
    has_counts = host.sum(axis=0) > 0
    assert np.all(np.isfinite(f.alpha[has_counts])) and np.all(np.isfinite(f.beta[has_counts]))
    again = sim.sample_density(tr.to_tree(), 500, alpha=0.2, beta=2.0, seed=5)
    assert np.asarray(again[0]).shape == (500, 300)
    assert accuracy >= BRANCH_ACCURACY[0] - SIGMAS * BRANCH_ACCURACY[1]
    assert rho >= SPEARMAN[0] - SIGMAS * SPEARMAN[1]
