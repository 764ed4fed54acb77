"""-m gpu: prosstt_amd.mapping on the device against tests/mapping_model.py.  Exact cases (dyadic panels, small counts: every
product and partial sum is exact in binary32) bit for bit on every path of the pass: every node tile, whole and ragged tiles of
cells, genes and nodes, every chain length, aligned rows, a row stride of G + 1 and a view one element off; the same bits for
the same call twice, on a second stream, with and without the scores, for a presented matrix, for any subset of rows and over
stale memory; the derived tolerance and the argmax rule on random counts, counts of 2^24 and more among them; ties; the
guards; rows beyond element 2^31; and the loop from a simulation's counts to positions on its tree and on to trends and fit."""
import ctypes
import functools

import numpy as np
import pytest

import mapping_model as mm

pytestmark = pytest.mark.gpu

INT_MAX = 2 ** 31 - 1
NS = (1, 31, 33, 133)
GS = (1, 31, 33, 255, 256, 257, 300)
RS = (1, 31, 33, 60, 129)                 # one and two 32-node tiles whole and ragged; several blocks of nodes at 129
CHAINS = (32, 256, 512)
LAYOUTS = ("aligned", "wide", "shifted")


def _view(host, layout):
    """The host matrix on the device: "aligned" (base on 16 bytes, a row stride that is a multiple of 4: the 16-byte loads),
    "wide" (a row stride of G + 1), "shifted" (the view starts one element in)."""
    import torch
    N, G = host.shape
    ld, shift = {"aligned": (-(-G // 4) * 4, 0), "wide": (G + 1, 0), "shifted": (G + 4, 1)}[layout]
    wide = torch.full((N, ld), 12345, dtype=torch.int32, device="cuda")
    wide[:, shift:shift + G] = torch.from_numpy(np.array(host)).cuda()
    view = wide[:, shift:shift + G]
    assert view.data_ptr() % 16 == 4 * shift and (N == 1 or view.stride(0) == ld)
    return view


def _exact_inputs(N, G, R, rng):
    """Counts below 64, panel entries k / 8 with k in -2 .. 2: every product and partial sum of up to 300 genes is a multiple
    of 1 / 8 below 2^24 / 8, exact in binary32 in any order."""
    X = (rng.integers(0, 64, size=(N, G)) * (rng.random((N, G)) < 0.5)).astype(np.int32)
    P = (rng.integers(-2, 3, size=(R, G)) / 8.0).astype(np.float32)
    s = rng.lognormal(0.0, 0.7, N)
    m = rng.standard_normal(R) * 20.0
    c = rng.standard_normal(R)
    return X, s, P, m, c


def _offsets(R, rng):
    """Branches of the R nodes: one node, none, and the rest in two."""
    if R == 1:
        return np.array([0, 1, 1], dtype=np.int64)
    cut = int(rng.integers(1, R))
    return np.array([0, 1, 1, cut, R], dtype=np.int64)


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


def _assert_against_model(got, X, s, P, m, c, offsets, chain, what, exact):
    S = mm.scores(X, s, P, m, c)
    b = mm.bound(X, s, P, m, c, chain)
    if exact:
        assert _same_bits(got.scores, S), what
        assert np.array_equal(got.best, mm.best(S)), what
        assert _same_bits(got.best_score, S[np.arange(len(S)), got.best]), what
    else:
        assert np.all(np.abs(got.scores - S) <= b), (what, float(np.max(np.abs(got.scores - S) / b)))
        assert _same_bits(got.best_score, got.scores[np.arange(len(S)), got.best]), what
    share = mm.check_argmax(S, b, got.best)
    want = mm.lse(S)
    assert np.all(np.abs(got.lse - want) <= mm.lse_bound(b, want)), what
    want_b = mm.branch_lse(S, offsets)
    empty = np.diff(offsets) == 0
    assert np.all(np.isneginf(got.branch_lse[:, empty])), what
    for k in np.flatnonzero(~empty):
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        assert np.all(np.abs(got.branch_lse[:, k] - want_b[:, k]) <= mm.lse_bound(b[:, lo:hi], want_b[:, k])), (what, k)
    return share


# ------------------------------------------------------------------------------------------------------ exact cases

@pytest.mark.parametrize("G", GS)
def test_exact_scores_bit_for_bit_on_every_path(G):
    from prosstt_amd import mapping
    rng = np.random.default_rng(7000 + G)
    for N in NS:
        for R in RS:
            X, s, P, m, c = _exact_inputs(N, G, R, rng)
            offsets = _offsets(R, rng)
            views = {layout: _view(X, layout) for layout in LAYOUTS}
            base = None
            for chain in CHAINS:
                got = mapping.node_scores(views["aligned"], s, P, m, c, offsets, genes_per_chain=chain, scores=True)
                assert got.best.dtype == np.int32 and got.scores.shape == (N, R) and got.branch_lse.shape == (N, len(offsets) - 1)
                _assert_against_model(got, X, s, P, m, c, offsets, chain, (N, G, R, chain), exact=True)
                if base is None:
                    base = got
                assert _bytes(got) == _bytes(base), (N, G, R, chain)         # exact sums: the chain length changes no bit
            for layout in LAYOUTS[1:]:
                other = mapping.node_scores(views[layout], s, P, m, c, offsets, scores=True)
                assert _bytes(other) == _bytes(base), (N, G, R, layout)
            for tile in (1, 2, 3, 4):
                layout = LAYOUTS[tile % 3]
                other = mapping.node_scores(views[layout], s, P, m, c, offsets, scores=True, node_tile=tile, genes_per_chain=32)
                assert _bytes(other) == _bytes(base), (N, G, R, "node_tile", tile)


def test_an_all_zero_matrix_gives_the_constants_minus_the_exposures():
    import torch
    from prosstt_amd import mapping
    rng = np.random.default_rng(1)
    N, G, R = 133, 257, 60
    P = rng.standard_normal((R, G)).astype(np.float32)
    s, m, c = rng.lognormal(0.0, 0.7, N), rng.standard_normal(R) * 30, rng.standard_normal(R)
    got = mapping.node_scores(torch.zeros((N, G), dtype=torch.int32, device="cuda"), s, P, m, c, scores=True)
    assert _same_bits(got.scores, (0.0 - s[:, None] * m[None, :]) + c[None, :])
    assert np.array_equal(got.best, mm.best(got.scores))
    none = mapping.node_scores(torch.zeros((N, G), dtype=torch.int32, device="cuda"), None, P, np.zeros(R), scores=True)
    assert not none.scores.any() and not none.best.any()
    np.testing.assert_allclose(none.lse, np.log(float(R)), rtol=1e-15)


# ------------------------------------------------------------------------------------------------------ random counts

def tree_inputs(per_branch, G, N, seed, step=0.12):
    """A bifurcation of three branches of ``per_branch`` nodes, in numpy alone: log-means that walk along every branch from
    where its parent ended (steps of standard deviation ``step`` in a fifth of the genes per branch), base levels spread
    over three decades, cells drawn at uniform nodes with log-normal size factors, negative-binomial counts of the count
    model with alpha = 0.2 and beta = 2.  Returns (X int32, s, means (3 per_branch, G), the true node of every cell)."""
    rng = np.random.default_rng(seed)
    base = np.exp(rng.normal(0.5, 1.5, G))
    walks = {}
    for b, parent in (("A", None), ("B", "A"), ("C", "A")):
        active = rng.random(G) < 0.2
        steps = rng.normal(0.0, step, size=(per_branch, G)) * active[None, :]
        start = walks[parent][-1] if parent else np.zeros(G)
        walks[b] = start[None, :] + np.cumsum(steps, axis=0)
    means = np.concatenate([np.exp(walks[b]) for b in "ABC"]) * base[None, :]
    node = rng.integers(0, means.shape[0], N)
    s = rng.lognormal(0.0, 0.7, N)
    mu = s[:, None] * means[node]
    X = rng.negative_binomial(mu / (0.2 * mu + 1.0), 1.0 / (0.2 * mu + 2.0)).astype(np.int32)
    return X, s, means, node


# (nodes per branch, G, N): at least MARGIN_SHARE of the cells of each must have a best node that is clear of the bounds
NAMED = ((20, 300, 512), (20, 1100, 512), (20, 300, 3000), (20, 1100, 3000), (7, 1100, 512), (7, 1100, 3000))
MARGIN_SHARE = 0.85


@functools.lru_cache(maxsize=None)
def _named(per_branch, G, N):
    X, s, means, node = tree_inputs(per_branch, G, N, 1000 * per_branch + G + N)
    for a in (X, s, means):
        a.setflags(write=False)
    return X, s, means, node


@pytest.mark.parametrize("per_branch, G, N", NAMED)
def test_tolerance_and_argmax_rule_on_random_counts(per_branch, G, N):
    from prosstt_amd import mapping
    X, s, means, _ = _named(per_branch, G, N)
    P, m = mapping.poisson_panel(means)
    R = 3 * per_branch
    offsets = np.array([0, per_branch, 2 * per_branch, R], dtype=np.int64)
    c = np.log(np.random.default_rng(3).dirichlet(np.full(R, 5.0)))
    view = _view(X, "aligned" if N == 512 else "shifted")
    for chain in (64, 256, 1024):
        got = mapping.node_scores(view, s, P, m, c, offsets, genes_per_chain=chain, scores=True)
        share = _assert_against_model(got, X, s, P, m, c, offsets, chain, (per_branch, G, N, chain), exact=False)
        print("3 x %d nodes, G = %d, N = %d, chain %d: %.1f %% of the cells have a clear best node" % (per_branch, G, N, chain,
                                                                                                     100 * share))
        if chain == 256:
            assert share >= MARGIN_SHARE


def test_counts_of_2_to_the_24_and_more():
    """Counts that binary32 cannot hold round once; the bound's second unit covers it."""
    from prosstt_amd import mapping
    X, s, means, _ = _named(7, 1100, 512)
    X = np.array(X)
    rng = np.random.default_rng(24)
    at = (rng.integers(0, 512, 40), rng.integers(0, 1100, 40))
    X[at] = rng.integers(2 ** 24, 2 ** 31 - 1, 40)
    X[5, 1099] = INT_MAX
    X[6, 0] = 2 ** 24 + 1
    P, m = mapping.poisson_panel(means)
    offsets = np.array([0, 7, 14, 21], dtype=np.int64)
    for layout, chain in (("aligned", 256), ("wide", 32), ("shifted", 4096)):
        got = mapping.node_scores(_view(X, layout), s, P, m, None, offsets, genes_per_chain=chain, scores=True)
        _assert_against_model(got, X, s, P, m, None, offsets, chain, (layout, chain), exact=False)


# ------------------------------------------------------------------------------------------------------ the same bits

@functools.lru_cache(maxsize=None)
def _case():
    """N = 133, G = 300, R = 129 (two node tiles), random counts and a random panel: sums that round."""
    rng = np.random.default_rng(133 * 300)
    X = rng.poisson(3.0, size=(133, 300)).astype(np.int32) * (rng.random((133, 300)) < 0.4)
    X = X.astype(np.int32)
    P = rng.standard_normal((129, 300)).astype(np.float32)
    s = rng.lognormal(0.0, 0.7, 133)
    m, c = rng.standard_normal(129) * 20.0, rng.standard_normal(129)
    offsets = np.array([0, 40, 41, 129], dtype=np.int64)
    for a in (X, P, s, m, c, offsets):
        a.setflags(write=False)
    return X, s, P, m, c, offsets


def test_the_same_bits_twice_on_a_second_stream_without_scores_presented_and_for_subsets_of_rows():
    import torch
    from prosstt_amd import device, mapping
    X, s, P, m, c, offsets = _case()
    view = _view(X, "aligned")
    base = mapping.node_scores(view, s, P, m, c, offsets, scores=True)
    _assert_against_model(base, X, s, P, m, c, offsets, 256, "the case", exact=False)
    assert _bytes(mapping.node_scores(view, s, P, m, c, offsets, scores=True)) == _bytes(base)
    assert _bytes(mapping.node_scores(view, s, P, m, c, offsets)) == _bytes(base)[:4]            # S in the workspace
    on_device = mapping.node_scores(view, torch.from_numpy(np.array(s)).cuda(), torch.from_numpy(np.array(P)).cuda(), m, c,
                                    offsets, scores=True, out="torch")
    assert on_device.scores.is_cuda and _bytes(on_device) == _bytes(base)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = mapping.node_scores(_view(X, "shifted"), s, P, m, c, offsets, scores=True, node_tile=3)
    stream.synchronize()
    assert _bytes(other) == _bytes(base)
    # rows are independent: any subset of rows against the whole call (what a matrix in chunks of cells relies on)
    rng = np.random.default_rng(9)
    for rows in (np.array([132]), np.arange(31, 64), np.sort(rng.choice(133, 57, replace=False)), rng.permutation(133)):
        part = mapping.node_scores(_view(np.array(X)[rows], "wide"), np.array(s)[rows], P, m, c, offsets, scores=True)
        assert _bytes(part) == _bytes([a[rows] for a in base]), rows[:4]
    # a presented matrix against its plan-order matrix: row i holds cell perm[i]; s is per cell
    perm = rng.permutation(133)
    presented = device.PresentedCounts(_view(np.ascontiguousarray(np.array(X)[perm]), "aligned"), perm)
    assert _bytes(mapping.node_scores(presented, s, P, m, c, offsets, scores=True)) == _bytes(base)
    assert _bytes(mapping.node_scores(presented, s, P, m, c, offsets, scores=True, out="torch")) == _bytes(base)
    assert _bytes(mapping.node_scores(presented.in_plan_order(), s, P, m, c, offsets, scores=True)) == _bytes(base)


def calls_mapping(place=lambda value: value):
    """The library's label and its calls over ``_case``; ``place`` puts the device inputs (tests/test_gpu_stale_memory.py)."""
    from prosstt_amd import mapping
    X, s, P, m, c, offsets = _case()
    shifted, aligned = place(_view(X, "shifted")), place(_view(X, "aligned"))
    return "mapping", {
        "node_scores": lambda: mapping.node_scores(shifted, s, P, m, c, offsets),
        "node_scores with scores, out='torch'": lambda: mapping.node_scores(aligned, s, P, m, c, offsets, scores=True,
                                                                             out="torch", genes_per_chain=32),
    }


def test_no_result_depends_on_stale_memory():
    from test_gpu_stale_memory import _thrice
    _thrice(*calls_mapping())


# ------------------------------------------------------------------------------------------------------ ties

def test_ties_go_to_the_lower_node_and_a_branch_of_one_node_is_its_score():
    from prosstt_amd import mapping
    X, s, P, m, c, _ = _case()
    P, m, c = np.array(P), np.array(m), np.array(c)
    # every node from 64 on repeats a node below 64 (other lanes of the finish kernel, the second node tile of the pass)
    source = np.random.default_rng(4).integers(0, 64, 65)
    P[64:], m[64:], c[64:] = P[source], m[source], c[source]
    offsets = np.array([0, 1, 64, 65, 129], dtype=np.int64)
    got = mapping.node_scores(_view(X, "aligned"), s, P, m, c, offsets, scores=True)
    assert np.array_equal(got.scores[:, 64:], got.scores[:, source])
    assert got.best.max() < 64 and np.array_equal(got.best, mm.best(got.scores))
    assert _same_bits(got.branch_lse[:, 0], got.scores[:, 0]) and _same_bits(got.branch_lse[:, 2], got.scores[:, 64])
    # all nodes equal: node 0, and lse = score + log R
    flat = mapping.node_scores(_view(X, "aligned"), s, np.repeat(P[:1], 129, axis=0), np.zeros(129), None, offsets, scores=True)
    assert not flat.best.any()
    np.testing.assert_allclose(flat.lse, flat.best_score + np.log(129.0), rtol=1e-15, atol=1e-12)


# ------------------------------------------------------------------------------------------------------ guards

def test_a_negative_count_raises():
    from prosstt_amd import device, mapping
    X, s, P, m, c, offsets = _case()
    for layout, where in (("aligned", (132, 299)), ("shifted", (0, 0)), ("wide", (64, 257))):
        neg = np.array(X)
        neg[where] = -3
        with pytest.raises(ValueError, match=r"status bit NEGATIVE \(1\): %s" % device.NEGATIVE_ENTRY):
            mapping.node_scores(_view(neg, layout), s, P, m, c, offsets)
        assert mapping._node_scores(_view(neg, layout), s, P, m, c, offsets)[1] == mapping.NEGATIVE


def _abi_call(L, X, s, P, m, c, offsets, B, chain, ws, out, *, N=None, G=None, ld=None, ldp=None, R=None, ws_bytes=None,
              tile=0):
    import torch
    best, best_score, lse, branch_lse, scores, status = out
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    return L.prosstt_amd_mapping_node_scores_tiled(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(X), X.shape[0] if N is None else N,
        X.shape[1] if G is None else G, X.stride(0) if ld is None else ld, ptr(s), ptr(P), P.stride(0) if ldp is None else ldp,
        P.shape[0] if R is None else R, ptr(m), ptr(c), ptr(offsets), B, chain, tile, ptr(ws),
        ws.numel() if ws_bytes is None else ws_bytes, ptr(best), ptr(best_score), ptr(lse), ptr(branch_lse), ptr(scores),
        ptr(status))


def test_the_c_abi_clamps_offsets_that_do_not_ascend_and_refuses_bad_arguments():
    import torch
    from prosstt_amd import _native, mapping
    L = _native.load("mapping")
    Xh, sh, Ph, mh, ch, _ = _case()
    N, G, R, B = 133, 300, 129, 3
    X, s, P, m, c = (torch.from_numpy(np.array(a)).cuda() for a in (Xh, sh, Ph, mh, ch))
    need = ctypes.c_uint64(0)
    assert L.prosstt_amd_mapping_workspace_bytes(N, G, R, B, ctypes.byref(need)) == 0 and need.value >= N * R * 8
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")

    def outputs():
        return (torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.float64, device="cuda"),
                torch.empty(N, dtype=torch.float64, device="cuda"), torch.empty((N, B), dtype=torch.float64, device="cuda"),
                torch.empty((N, R), dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"))

    good = torch.tensor([0, 40, 41, 129], dtype=torch.int64, device="cuda")
    out = outputs()
    assert _abi_call(L, X, s, P, m, c, good, B, 256, ws, out) == 0
    torch.cuda.synchronize()
    assert int(out[5].item()) == 0
    want = mapping.node_scores(X, sh, Ph, mh, ch, np.array([0, 40, 41, 129]), scores=True)
    assert _bytes([t for t in out[:5]]) == _bytes(want)
    # crooked offsets in device memory: reported, clamped into [0, R], nothing read out of bounds
    S, b = mm.scores(Xh, sh, Ph, mh, ch), mm.bound(Xh, sh, Ph, mh, ch, 256)
    for crooked, spans in (([0, 50, 41, 129], [(0, 50), (50, 50), (41, 129)]), ([0, 40, 41, 1 << 40], [(0, 40), (40, 41), (41, 129)]),
                           ([-5, 40, 41, 129], [(0, 40), (40, 41), (41, 129)]), ([0, 40, 41, 100], [(0, 40), (40, 41), (41, 100)]),
                           ([7, -(1 << 62), 1 << 62, 129], [(7, 7), (0, 129), (129, 129)])):
        out = outputs()
        assert _abi_call(L, X, s, P, m, c, torch.tensor(crooked, dtype=torch.int64, device="cuda"), B, 256, ws, out) == 0
        torch.cuda.synchronize()
        assert int(out[5].item()) == mapping.BRANCH_RANGE, crooked
        assert _bytes(out[:3]) == _bytes(want[:3])
        got = out[3].cpu().numpy()
        for k, (lo, hi) in enumerate(spans):
            if hi == lo:
                assert np.all(np.isneginf(got[:, k])), (crooked, k)
            else:
                span = mm.lse(S, lo, hi)
                assert np.all(np.abs(got[:, k] - span) <= mm.lse_bound(b[:, lo:hi], span)), (crooked, k)
    # refusals: nothing is enqueued
    out = outputs()
    refusals = [
        (dict(N=0), "1 <= N < 2\\^31"), (dict(G=0), "1 <= G < 2\\^31"), (dict(R=0), "nodes"), (dict(R=65535 * 32 + 1), "nodes"),
        (dict(ld=G - 1), "row stride 299 is below the row length 300"), (dict(ldp=G - 1), "panel stride 299 is below"),
        (dict(ws_bytes=need.value - 1), "workspace of %d bytes, %d needed" % (need.value - 1, need.value)), (dict(tile=5), "node_tile"),
    ]
    for change, match in refusals:
        assert _abi_call(L, X, s, P, m, c, good, B, 256, ws, out, **change) == _native.EINVAL, change
        assert __import__("re").search(match, L.prosstt_amd_mapping_last_error().decode()), (change, L.prosstt_amd_mapping_last_error())
    for chain in (0, 16, 48, 4128, -32):
        assert _abi_call(L, X, s, P, m, c, good, B, chain, ws, out) == _native.EINVAL
        assert "genes_per_chain" in L.prosstt_amd_mapping_last_error().decode()
    assert _abi_call(L, X, s, P, m, c, good, 0, 256, ws, out) == _native.EINVAL          # branch_lse without branches
    assert _abi_call(L, X, s, P, m, c, None, B, 256, ws, out) == _native.EINVAL          # ... without offsets
    assert _abi_call(L, X, s, P, m, c, good, B, 256, ws[1:], out, ws_bytes=need.value) == _native.EINVAL
    assert "16-byte aligned" in L.prosstt_amd_mapping_last_error().decode()
    # neither branch_lse nor scores: B and the offsets are not looked at
    out = outputs()
    bare = out[:3] + (None, None, out[5])
    assert _abi_call(L, X, s, P, m, c, None, 0, 256, ws, bare) == 0
    torch.cuda.synchronize()
    assert _bytes(out[:3]) == _bytes(want[:3]) and int(out[5].item()) == 0


# ------------------------------------------------------------------------------------------------------ far offsets

from test_gpu_far_offsets import arena  # noqa: E402,F401  (the 19 GiB buffer, allocated for this module's one case)


def test_rows_2_to_the_24_plus_4_elements_apart(arena):  # noqa: F811
    import test_gpu_far_offsets as far
    from prosstt_amd import mapping
    X = far._inputs()["X"]                            # 161 x 1029, INT_MAX among the counts
    stride, near_stride, shift = far.PATHS["vector"]
    rng = np.random.default_rng(31)
    P = rng.standard_normal((33, far.G)).astype(np.float32)
    s, m, c = far._inputs()["s"], rng.standard_normal(33), rng.standard_normal(33)
    offsets = np.array([0, 10, 33], dtype=np.int64)
    near = mapping.node_scores(far._near(X, near_stride, shift), s, P, m, c, offsets, scores=True)
    _assert_against_model(near, np.array(X), s, P, m, c, offsets, 256, "the near view", exact=False)
    got = mapping.node_scores(far._far(arena, X, stride, shift), s, P, m, c, offsets, scores=True)
    assert _bytes(got) == _bytes(near)


# ---------------------------------------------------------------------------------------------------------- the loop

# What the numpy model reaches on numpy-drawn matrices, measured without the code under test: 24 seeds of numpy's negative
# binomial (n = mu / (alpha mu + beta - 1), p = 1 / (alpha mu + beta)) from the same means, size factors, pseudotimes and
# branches as test_gpu_trends._simulation(), the positions by tests/mapping_model.py (poisson_panel, scores, best) under the
# uniform prior; as (mean, standard deviation over the seeds, ddof 1).  The floor of the test is the mean minus SIGMAS standard
# deviations.  DESIGN.md, section 27, has the same figures beside the device's.
BRANCH_ACCURACY = (0.891000, 0.004112)
WITHIN_ONE_NODE = (0.546778, 0.008604)
SIGMAS = 5.0


def position_scores(tree, node, truth):
    """(the share of cells whose node lies on the true branch, the share within one node of the true node on the node tree)."""
    names = list(tree.branches)
    args = ([list(p) for p in tree.topology], {b: int(tree.time[b]) for b in names}, names, tree.root)
    _, code, _ = mm.node_table(*args)
    distance = mm.tree_distance(*args, node, truth)
    return float(np.mean(code[node] == code[truth])), float(np.mean(distance <= 1))


def test_the_loop_from_counts_to_positions_and_on_to_trends_and_fit():
    from test_gpu_trends import _simulation
    from prosstt_amd import fit, mapping, simulation as sim, trends
    t, X, pt, br, sc = _simulation()
    truth = sim.cell_rows(t, pt, br)
    m = mapping.map_cells(X, sc, t, scores=True)
    assert m.node.shape == (3000,) and m.node.dtype == np.int32 and m.scores.shape == (3000, 60)
    # the tolerance and the argmax rule against the model on the device's matrix, from the same float32 panel
    host = X.cpu().numpy()
    means = fit.simulation_means(t)
    P, expo = mapping.poisson_panel(means)
    table = mapping.node_table(t)
    S = mm.scores(host, sc, P, expo)
    b = mm.bound(host, sc, P, expo, None, 256)
    assert np.all(np.abs(m.scores - S) <= b)
    share = mm.check_argmax(S, b, m.node)
    raw = mapping.node_scores(X, sc, P, expo, None, table.offsets)
    assert np.array_equal(raw.best, m.node) and _same_bits(raw.best_score, m.loglik)
    want = mm.lse(S)
    assert np.all(np.abs(raw.lse - want) <= mm.lse_bound(b, want))
    # the fields of the mapping
    assert np.array_equal(sim.cell_rows(t, m.pseudotime, m.branches), m.node)
    assert np.array_equal(np.asarray(m.branch_names)[m.branch_codes], m.branches)
    assert m.branch_posterior.shape == (3000, 3) and np.all(np.abs(m.branch_posterior.sum(axis=1) - 1.0) <= 1e-12)
    assert np.all((m.posterior > 0) & (m.posterior <= 1.0 + 1e-12))
    post = np.exp(S - want[:, None])
    for k in range(3):
        lo, hi = int(table.offsets[k]), int(table.offsets[k + 1])
        # (every term of the two sums moves by a factor within exp(+-b): their ratio by one within exp(+-2 max b))
        share_k = post[:, lo:hi].sum(axis=1)
        assert np.all(np.abs(m.branch_posterior[:, k] - share_k) <= share_k * np.expm1(2 * b.max(axis=1)) + 1e-12), k
    # the density prior moves the scores by the log density; chunks of cells give the same bits
    dens = mapping.map_cells(X, sc, t, prior="density", scores=True)
    log_density = np.log(np.concatenate([t.density[b_] for b_ in t.branches]))
    assert np.all(np.abs((dens.scores - m.scores) - log_density[None, :]) <= 1e-9)
    chunks = [mapping.map_cells(X[lo:lo + 1100], sc[lo:lo + 1100], t) for lo in range(0, 3000, 1100)]
    assert np.array_equal(np.concatenate([ch.node for ch in chunks]), m.node)
    assert _same_bits(np.concatenate([ch.branch_posterior for ch in chunks]), m.branch_posterior)
    # trends and fit run on the mapped positions; a Trends maps cells as its tree does
    tr = trends.expression_trends(X, sc, t, m.pseudotime, m.branches, bandwidth=3.0)
    assert tr.means.shape == (60, 300) and np.array_equal(tr.labels, m.node) and len(tr.empty) == 0
    f = fit.count_model(X, sc, m.node, tr.means)
    has_counts = host.sum(axis=0) > 0
    fitted = np.isfinite(f.alpha[has_counts]) & np.isfinite(f.beta[has_counts])
    print("fit on the mapped positions: alpha and beta finite for %d of %d genes with counts" % (fitted.sum(), has_counts.sum()))
    assert fitted.mean() > 0.9
    again = mapping.map_cells(X, sc, tr)
    assert again.node.shape == (3000,)
    print("mapped again on the learned means: %.4f of the cells keep their node" % np.mean(again.node == m.node))
    accuracy, near = position_scores(t, m.node, truth)
    print("map_cells on smoke()'s tree: branch accuracy %.4f, within one node %.4f, clear best node %.4f"
          % (accuracy, near, share))
    assert accuracy >= BRANCH_ACCURACY[0] - SIGMAS * BRANCH_ACCURACY[1]
    assert near >= WITHIN_ONE_NODE[0] - SIGMAS * WITHIN_ONE_NODE[1]
