"""-m gpu: prosstt_amd.evaluate (libprosstt_amd_evaluate.so) against the numpy model of tests/evaluate_model.py.  Everything
the library computes is an integer: every comparison is exact, on every path (tests/test_evaluate_host.py shows with a mirror
of the block tables which kinds of block and tile the cases below reach).

The class sizes are drawn from {0, 1, 2, 255, 256, 257, 511, 512, 513, 1025}: both sides of a tile edge (256 columns) and of
a row-block edge (512 rows), and 1025 = two whole row blocks and one row, four whole tiles and one column."""
import ctypes
import functools

import numpy as np
import pytest

import evaluate_model as em

pytestmark = pytest.mark.gpu

CAP = em.MAX_TILES
TILES = (1, 2, 3, CAP, 0)
# class sizes, in several orders; the first of each K stands for "K = 1, 2, 3"
SIZE_CASES = {
    "K = 1": (700,),
    "K = 2": (300, 513),
    "K = 3": (257, 2, 512),
    "edges": (513, 0, 257, 1, 2),
    "tiles": (1025, 256, 255, 512),
    "small and large": (2, 511, 0, 0, 1025, 1),
    "N = 2, one class": (2,),
    "N = 2, two classes": (1, 1),
}
KINDS = ("heavy ties", "no ties", "all equal", "a = b", "a = -b")


def _sizes_64():
    """K = 64 with about 200 cells: most classes empty or of one cell."""
    rng = np.random.default_rng(64)
    sizes = rng.integers(0, 2, 64)
    sizes[[3, 40, 63]] = (70, 50, 30)
    return tuple(int(v) for v in sizes)


SIZE_CASES["K = 64"] = _sizes_64()


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()


@functools.lru_cache(maxsize=None)
def _classes(case):
    """The class of every cell, shuffled (the wrapper sorts), read-only."""
    sizes = SIZE_CASES[case]
    rng = np.random.default_rng(len(sizes) + sum(sizes))
    classes = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    classes.setflags(write=False)
    return classes


@functools.lru_cache(maxsize=None)
def _sequences(case, kind):
    """(a, b, the model's (K, K, 4) counts, the model's pairs), read-only."""
    classes = _classes(case)
    N, K = len(classes), len(SIZE_CASES[case])
    rng = np.random.default_rng(N + len(kind))
    perm = rng.permutation(N)
    a, b = {
        "heavy ties": (rng.integers(0, 6, N), rng.integers(0, 6, N)),
        "no ties": (perm, rng.permutation(N)),
        "all equal": (np.full(N, 7), perm),
        "a = b": (perm, perm),
        "a = -b": (perm, -perm),
    }[kind]
    order, offsets = em.by_class(classes, K)
    out = (a.astype(np.int64), b.astype(np.int64), em.pair_counts(a[order], b[order], offsets), em.pairs(offsets))
    for arr in out:
        arr.setflags(write=False)
    return out


def _stack(pc):
    return np.stack([np.asarray(v) for v in (pc.s, pc.p, pc.a2, pc.b2)], axis=-1)


@pytest.mark.parametrize("case", list(SIZE_CASES))
def test_pair_counts_are_the_models_on_every_tiles_per_block(case):
    from prosstt_amd import evaluate
    classes, K = _classes(case), len(SIZE_CASES[case])
    for kind in KINDS:
        a, b, want, pairs = _sequences(case, kind)
        for tiles in TILES:
            got = evaluate.pair_counts(a, b, classes, K, tiles_per_block=tiles)
            assert got.s.dtype == np.int64 and np.array_equal(got.pairs, pairs)
            assert np.array_equal(_stack(got), want), (kind, tiles)
    # the closed forms of the extremes
    a, b, want, pairs = _sequences(case, "a = b")
    assert np.array_equal(want[..., 0], pairs) and np.array_equal(want[..., 1], pairs)
    assert np.array_equal(_sequences(case, "a = -b")[2][..., 0], -pairs)
    assert not _sequences(case, "all equal")[2][..., :3].any()


def test_device_inputs_out_torch_a_second_stream_and_k_from_the_classes():
    import torch
    from prosstt_amd import evaluate
    case = "edges"
    classes, K = _classes(case), len(SIZE_CASES[case])
    a, b, want, pairs = _sequences(case, "heavy ties")
    on_device = evaluate.pair_counts(_cuda(a), _cuda(b), _cuda(classes), K, out="torch")
    assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dtype == torch.int64 for v in on_device[:4])
    assert np.array_equal(np.stack([v.cpu().numpy() for v in on_device[:4]], axis=-1), want)
    assert on_device.gamma() == evaluate.pair_counts(a, b, classes, K).gamma()
    mixed = evaluate.pair_counts(a.astype(np.int32), _cuda(b), classes)             # K = the largest class + 1
    assert np.array_equal(_stack(mixed), want)
    unsigned = evaluate.pair_counts(a.astype(np.uint64), b.astype(np.uint16), classes.astype(np.uint8), K)   # (values 0 .. 5)
    assert np.array_equal(_stack(unsigned), want)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = evaluate.pair_counts(_cuda(a), _cuda(b), _cuda(classes), K, tiles_per_block=2)
    stream.synchronize()
    assert np.array_equal(_stack(other), want)
    with pytest.raises(ValueError):
        evaluate.pair_counts(_cuda(a), _cuda(b), _cuda(classes), 2)                 # a class outside [0, K), seen on the device
    with pytest.raises(ValueError):
        evaluate.pair_counts(_cuda(a + (1 << 30)), _cuda(b), _cuda(classes), K)


# ------------------------------------------------------------------------------------------------------- the moments

def _junctions(rng, K):
    """A symmetric table: junction depths off the diagonal, some pairs on a common lineage (MAX_DEPTH)."""
    J = rng.integers(0, 40000, (K, K))
    J = np.minimum(J, J.T)
    J[rng.random((K, K)) < 0.3] = em.MAX_DEPTH
    J = np.maximum(J, J.T)
    J[np.diag_indices(K)] = em.MAX_DEPTH
    return J.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _trees(case, K2):
    """(h, J, h2, c2, J2, the model's words, pairs): depths over the whole range with 0 and 65 535 among them; read-only."""
    classes = _classes(case)
    N, K = len(classes), len(SIZE_CASES[case])
    rng = np.random.default_rng(N + K2)
    h, h2 = rng.integers(0, em.MAX_DEPTH + 1, N), rng.integers(0, em.MAX_DEPTH + 1, N)
    h[:2], h2[:2] = (0, em.MAX_DEPTH), (em.MAX_DEPTH, 0)
    c2 = rng.integers(0, K2, N)
    c2[-1] = K2 - 1
    J, J2 = _junctions(rng, K), _junctions(rng, K2)
    order, offsets = em.by_class(classes, K)
    out = (h, J, h2, c2, J2, em.words(em.pair_moments(h[order], offsets, J, h2[order], c2[order], J2)), em.pairs(offsets))
    for arr in out:
        arr.setflags(write=False)
    return out


@pytest.mark.parametrize("K2", [1, 64])
@pytest.mark.parametrize("case", list(SIZE_CASES))
def test_pair_moments_are_the_models_on_every_tiles_per_block(case, K2):
    import torch
    from prosstt_amd import evaluate
    classes = _classes(case)
    h, J, h2, c2, J2, want, pairs = _trees(case, K2)
    for tiles in TILES:
        got = evaluate.tree_moments(h, classes, J, h2, c2, J2, tiles_per_block=tiles)
        assert got.words.dtype == np.uint64 and np.array_equal(got.words, want), tiles
        assert np.array_equal(got.pairs, pairs)
    on_device = evaluate.tree_moments(_cuda(h), _cuda(classes), J, _cuda(h2), _cuda(c2), J2, out="torch")
    assert on_device.words.is_cuda and np.array_equal(on_device.words.cpu().numpy().view(np.uint64), want)
    assert np.array_equal([on_device.pearson()], [got.pearson()], equal_nan=True)     # (one pair: no variance, NaN)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        other = evaluate.tree_moments(_cuda(h), _cuda(classes), J, _cuda(h2), _cuda(c2), J2, tiles_per_block=2)
    stream.synchronize()
    assert np.array_equal(other.words, want)
    # the second tree equal to the first: r = 1 exactly (where the distances vary at all)
    same = evaluate.tree_moments(h, classes, J, h, classes, J)
    assert np.array_equal(same.d, same.d2) and np.array_equal(same.dd, same.dd2) and np.array_equal(same.dd, same.d2d2)
    r = same.pearson()
    assert r == 1.0 or (np.isnan(r) and len(h) == 2)


def test_the_64_bit_bound_where_it_is_tightest():
    """Two classes of 512 and 4096 x 256 cells, every depth 65 535, junction 0, tiles_per_block at the cap: one block holds
    512 x 2^20 pairs of distance 131 070 each, the largest partial sum a block can have.  The sums are a closed form."""
    import torch
    from prosstt_amd import evaluate
    n0, n1 = em.BLOCK_ROWS, CAP * em.TILE
    classes = torch.cat([torch.zeros(n0, dtype=torch.int64), torch.ones(n1, dtype=torch.int64)]).cuda()
    h = torch.full((n0 + n1,), em.MAX_DEPTH, dtype=torch.int32, device="cuda")
    J = np.array([[em.MAX_DEPTH, 0], [0, em.MAX_DEPTH]], dtype=np.int32)
    got = evaluate.tree_moments(h, classes, J, h, classes, J, tiles_per_block=CAP)
    n, d = n0 * n1, 2 * em.MAX_DEPTH
    assert n * d * d < 1 << 63 and 2 * n * d * d >= 1 << 63       # the bound of the header, and no slack of a factor 2
    for table, value in ((got.d, n * d), (got.d2, n * d), (got.dd, n * d * d), (got.d2d2, n * d * d), (got.dd2, n * d * d)):
        assert table[0, 1] == value and table[0, 0] == 0 and table[1, 1] == 0 and table[1, 0] == 0
    assert got.pairs[0, 1] == n and got.pairs[1, 1] == n1 * (n1 - 1) // 2
    # the same through the default: several chunks and the 128-bit fold
    assert np.array_equal(evaluate.tree_moments(h, classes, J, h, classes, J).words, got.words)


# ------------------------------------------------------------------------------------------------------- the ABI

def _abi(N, K, K2, offsets, h, h2, c2, tiles=0, counts=False):
    """(return code of pair_moments, status, the output words after the call, prefilled with 0x5A bytes); with ``counts``, of
    pair_counts on (h, h2) as its two sequences."""
    import torch
    from prosstt_amd import _native
    L = _native.load("evaluate")
    need = ctypes.c_uint64(0)
    if L.prosstt_amd_evaluate_workspace_bytes(N, min(K, 64), tiles, ctypes.byref(need)) != 0:
        need.value = 1 << 20
    ws = torch.zeros(int(need.value), dtype=torch.uint8, device="cuda")
    out = torch.full((K * K * 10 * 8,), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    J = torch.full((K * K,), em.MAX_DEPTH, dtype=torch.int32, device="cuda")
    J2 = torch.full((K2 * K2,), em.MAX_DEPTH, dtype=torch.int32, device="cuda")
    tensors = [_cuda(np.asarray(v, dtype=np.int32)) for v in (h, h2, c2)] + [_cuda(np.asarray(offsets, dtype=np.int64))]
    p = [ctypes.c_void_p(t.data_ptr()) for t in tensors]
    if counts:
        rc = L.prosstt_amd_evaluate_pair_counts(None, p[0], p[1], p[3], N, K, tiles, ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                                ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    else:
        rc = L.prosstt_amd_evaluate_pair_moments(None, p[0], p[1], p[2], p[3], ctypes.c_void_p(J.data_ptr()),
                                                 ctypes.c_void_p(J2.data_ptr()), N, K, K2, tiles, ctypes.c_void_p(ws.data_ptr()),
                                                 ws.numel(), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(status.data_ptr()))
    torch.cuda.synchronize()
    return rc, int(status.item()), out.cpu().numpy()


def test_one_past_each_limit_is_refused_or_flagged_and_nothing_is_written():
    from prosstt_amd import _native, evaluate
    N = 300
    zeros = np.zeros(N, dtype=np.int32)
    good = [0, 100, 300]
    rc, status, out = _abi(N, 2, 1, good, zeros, zeros, zeros)
    assert rc == 0 and status == 0 and not np.all(out == 0x5A)              # the call itself is sound
    untouched = lambda out: bool(np.all(out == 0x5A))                       # noqa: E731
    # refused before anything is enqueued
    for K, K2, tiles in ((65, 1, 0), (2, 65, 0), (2, 0, 0), (0, 1, 0), (2, 1, CAP + 1), (2, 1, -1)):
        offsets = [0] * max(K, 1) + [N]
        rc, status, out = _abi(N, K, K2, offsets, zeros, zeros, zeros, tiles)
        assert rc == _native.EINVAL and status == 0 and untouched(out), (K, K2, tiles)
    # flagged by the pass: nothing is written
    deep = zeros.copy()
    deep[150] = em.MAX_DEPTH + 1
    for args, bit in (((good, deep, zeros, zeros), evaluate.DEPTH_RANGE), ((good, zeros, deep, zeros), evaluate.DEPTH_RANGE),
                      ((good, zeros - 1, zeros, zeros), evaluate.DEPTH_RANGE),
                      ((good, zeros, zeros, zeros + 1), evaluate.BRANCH_RANGE), ((good, zeros, zeros, zeros - 1), evaluate.BRANCH_RANGE),
                      (([0, 200, 100], zeros, zeros, zeros), evaluate.OFFSETS_RANGE),
                      (([0, 100, 299], zeros, zeros, zeros), evaluate.OFFSETS_RANGE),
                      (([1, 100, 300], zeros, zeros, zeros), evaluate.OFFSETS_RANGE),
                      (([0, 100, 1 << 40], zeros, zeros, zeros), evaluate.OFFSETS_RANGE)):
        rc, status, out = _abi(N, 2, 1, *args)
        assert rc == 0 and status & bit and untouched(out), (args[0], bit)
        with pytest.raises(ValueError):
            evaluate.check_status(status)
    # the counts through the ABI: a sound call, the same refusals, bad offsets flagged, nothing written
    rc, status, out = _abi(N, 2, 1, good, zeros, zeros, zeros, counts=True)
    assert rc == 0 and status == 0 and not np.all(out[:2 * 2 * 4 * 8] == 0x5A) and untouched(out[2 * 2 * 4 * 8:])
    for K, tiles in ((65, 0), (0, 0), (2, CAP + 1), (2, -1)):
        rc, status, out = _abi(N, K, 1, [0] * max(K, 1) + [N], zeros, zeros, zeros, tiles, counts=True)
        assert rc == _native.EINVAL and status == 0 and untouched(out), (K, tiles)
    for offsets in ([0, 200, 100], [0, 100, 299], [1, 100, 300], [0, 100, 1 << 40]):
        rc, status, out = _abi(N, 2, 1, offsets, zeros, zeros, zeros, counts=True)
        assert rc == 0 and status == evaluate.OFFSETS_RANGE and untouched(out), offsets
    # the wrapper's verdict for device tensors that it does not look at on the host
    with pytest.raises(ValueError, match="DEPTH_RANGE"):
        evaluate.tree_moments(_cuda(deep), _cuda(zeros), [[em.MAX_DEPTH]], _cuda(zeros), _cuda(zeros), [[em.MAX_DEPTH]])


# ------------------------------------------------------------------------------------------------------ the whole call

def test_trajectory_of_a_lineage_fit_on_smokes_tree():
    import ptree_quality
    from test_gpu_trends import _simulation
    from prosstt_amd import embed, evaluate, ptree
    t, X, pt, br, sc = _simulation()
    lf = ptree.principal_tree(embed.pca(X, sc, ptree_quality.N_COMPONENTS).scores).to_tree(root=int(np.argmin(pt)), G=300)
    ev = evaluate.trajectory(t, pt, br, lf)
    assert ev.labels.accuracy == ptree_quality.branch_accuracy(lf.branches, br)
    assert abs(ev.ordering.spearman - ptree_quality.spearman(lf.position, pt)) <= 1e-12
    # the ordering's counts against the model, with the ranks the wrapper takes
    codes = np.array([list(t.branches).index(b) for b in br])
    a = np.unique(pt, return_inverse=True)[1]
    b = np.unique(lf.position, return_inverse=True)[1]
    order, offsets = em.by_class(codes, 3)
    assert np.array_equal(_stack(ev.ordering.counts), em.pair_counts(a[order], b[order], offsets))
    assert ev.ordering.branch_names == list(t.branches)
    assert np.array_equal(ev.ordering.comparable_mask, np.array([[1, 1, 1], [1, 1, 0], [1, 0, 1]], dtype=bool))
    assert -1.0 <= ev.ordering.comparable.gamma <= 1.0 and ev.ordering.within.tau_b > 0
    r = ev.distances.pearson()
    print("trajectory on smoke()'s tree: accuracy %.4f, ARI %.4f, NMI %.4f, gamma (comparable) %.4f, tau-b (all) %.4f, "
          "Spearman %.4f, distance correlation %.4f" % (ev.labels.accuracy, ev.labels.ari, ev.labels.nmi,
                                                        ev.ordering.comparable.gamma, ev.ordering.overall.tau_b,
                                                        ev.ordering.spearman, r))
    assert 0.0 < r <= 1.0
    # the truth against itself; a DPT-like and a mapping-like answer through the tuple form
    perfect = evaluate.trajectory(t, pt, br, (br, pt, t))
    assert perfect.labels.accuracy == 1.0 and perfect.labels.ari == 1.0 and perfect.ordering.overall.tau_b == 1.0
    assert perfect.ordering.spearman == 1.0 and perfect.distances.pearson() == 1.0
    partial = evaluate.trajectory(t, pt, br, (None, -pt.astype(np.float64)))
    assert partial.labels is None and partial.distances is None and partial.ordering.overall.gamma == -1.0
    # the other two result types, as their libraries return them: device tensors with groups, and host arrays
    from prosstt_amd import dpt, mapping
    groups = np.array([list(t.branches).index(b) + 1 for b in br], dtype=np.int8)
    groups[::7] = 0                                                # the branching region: a label of its own
    found = dpt.DPT(_cuda(pt / pt.max()), _cuda(groups), (0, 1, 2), (5, 5, 5))
    ev = evaluate.trajectory(t, pt, br, found)
    assert ev.distances is None and ev.ordering.overall.tau_b == 1.0 and ev.labels.table.shape == (3, 4)
    assert ev.labels.accuracy == float(np.mean(groups > 0)) and ev.labels.matching == {"A": 1, "B": 2, "C": 3}
    assert evaluate.trajectory(t, pt, br, dpt.DPT(pt / pt.max(), None, None, None)).labels is None
    found = mapping.CellMapping(None, lf.branches, None, lf.pseudotime, None, None, None, None, list(lf.tree.branches))
    ev = evaluate.trajectory(t, pt, br, found)
    assert ev.distances is None and ev.labels.accuracy == ptree_quality.branch_accuracy(lf.branches, br)
    assert abs(ev.ordering.spearman - ptree_quality.spearman(lf.pseudotime, pt)) <= 1e-12
