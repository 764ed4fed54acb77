"""-m gpu: libprosstt_amd_ranks.so (prosstt_amd/csrc/ranks/ranks.hip) and prosstt_amd.ranks on top of it.

Q and T are exact integers, so every comparison is ``np.array_equal``.  The model (tests/ranks_model.py) works on the device's
own float32 entries: ``embed.LogNormalized.matmul`` with 0/1 selection panels returns them exactly (as ``_a32`` of
tests/test_gpu_markers.py obtains them), and the model only compares them.  Equal integers therefore also show that the emit
kernel forms embed's entries.  The sizes sit around every boundary of the kernels: the wave (64), the block and the fold's
tile (256), the sort's tile (``ranks.SORT_TILE``), more than two tiles, and the strip of 64 x 16 bytes of the 16-byte loads."""
import numpy as np
import pytest

import ranks_model as rm
from test_gpu_markers import FILL, VIEWS, _draw
from test_markers_model import planted_case

pytestmark = pytest.mark.gpu

_cache = {}


def _w():
    from prosstt_amd import ranks
    return ranks.SORT_TILE


def _labels(n_sel, K, seed=0):
    """(labels, N): ``_labels``' pattern of tests/test_gpu_markers.py with exactly ``n_sel`` labelled cells: about 15 % of
    the N cells left out (-1), for K >= 3 group 1 empty and group K - 1 a single cell; interleaved."""
    rng = np.random.default_rng(n_sel * 31 + K + seed)
    N = n_sel + max(1, int(round(n_sel * 0.15 / 0.85)))
    many = [k for k in range(K) if K < 3 or k not in (1, K - 1)]
    inside = np.asarray(many)[rng.integers(0, len(many), size=n_sel)]
    inside[rng.integers(0, n_sel)] = K - 1
    labels = np.full(N, -1, dtype=np.int64)
    labels[np.sort(rng.choice(N, size=n_sel, replace=False))] = inside
    return labels, N


def _input(kind, N, G):
    """(X int32 (N, G), s): (a) the negative-binomial draw of tests/test_gpu_markers.py, half zeros, lognormal size factors:
    nearly all non-zero keys distinct; (b) size factor 1 and small counts: long runs of ties, with a column of one repeated
    non-zero value, an all-zero column and a column alternating two values; (c) size factors from 2^-90 to 2^90: all four key
    bytes differ between cells; (d) size factor 1, counts ascending and descending in row order."""
    key = (kind, N, G)
    if key not in _cache:
        rng = np.random.default_rng(N * 7919 + G + ord(kind))
        if kind == "a":
            X, s = _draw(N, G)
        elif kind == "b":
            X, s = rng.poisson(1.5, size=(N, G)).astype(np.int32), np.ones(N)
            X[:, 0] = 7
            if G > 1:
                X[:, 1] = 0
            if G > 2:
                X[:, 2] = np.where(np.arange(N) % 2 == 0, 3, 11)
        elif kind == "c":
            X = rng.integers(0, 1 << 20, size=(N, G)).astype(np.int32)
            X[rng.random((N, G)) < 0.3] = 0
            s = 2.0 ** rng.uniform(-90, 90, size=N)
        else:
            X = np.empty((N, G), dtype=np.int32)
            X[:, 0::2] = np.arange(N)[:, None] * 3 + 1
            X[:, 1::2] = (N - np.arange(N))[:, None] * 5
            s = np.ones(N)
        _cache[key] = (X, s)
    return _cache[key]


def _view(kind, N, G, view):
    """The matrix on the device: "aligned", or "shifted": an odd row stride and a base one element past 16-byte alignment
    (the scalar path) inside a wider tensor filled with FILL, so that a read past the view shows in the sums."""
    import torch
    key = ("view", kind, N, G, view)
    if key not in _cache:
        X = torch.as_tensor(_input(kind, N, G)[0]).cuda()
        if view == "aligned":
            assert X.data_ptr() % 16 == 0
            _cache[key] = X
        else:
            pad = 3 if G % 2 == 0 else 2
            wide = torch.full((N, G + pad), FILL, dtype=torch.int32, device="cuda")
            wide[:, 1:1 + G] = X
            _cache[key] = wide[:, 1:1 + G]
            assert _cache[key].data_ptr() % 16 == 4 and (N == 1 or _cache[key].stride(0) % 2 == 1)
    return _cache[key]


def _a32(kind, N, G):
    """The device's own float32 entries of the matrix, as a host array: selection panels of at most 128 genes."""
    import torch
    from prosstt_amd import embed
    key = ("a32", kind, N, G)
    if key not in _cache:
        op = embed.LogNormalized(_view(kind, N, G, "aligned"), _input(kind, N, G)[1])
        out = torch.empty(N, G, dtype=torch.float32, device="cuda")
        for g0 in range(0, G, 128):
            w = min(128, G - g0)
            P = torch.zeros(G, w, dtype=torch.float32, device="cuda")
            P[g0 + torch.arange(w, device="cuda"), torch.arange(w, device="cuda")] = 1.0
            out[:, g0:g0 + w] = op.matmul(P)
        _cache[key] = out.cpu().numpy()
    return _cache[key]


def _want(kind, N, G, labels, K, reference):
    """The model's (Q, T, n), computed once per case."""
    key = ("want", kind, N, G, K, reference, labels.tobytes())
    if key not in _cache:
        _cache[key] = rm.rank_sums(_a32(kind, N, G), labels, K, reference=reference)
    return _cache[key]


def _check(rs, want, K):
    Q, T, n = want
    assert list(rs.groups) == list(range(K)) and np.array_equal(rs.n, n)
    assert rs.q.dtype == np.int64 and rs.ties.dtype == np.int64
    assert np.array_equal(rs.q, Q), np.argwhere(rs.q != Q)[:5]
    assert np.array_equal(rs.ties, T), np.flatnonzero(rs.ties != T)[:5]


def _sizes():
    W = 1024                    # (asserted against ranks.SORT_TILE in the test: the parameters are made before the import)
    return [1, 2, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, 2 * W + 3, 5000]


@pytest.mark.parametrize("n_sel", _sizes())
def test_every_boundary_of_the_segment(n_sel):
    """n_sel around the wave, the block and the sort's tile, K = 3 with its empty and single-cell groups, both views."""
    from prosstt_amd import ranks
    W = _w()
    assert _sizes() == [1, 2, 63, 64, 65, 255, 256, 257, W - 1, W, W + 1, 2 * W + 3, 5000]
    K, G = 3, 5
    labels, N = _labels(n_sel, K)
    assert int((labels >= 0).sum()) == n_sel
    for kind in ("a", "b"):
        s = _input(kind, N, G)[1]
        want = _want(kind, N, G, labels, K, None)
        for view in VIEWS:
            _check(ranks.rank_sums(_view(kind, N, G, view), s, labels), want, K)


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("view", VIEWS)
def test_gene_counts_and_views(G, view):
    from prosstt_amd import ranks
    K = 3
    labels, N = _labels(257, K)
    s = _input("a", N, G)[1]
    _check(ranks.rank_sums(_view("a", N, G, view), s, labels), _want("a", N, G, labels, K, None), K)


@pytest.mark.parametrize("view", VIEWS)
def test_a_whole_strip_and_its_remainder(view):
    """More genes than one strip of the emit kernel (1024): the 16-byte path over a whole strip, and the strip's remainder.
    (Few cells: the model compares all pairs.)"""
    from prosstt_amd import ranks
    K, G = 3, 1024 + 37
    labels, N = _labels(65, K)
    s = _input("a", N, G)[1]
    want = _want("a", N, G, labels, K, None)
    for gpp in (0, 1024, 1028):
        _check(ranks.rank_sums(_view("a", N, G, view), s, labels, genes_per_pass=gpp), want, K)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("K", [1, 3, 7, 1024])
def test_inputs_groups_and_references(kind, K):
    """Every input over two tiles of the sort and nine of the fold, for "rest", a populated group and the empty group."""
    from prosstt_amd import ranks
    G = 6
    labels, N = _labels(2 * _w() + 3, K)
    s = _input(kind, N, G)[1]
    X = _view(kind, N, G, "aligned")
    populated = 0
    references = [(None, "rest"), (populated, populated)] + ([(1, 1)] if K >= 3 else [])
    for index, reference in references:
        rs = ranks.rank_sums(X, s, labels, reference=reference)
        _check(rs, _want(kind, N, G, labels, K, index), K)
        assert rs.reference == reference and np.array_equal(rs.codes, labels)
        if index == 1:
            assert rs.n[1] == 0 and not rs.q.any()                          # an empty counting set gives zeros
    if K >= 3:
        assert rs.n[K - 1] == 1
    if kind == "b":
        n = 2 * _w() + 3
        rest = ranks.rank_sums(X, s, labels)
        assert rest.ties[0] == n ** 3 - n and rest.ties[1] == n ** 3 - n    # one run of n_sel positions
        assert np.array_equal(rest.q[:, 0], rest.n * n) and np.array_equal(rest.q[:, 1], rest.n * n)


@pytest.mark.parametrize("kind", ["a", "b"])
def test_every_genes_per_pass_gives_the_same(kind):
    from prosstt_amd import ranks
    K, G = 7, 130
    labels, N = _labels(257, K)
    s = _input(kind, N, G)[1]
    want = _want(kind, N, G, labels, K, 0)
    for view in VIEWS:
        for gpp in (0, 1, 7, 64):
            _check(ranks.rank_sums(_view(kind, N, G, view), s, labels, reference=0, genes_per_pass=gpp), want, K)


def test_presented_counts():
    """Rows permuted: the labels follow the cells; the integers do not depend on the order of the rows."""
    import torch
    from prosstt_amd import device, ranks
    K, G = 3, 65
    labels, N = _labels(257, K)
    X, s = _input("a", N, G)
    cell_of_row = np.random.default_rng(N).permutation(N)
    presented = device.PresentedCounts(torch.as_tensor(X[cell_of_row]).cuda(), cell_of_row)
    rs = ranks.rank_sums(presented, s, labels, reference=2)
    _check(rs, _want("a", N, G, labels, K, 2), K)
    assert np.array_equal(rs.codes, labels)


def test_equal_integers_across_calls_and_streams():
    import torch
    from prosstt_amd import ranks
    K, G = 7, 130
    labels, N = _labels(_w() + 1, K)
    s = _input("b", N, G)[1]
    X = _view("b", N, G, "aligned")
    first = ranks.rank_sums(X, s, labels, out="torch")
    again = ranks.rank_sums(X, s, labels, out="torch")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = ranks.rank_sums(X, s, labels, out="torch")
    side.synchronize()
    assert first.q.is_cuda and first.q.shape == (K, G) and first.ties.shape == (G,)
    for y in (again, other):
        assert torch.equal(first.q, y.q) and torch.equal(first.ties, y.ties)
    _check(first._replace(q=first.q.cpu().numpy(), ties=first.ties.cpu().numpy()), _want("b", N, G, labels, K, None), K)


def test_a_negative_count_raises():
    import torch
    from prosstt_amd import ranks
    N, G = 130, 65
    X, s = _input("a", N, G)
    bad = torch.as_tensor(X).cuda()
    bad[N - 1, G - 1] = -1
    labels = np.arange(N) % 3
    with pytest.raises(ValueError, match="negative"):
        ranks.rank_sums(bad, s, labels)
    labels[N - 1] = -1                                             # the row is not selected: nothing reads it
    ranks.rank_sums(bad, s, labels)


def test_refusals_of_the_abi():
    import ctypes
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load("ranks")
    N, G, K = 67, 65, 3
    X = _view("a", N, G, "aligned")
    inv = torch.ones(N, dtype=torch.float32, device="cuda")
    rows = torch.arange(N, dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 20, 20, N], dtype=torch.int64, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_ranks_workspace_bytes(N, G, 0, ctypes.byref(need)), "ranks")
    assert need.value == 2 * (-(-N * G * 4 // 256) * 256) + 2 * (-(-N * G * 2 // 256) * 256)      # 12 bytes per entry, padded
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    Q = torch.empty((K, G), dtype=torch.int64, device="cuda")
    T = torch.empty(G, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(N=N, G=G, ld=X.stride(0), n_sel=N, K=K, reference=-1, gpp=0, bytes_=need.value):
        return L.prosstt_amd_ranks_rank_sums(None, _ptr(X), N, G, ld, _ptr(inv), _ptr(rows), n_sel, _ptr(start), K, reference, gpp,
                                             _ptr(ws), bytes_, _ptr(Q), _ptr(T), _ptr(status))

    assert call() == 0
    for kw, text in ((dict(K=1025), "groups"), (dict(K=0), "groups"), (dict(bytes_=need.value - 1), "workspace"),
                     (dict(ld=G - 1), "row stride"), (dict(N=0), "N"), (dict(N=1 << 31), "N"), (dict(n_sel=N + 1), "selected"),
                     (dict(n_sel=-1), "n_sel"), (dict(gpp=-1), "genes_per_pass"), (dict(G=0), "G"), (dict(reference=K), "reference"),
                     (dict(reference=-2), "reference")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(call(**kw), "ranks")
    for sizes, text in ((((1 << 20) + 1, G, 0), "n_sel"), ((N, 0, 0), "G"), ((N, G, -1), "genes_per_pass")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_ranks_workspace_bytes(*sizes, ctypes.byref(need)), "ranks")
    # the rule for genes_per_pass = 0 keeps the workspace at or below 1 GiB, and one gene always fits
    for n_sel, genes in ((50000, 20000), (1 << 20, 20000), (0, 5)):
        _native.check(L.prosstt_amd_ranks_workspace_bytes(n_sel, genes, 0, ctypes.byref(need)), "ranks")
        assert need.value <= 1 << 30
        if n_sel:
            assert need.value > (1 << 30) - 12 * n_sel - 1024
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_a_row_outside_the_matrix_and_bad_offsets_are_reported():
    """The C ABI's own guards (ranks.py builds both arrays itself): a row index outside [0, N) is not read and sets a bit;
    offsets that do not ascend from 0 to n_sel set another, and every position still gets a group below K."""
    import ctypes
    import torch
    from prosstt_amd import _native, ranks
    from prosstt_amd.device import _ptr
    L = _native.load("ranks")
    N, G, K = 67, 65, 2
    X = _view("a", N, G, "aligned")
    inv = torch.ones(N, dtype=torch.float32, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_ranks_workspace_bytes(9, G, 0, ctypes.byref(need)), "ranks")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    Q = torch.empty((K, G), dtype=torch.int64, device="cuda")
    T = torch.empty(G, dtype=torch.int64, device="cuda")
    for rows, start, want in (([0, 1, N, 3, 4, 5, -1, 7, 8], [0, 5, 9], ranks.ROW_RANGE),
                              ([0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 12, 9], ranks.GROUP_RANGE),
                              ([0, 1, 2, 3, 4, 5, 6, 7, 8], [-3, 4, 1 << 40], ranks.GROUP_RANGE)):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        r = torch.tensor(rows, dtype=torch.int32, device="cuda")
        st = torch.tensor(start, dtype=torch.int64, device="cuda")
        _native.check(L.prosstt_amd_ranks_rank_sums(None, _ptr(X), N, G, X.stride(0), _ptr(inv), _ptr(r), len(rows), _ptr(st), K, -1,
                                                    0, _ptr(ws), need.value, _ptr(Q), _ptr(T), _ptr(status)), "ranks")
        assert int(status.item()) == want
        # whatever the groups are, every position was counted once: the rank sums of all groups add up to n^2
        assert np.array_equal(Q.sum(0).cpu().numpy(), np.full(G, 81))


@pytest.mark.parametrize("tie_correct", [False, True])
def test_planted_markers_end_to_end(tie_correct):
    import torch
    from prosstt_amd import embed, markers
    X, s, labels = planted_case()
    Xd = torch.as_tensor(X).cuda()
    res = markers.rank_genes_groups(Xd, s, labels, method="wilcoxon", tie_correct=tie_correct)
    N, G = X.shape
    op = embed.LogNormalized(Xd, s)
    A = op.matmul(torch.eye(G, dtype=torch.float32, device="cuda")).cpu().numpy()      # (G = 60: one selection panel)
    Q, T, n = rm.rank_sums(A, labels, 3)
    want = rm.wilcoxon(Q, T, n, tie_correct=tie_correct)
    names = rm.rank(want["z"])
    assert np.array_equal(res.names, names)
    for field, key in (("scores", "z"), ("pvals", "pvals"), ("pvals_adj", "pvals_adj")):
        np.testing.assert_allclose(getattr(res, field), np.take_along_axis(want[key], names, 1), rtol=1e-12, atol=0, err_msg=field)
    assert set(res.names[1][:10]) == set(range(10))                                   # the planted genes are on top
    assert np.all(res.pvals_adj[1][:10] < 0.01) and np.all(res.logfoldchanges[1][:10] > 2.5)     # ten times the mean
    t = markers.rank_genes_groups(res.moments)
    assert set(t.names[1][:10]) == set(range(10)) and res.moments.n.sum() == N
    top = markers.rank_genes_groups(Xd, s, labels, method="wilcoxon", reference=0, n_genes=10)
    assert top.names.shape == (3, 10) and not top.scores[0].any()
