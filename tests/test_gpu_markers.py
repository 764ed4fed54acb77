"""-m gpu: the grouped pass of libprosstt_amd_markers.so (prosstt_amd/csrc/markers/markers.hip) and prosstt_amd.markers on
top of it.

The float sums are compared BIT FOR BIT: ``embed.LogNormalized.matmul`` with 0/1 selection panels returns the device's own
float32 entries log1p(x * inv_size) exactly (an f32 MFMA chain with a single 1; tests/test_gpu_embed_paths.py), and
``markers_model.sums`` adds them in the kernel's order.  So equal bits here also prove that the pass forms embed's entries.
The integers are compared with numpy's.  Against binary64 log1p(X / s) the sums are within embed's entry bound (2^-20 per
entry, so 2^-19 + 2^-39 per square) plus the bound n 2^-52 of recursive summation over n rows."""
import ctypes

import numpy as np
import pytest

import markers_model as mm
from test_markers_model import planted_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 3), (67, 1023), (130, 1024), (259, 1025), (300, 2051)]
VIEWS = ["aligned", "shifted"]          # shifted: odd row stride and a base one element past 16-byte alignment (scalar path)
GROUPS = [1, 3, 7]
ROWS_PER_BLOCK = [0, 1, 64, 100]
FILL = 12345                            # the padding of the wider tensor: a read past the view shows in every sum

_cache = {}


def _draw(N, G):
    """(X int32, s): negative-binomial counts, two thirds of them zeros, a few large ones; size factors around 1."""
    rng = np.random.default_rng(N * 7919 + G)
    X = rng.negative_binomial(0.7, 0.1, size=(N, G)).astype(np.int64)
    kind = rng.random((N, G))
    X[kind < 0.5] = 0
    X[kind > 0.99] = rng.integers(1 << 16, 1 << 31, size=int((kind > 0.99).sum()))
    return X.astype(np.int32), rng.lognormal(0.0, 0.7, size=N)


def _host(N, G):
    if ("host", N, G) not in _cache:
        _cache["host", N, G] = _draw(N, G)
    return _cache["host", N, G]


def _view(N, G, view):
    import torch
    key = ("view", N, G, view)
    if key not in _cache:
        X = torch.as_tensor(_host(N, G)[0]).cuda()
        if view == "aligned":
            assert X.data_ptr() % 16 == 0
            _cache[key] = X
        else:
            pad = 3 if G % 2 == 0 else 2                   # an odd row stride
            wide = torch.full((N, G + pad), FILL, dtype=torch.int32, device="cuda")
            wide[:, 1:1 + G] = X
            _cache[key] = wide[:, 1:1 + G]
            assert _cache[key].data_ptr() % 16 == 4 and (N == 1 or _cache[key].stride(0) % 2 == 1)
    return _cache[key]


def _a32(N, G):
    """The device's own float32 entries of the drawn matrix, as a host array: selection panels of at most 128 genes."""
    import torch
    from prosstt_amd import embed
    if ("a32", N, G) not in _cache:
        op = embed.LogNormalized(_view(N, G, "aligned"), _host(N, G)[1])
        out = torch.empty(N, G, dtype=torch.float32, device="cuda")
        for g0 in range(0, G, 128):
            w = min(128, G - g0)
            P = torch.zeros(G, w, dtype=torch.float32, device="cuda")
            P[g0 + torch.arange(w, device="cuda"), torch.arange(w, device="cuda")] = 1.0
            out[:, g0:g0 + w] = op.matmul(P)
        _cache["a32", N, G] = out.cpu().numpy()
    return _cache["a32", N, G]


def _labels(N, K):
    """Interleaved integer labels in [-1, K): about one cell in seven left out; for K >= 3 group 1 is empty and group
    K - 1 has a single cell (the last label present makes K the number of categories)."""
    rng = np.random.default_rng(N * 31 + K)
    many = [k for k in range(K) if K < 3 or k not in (1, K - 1)]
    labels = np.asarray(many)[rng.integers(0, len(many), size=N)]
    labels[rng.random(N) < 0.15] = -1
    labels[rng.integers(0, N)] = K - 1
    return labels.astype(np.int64)


def _integers(X, labels, K):
    nz = np.stack([(X[labels == k] > 0).sum(0) for k in range(K)]).astype(np.int64)
    cs = np.stack([X[labels == k].astype(np.int64).sum(0) for k in range(K)])
    return nz, cs


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize("K", GROUPS)
@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("N,G", SHAPES)
def test_sums_bit_for_bit(N, G, view, K):
    from prosstt_amd import markers
    X, s = _host(N, G)
    labels = _labels(N, K)
    A = _a32(N, G)
    nz, cs = _integers(X, labels, K)
    n_sel = int((labels >= 0).sum())
    for rpb in ROWS_PER_BLOCK:
        gm = markers.group_moments(_view(N, G, view), s, labels, rows_per_block=rpb)
        assert list(gm.groups) == list(range(K)) and np.array_equal(gm.n, np.bincount(labels[labels >= 0], minlength=K))
        assert np.array_equal(gm.nonzero, nz) and np.array_equal(gm.count_sum, cs), rpb     # the same for every rows_per_block
        S1, S2, _ = mm.sums(A, labels, rpb or mm.default_rows_per_block(n_sel, G), K)
        assert _same_bits(gm.s1, S1) and _same_bits(gm.s2, S2), rpb
    if K >= 3:
        assert gm.n[1] == 0 and not gm.s1[1].any() and not gm.count_sum[1].any()             # an empty group gives zeros


@pytest.mark.parametrize("rpb", [0, 64])
def test_presented_counts(rpb):
    """Rows permuted: the labels follow the cells, the sums take each group's rows in the order they lie in."""
    import torch
    from prosstt_amd import device, markers
    N, G, K = 259, 1025, 3
    X, s = _host(N, G)
    labels = _labels(N, K)
    cell_of_row = np.random.default_rng(N).permutation(N)
    presented = device.PresentedCounts(torch.as_tensor(X[cell_of_row]).cuda(), cell_of_row)
    gm = markers.group_moments(presented, s, labels, rows_per_block=rpb)
    nz, cs = _integers(X, labels, K)
    assert np.array_equal(gm.nonzero, nz) and np.array_equal(gm.count_sum, cs) and np.array_equal(gm.codes, labels)
    S1, S2, _ = mm.sums(_a32(N, G)[cell_of_row], labels[cell_of_row], rpb or mm.default_rows_per_block(int((labels >= 0).sum()), G), K)
    assert _same_bits(gm.s1, S1) and _same_bits(gm.s2, S2)


@pytest.mark.parametrize("N,G", [(259, 1025), (300, 2051)])
def test_against_binary64(N, G):
    from prosstt_amd import markers
    X, s = _host(N, G)
    K = 3
    labels = np.arange(N) % K
    gm = markers.group_moments(_view(N, G, "aligned"), s, labels)
    A = mm.dense(X, s)
    worst = [0.0, 0.0]
    for k in range(K):
        a = A[labels == k]
        n = len(a)
        for i, (got, terms, entry) in enumerate(((gm.s1[k], a, 2.0 ** -20), (gm.s2[k], a * a, 2.0 ** -19 + 2.0 ** -39))):
            want, mass = terms.sum(0), np.abs(terms).sum(0)
            bound = (entry + n * 2.0 ** -52) * mass
            err = np.abs(got - want)
            worst[i] = max(worst[i], float(np.max(err[mass > 0] / mass[mass > 0])))
            assert np.all(err <= bound), (k, float(np.max(err - bound)))
    print("%d x %d: max |S1 - sum a| / sum |a| = 2^%.2f (bound 2^-20), max |S2 - sum a^2| / sum a^2 = 2^%.2f (bound 2^-19)"
          % (N, G, np.log2(worst[0]), np.log2(worst[1])))


def test_across_libraries():
    """Every cell labelled: the groups add up to count_summary's exact gene sums and zeros and to embed's gene moments."""
    from prosstt_amd import embed, markers, summary
    N, G, K = 300, 2051, 7
    X, s = _host(N, G)
    Xd = _view(N, G, "shifted")
    gm = markers.group_moments(Xd, s, np.arange(N) % K)
    cs = summary.count_summary(Xd)
    assert np.array_equal(gm.count_sum.sum(0), cs.gene_sum) and np.array_equal(N - gm.nonzero.sum(0), cs.gene_zeros)
    S1, S2 = embed.LogNormalized(Xd, s).gene_moments()
    A = _a32(N, G).astype(np.float64)
    # both add the same entries, each within n 2^-53 sum |a| of the exact sum; the K-term sum on the host adds K roundings
    for got, want, mass in ((gm.s1.sum(0), S1, np.abs(A).sum(0)), (gm.s2.sum(0), S2, (A * A).sum(0))):
        assert np.all(np.abs(got - want) <= (N + K) * 2.0 ** -52 * mass)


def _tree_sample():
    from prosstt_amd import simulation as sim, workloads
    if "tree" not in _cache:
        work = workloads.build("C2", G=300)
        np.random.seed(10)          # (a plan and a sampler seed for which the model's scores have no ties within a group)
        _cache["tree"] = sim.sample_density(work.tree, 600, alpha=work.alpha, beta=work.beta, seed=10, out="torch")
    return _cache["tree"]


def test_whole_call_on_a_sampled_tree():
    from prosstt_amd import device, markers
    X, pt, br, sc = _tree_sample()
    assert isinstance(X, device.PresentedCounts) and len(np.unique(br)) == 3
    res = markers.rank_genes_groups(X, sc, br)
    gm = res.moments
    assert list(res.groups) == list(np.unique(br)) and gm.n.sum() == 600
    want = mm.statistics(gm.s1, gm.s2, gm.nonzero, gm.n)
    for row in want["t"]:
        assert len(np.unique(row)) == row.size                     # no ties: the ranking is determined
    names = mm.rank(want["t"])
    assert np.array_equal(res.names, names)
    for field, key in (("scores", "t"), ("pvals", "pvals"), ("logfoldchanges", "logfoldchanges"), ("pvals_adj", "pvals_adj")):
        np.testing.assert_allclose(getattr(res, field), np.take_along_axis(want[key], names, 1), rtol=1e-12, atol=0, err_msg=field)
    # the sums themselves: the integers against the host matrix in plan order
    host = X.to_host("numpy32")
    codes = np.unique(br, return_inverse=True)[1]
    nz, cs = _integers(host, codes, 3)
    assert np.array_equal(gm.nonzero, nz) and np.array_equal(gm.count_sum, cs)
    np.testing.assert_allclose(gm.pseudobulk(sc), cs / np.bincount(codes, weights=sc)[:, None], rtol=1e-15)
    top = markers.rank_genes_groups(gm, n_genes=10, method="t-test_overestim_var", reference=res.groups[0])
    assert top.names.shape == (3, 10)


def test_planted_markers_on_the_device():
    import torch
    from prosstt_amd import markers
    X, s, labels = planted_case()
    res = markers.rank_genes_groups(torch.as_tensor(X).cuda(), s, labels, n_genes=10)
    assert set(res.names[1]) == set(range(10))
    assert np.all(res.pvals_adj[1] < 1e-20) and np.all(res.logfoldchanges[1] > 2.5)


def test_equal_bits_across_calls_and_streams():
    import torch
    from prosstt_amd import markers
    N, G = 300, 2051
    X, s = _host(N, G)
    labels = _labels(N, 7)
    first = markers.group_moments(_view(N, G, "aligned"), s, labels, out="torch")
    again = markers.group_moments(_view(N, G, "aligned"), s, labels, out="torch")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = markers.group_moments(_view(N, G, "aligned"), s, labels, out="torch")
    side.synchronize()
    for a in ("nonzero", "count_sum", "s1", "s2"):
        x = getattr(first, a)
        assert x.is_cuda and x.shape == (7, G)
        for y in (getattr(again, a), getattr(other, a)):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), a


def test_a_negative_count_raises():
    import torch
    from prosstt_amd import markers
    N, G = 130, 1024
    X, s = _host(N, G)
    bad = torch.as_tensor(X).cuda()
    bad[N - 1, G - 1] = -1
    labels = np.arange(N) % 3
    with pytest.raises(ValueError, match="negative"):
        markers.group_moments(bad, s, labels)
    labels[N - 1] = -1                                             # the row is not selected: nothing reads it
    markers.group_moments(bad, s, labels)


def test_refusals_of_the_abi():
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load("markers")
    N, G, K = 67, 1023, 3
    X = _view(N, G, "aligned")
    inv = torch.ones(N, dtype=torch.float32, device="cuda")
    rows = torch.arange(N, dtype=torch.int32, device="cuda")
    start = torch.tensor([0, 20, 20, N], dtype=torch.int64, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_markers_workspace_bytes(N, G, K, 0, ctypes.byref(need)), "markers")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = [torch.empty((K, G), dtype=t, device="cuda") for t in (torch.int64, torch.int64, torch.float64, torch.float64)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(N=N, G=G, ld=X.stride(0), n_sel=N, K=K, rpb=0, bytes_=need.value):
        return L.prosstt_amd_markers_group_moments(None, _ptr(X), N, G, ld, _ptr(inv), _ptr(rows), n_sel, _ptr(start), K, rpb,
                                                   _ptr(ws), bytes_, *[_ptr(o) for o in out], _ptr(status))

    assert call() == 0
    for kw, text in ((dict(K=1025), "groups"), (dict(K=0), "groups"), (dict(bytes_=need.value - 1), "workspace"),
                     (dict(ld=G - 1), "row stride"), (dict(N=0), "N"), (dict(N=1 << 31), "N"), (dict(n_sel=N + 1), "selected"),
                     (dict(n_sel=-1), "n_sel"), (dict(rpb=-1), "rows_per_block"), (dict(G=0), "G")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(call(**kw), "markers")
    for sizes, text in (((70000, G, K, 1), "blocks"), ((N, G, 1025, 0), "groups"), ((N, 0, K, 0), "G")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_markers_workspace_bytes(*sizes, ctypes.byref(need)), "markers")
    torch.cuda.synchronize()
    assert int(status.item()) == 0


def test_a_row_outside_the_matrix_and_bad_offsets_are_reported():
    """The C ABI's own guards (markers.py builds both arrays itself): a row index outside [0, N) is not read and sets a bit;
    offsets that do not ascend from 0 to n_sel are clamped and set another."""
    import torch
    from prosstt_amd import _native, markers
    from prosstt_amd.device import _ptr
    L = _native.load("markers")
    N, G, K = 67, 1023, 2
    X = _view(N, G, "aligned")
    host = _host(N, G)[0]
    inv = torch.ones(N, dtype=torch.float32, device="cuda")
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_markers_workspace_bytes(N, G, K, 4, ctypes.byref(need)), "markers")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = [torch.empty((K, G), dtype=t, device="cuda") for t in (torch.int64, torch.int64, torch.float64, torch.float64)]
    for rows, start, want in (([0, 1, N, 3, 4, 5, -1, 7, 8], [0, 5, 9], markers.ROW_RANGE),
                              ([0, 1, 2, 3, 4, 5, 6, 7, 8], [0, 12, 9], markers.GROUP_RANGE),
                              ([0, 1, 2, 3, 4, 5, 6, 7, 8], [-3, 4, 1 << 40], markers.GROUP_RANGE)):
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        r = torch.tensor(rows, dtype=torch.int32, device="cuda")
        st = torch.tensor(start, dtype=torch.int64, device="cuda")
        _native.check(L.prosstt_amd_markers_group_moments(None, _ptr(X), N, G, X.stride(0), _ptr(inv), _ptr(r), len(rows), _ptr(st), K,
                                                          4, _ptr(ws), need.value, *[_ptr(o) for o in out], _ptr(status)), "markers")
        assert int(status.item()) == want
        if want == markers.ROW_RANGE:                              # the rows inside the matrix are summed all the same
            assert np.array_equal(out[1][0].cpu().numpy(), host[[0, 1, 3, 4]].astype(np.int64).sum(0))
            assert np.array_equal(out[1][1].cpu().numpy(), host[[5, 7, 8]].astype(np.int64).sum(0))
