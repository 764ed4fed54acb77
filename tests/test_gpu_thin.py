"""-m gpu: libprosstt_amd_thin.so through prosstt_amd/thin.py against the numpy model of THIN-1 (tests/thin_model.py: every plane
of every trial, no shortcut), bit for bit: the part Y and the complement R of every case of tests/thin_cases.py (the shapes and
views, the planted counts, the scalar intervals and the per-cell tables, with and without the complement), one entry of 2^24
under one plane and under sixteen, the same bits for a matrix in chunks of cells, a slice of genes, a presented matrix and a
non-default stream, the folds' sum, and the refusals through the status word."""
import numpy as np
import pytest

import thin_cases as C
import thin_model as T

pytestmark = pytest.mark.gpu

_views = {}


def _view(N, G, view):
    import torch
    key = (N, G, view)
    if key not in _views:
        X = torch.as_tensor(C.counts(N, G)).cuda()
        off, ld = C.layout(N, G, view)
        if view == "aligned":
            assert X.data_ptr() % 16 == 0 and X.is_contiguous()
            _views[key] = X
        else:
            wide = torch.full((N, ld), 12345, dtype=torch.int32, device="cuda")
            wide[:, 1:1 + G] = X
            _views[key] = wide[:, 1:1 + G]
            assert _views[key].data_ptr() % 16 == off
    return _views[key]


def _host(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("case", list(C.CASES), ids=lambda c: "%dx%d-%s" % c)
def test_parts_and_complements_bit_for_bit(case):
    from prosstt_amd import thin
    N, G, view = case
    X = _view(N, G, view)
    want_x = C.counts(N, G).astype(np.int64)
    vec = C.CASES[case][0]
    for lo, hi in C.SCALAR_INTERVALS + [("tables", "tables")]:
        a, b = C.tables(N) if lo == "tables" else (lo, hi)
        want = C.model(N, G, lo, hi)
        Y = thin.interval(X, a, b)
        assert Y.dtype == X.dtype and tuple(Y.shape) == (N, G) and Y.is_contiguous()
        assert thin.plan(N, G, X.data_ptr(), X.stride(0) if N > 1 else G, Y.data_ptr(), G)[0] is vec
        assert np.array_equal(_host(Y), want), (lo, hi)
        Y2, R = thin.interval(X, a, b, complement=True)
        assert np.array_equal(_host(Y2), want) and np.array_equal(_host(R), want_x - want), (lo, hi)
    assert np.array_equal(C.model(N, G, 0, 65536), want_x) and not C.model(N, G, 12345, 12345).any()
    assert np.array_equal(C.model(N, G, 0, 32768) + C.model(N, G, 32768, 65536), want_x)


@pytest.mark.parametrize("value", C.PLANTED)
def test_one_by_one_holds_each_planted_count(value):
    import torch
    from prosstt_amd import thin
    X = torch.tensor([[value]], dtype=torch.int32, device="cuda")
    for lo, hi in ((0, 32768), (1, 65536), (777, 30001)):
        Y, R = thin.interval(X, lo, hi, seed=5, complement=True, cell_offset=3, gene_offset=9)
        want = T.interval(np.array([[value]]), lo, hi, seed=5, cell_ids=[3], gene_ids=[9])
        assert int(Y) == int(want[0, 0]) and int(R) == value - int(want[0, 0])


@pytest.mark.parametrize("lo,hi,planes", [(0, 32768, 1), (1, 65536, 16)])
def test_the_largest_count(lo, hi, planes):
    """A matrix of its own: 2^24 trials, 2^18 words of 64, beside a few small counts."""
    import torch
    from prosstt_amd import thin
    assert T.planes_needed(lo, hi) == planes
    host = np.array([[3, 0, T.MAX_COUNT], [64, 1, 0]], dtype=np.int32)
    Y, R = thin.interval(torch.as_tensor(host).cuda(), lo, hi, seed=2, complement=True)
    want = T.interval(host, lo, hi, seed=2)
    assert np.array_equal(_host(Y), want) and np.array_equal(_host(R), host - want)


def test_the_same_bits_in_chunks_slices_presentations_and_streams():
    import torch
    from prosstt_amd import device, thin
    N, G = 259, 1025
    X = _view(N, G, "aligned")
    lo, hi = C.tables(N)
    want = C.model(N, G, "tables", "tables")
    # two chunks of rows
    top = thin.interval(X[:100], lo[:100], hi[:100])
    rest = thin.interval(X[100:], lo[100:], hi[100:], cell_offset=100)
    assert np.array_equal(_host(top), want[:100]) and np.array_equal(_host(rest), want[100:])
    # a slice of the genes: a view with the whole matrix's row stride
    part = thin.interval(X[:, 300:1025], lo, hi, gene_offset=300)
    assert np.array_equal(_host(part), want[:, 300:])
    part = thin.interval(X[:, 4:28], 0, 32768, gene_offset=4)
    assert np.array_equal(_host(part), C.model(N, G, 0, 32768)[:, 4:28])
    # rows permuted: per cell the same
    perm = np.random.default_rng(3).permutation(N)
    presented = device.PresentedCounts(X[torch.as_tensor(perm).cuda()].contiguous(), perm)
    Y, R = thin.interval(presented, lo, hi, complement=True)
    assert isinstance(Y, device.PresentedCounts) and isinstance(R, device.PresentedCounts)
    assert np.array_equal(Y.cell_of_row, perm) and np.array_equal(_host(Y.in_plan_order()), want)
    assert np.array_equal(_host(R.in_plan_order()), C.counts(N, G) - want)
    s = thin.split(presented, 0.5)
    assert np.array_equal(_host(s.train.in_plan_order()), C.model(N, G, 0, 32768))
    # a stream of its own
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        other = thin.interval(X, lo, hi)
    stream.synchronize()
    assert np.array_equal(_host(other), want)
    # another seed gives other bits
    assert not np.array_equal(_host(thin.interval(X, lo, hi, seed=1)), want)


def test_split_fold_and_downsample():
    from prosstt_amd import summary, thin
    N, G = 259, 1025
    X = _view(N, G, "shifted")
    host = C.counts(N, G).astype(np.int64)
    s = thin.split(X, 0.25, seed=0)
    assert s.fraction == 0.25 and np.array_equal(_host(s.train), C.model(N, G, 0, 16384))
    assert np.array_equal(_host(s.train) + _host(s.test), host)
    # the five folds of one seed add up to X on the device
    folds = [thin.fold(X, 5, f, seed=7) for f in range(5)]
    total = folds[0].test.clone()
    for f in folds[1:]:
        total += f.test
    assert bool((total == X).all())
    for f, piece in enumerate(folds):
        lo, hi = thin.fold_interval(5, f)
        assert piece.fraction == 1.0 - (hi - lo) / 65536 and bool((piece.train + piece.test == X).all())
    assert np.array_equal(_host(folds[2].test), T.interval(host, *thin.fold_interval(5, 2), seed=7))
    # downsample: the per-cell table from the exact totals
    totals = host.sum(axis=1)
    assert np.array_equal(summary.count_summary(X).cell_total, totals)
    target = int(np.median(totals))
    Y, p = thin.downsample(X, total=target, seed=4)
    grid = thin.downsample_grid(totals, target)
    assert np.array_equal(p, grid / 65536) and p.max() == 1.0 and p.min() < 1.0
    assert np.array_equal(_host(Y), T.interval(host, 0, grid.astype(np.int64), seed=4))
    deep = totals > target
    assert np.array_equal(_host(Y)[~deep], host[~deep])
    assert abs(_host(Y)[deep].sum(axis=1).mean() / target - 1.0) < 0.05
    Y2, p2 = thin.downsample(X, fraction=0.3, seed=4)
    assert np.all(p2 == np.floor(0.3 * 65536) / 65536)
    assert np.array_equal(_host(Y2), T.interval(host, 0, int(np.floor(0.3 * 65536)), seed=4))


def test_refusals_through_the_status_word():
    """A negative count and a count of 2^24 + 1 each raise and name the entry's kind; the entry is 0 in Y and in R and every
    other entry is still the model's.  An output that is the input is refused by the ABI."""
    import torch
    from prosstt_amd import _native, device, thin
    N, G = 3, 1024
    host = C.counts(N, G).astype(np.int64)
    want = T.interval(host, 777, 30001)
    for bad, bit, match in ((-1, thin.NEGATIVE, "negative entry"), (T.MAX_COUNT + 1, thin.OVER, r"above 2\^24")):
        planted = host.copy()
        planted[1, 500] = bad
        X = torch.as_tensor(planted.astype(np.int32)).cuda()
        with pytest.raises(ValueError, match=match):
            thin.interval(X, 777, 30001)
        m = thin._matrix(X, "test").on_device()
        Y, R, status = thin._enqueue(m, 777, None, 30001, None, 0, True, 0, 0)
        assert int(status.item()) == bit
        others = np.ones((N, G), dtype=bool)
        others[1, 500] = False
        assert int(Y[1, 500]) == 0 and int(R[1, 500]) == 0
        assert np.array_equal(_host(Y)[others], want[others]) and np.array_equal(_host(R)[others], (host - want)[others])
    # a row of the tables that is no interval: the status word's third bit, the row is 0
    X = _view(N, G, "aligned")
    m = thin._matrix(X, "test").on_device()
    Y, R, status = thin._enqueue(m, None, np.array([0, 9, 0], dtype=np.uint32), None, np.array([5, 3, 70000], dtype=np.uint32),
                                 0, True, 0, 0)
    assert int(status.item()) == thin.RANGE and not Y[1:].any() and not R[1:].any()
    assert np.array_equal(_host(Y)[0], T.interval(host, 0, 5)[0])
    # aliasing
    for out in ((X, None), (torch.empty_like(X), X), (X[:, :512], None)):
        with pytest.raises(_native.NativeError, match="overlap"):
            thin._enqueue(thin._matrix(X[:, :out[0].shape[1]], "test").on_device(), 0, None, 5, None, 0, out[1] is not None, 0, 0, out=out)
    assert device.NEGATIVE_ENTRY == "the count matrix has a negative entry"
