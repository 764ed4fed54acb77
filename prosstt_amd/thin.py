"""
Binomial thinning of a count matrix, where it lies: on the device.  A count x is split at random into a part
y ~ Binomial(x, p) and the rest x - y.  Fit on one part, score on the other (molecular cross-validation, count splitting): for
a Poisson count the two parts are independent Poisson counts, and under the simulator's gamma-Poisson law they stay Poisson
given the entry's rate.  It chooses a knob that has no truth to be calibrated against:

    s = thin.split(X, 0.5, seed=1)                              # s.train + s.test == X, entry by entry
    sc_train, sc_test = s.sizes(sc)                             # means at unit size are comparable across the parts
    f = factors.glmpca(s.train, sc_train, 3, alpha=a, beta=b)
    thin.heldout(f, s.test, sc_test).total                      # the held-out quasi-log-likelihood
    thin.rank_curve(X, sc, (1, 2, 3, 4, 6), alpha=a, beta=b).best
    [thin.fold(X, 5, f, seed=1).test for f in range(5)]         # five parts that add up to X
    Xd, p = thin.downsample(X, total=2000)                      # every cell at an expected depth of at most 2000

libprosstt_amd_thin.so (include/prosstt_amd_thin.h, which holds the definition THIN-1) makes the one pass: a part is named by an
interval [lo, hi) of the grid 0 .. 65 536, trial t of the entry of cell c and gene g has a 16-bit uniform U_t that is a pure
function of (seed, c, g, t), and y counts the trials with lo <= U_t < hi.  So y ~ Binomial(x, (hi - lo) / 65 536), the parts of
disjoint intervals add up exactly, and nothing depends on where the entry lies, on the other entries of the call, on the stream
or on the launch: a matrix in chunks of cells (``cell_offset``), a slice of its genes (``gene_offset``) and a
``device.PresentedCounts`` (its ``cell_of_row`` names the cells) give every cell and gene the same bits.  Integer arithmetic
only.  There is no CPU fallback: host arrays are refused.

Counts above 2^24 (``MAX_COUNT``) and negative counts are refused (ValueError) after the pass.
"""
import ctypes
from typing import NamedTuple

import numpy as np

from . import _native
from . import device as _device
from .device import _ptr, _torch

GRID = 65536                    # PROSSTT_AMD_THIN_GRID
MAX_COUNT = 1 << 24             # PROSSTT_AMD_THIN_MAX_COUNT
NEGATIVE, OVER, RANGE = 1, 2, 4     # the bits of the status word
MAX_FOLDS = 64
OVER_ENTRY = "the count matrix has an entry above 2^24: thinning draws no count that large"


class Split:
    """``train`` and ``test``: two int32 device matrices (``device.PresentedCounts`` when the input was one) that add up to the
    input entry by entry; ``fraction``: the realised share of the train part, a multiple of 1 / 65 536."""

    def __init__(self, train, test, fraction):
        self.train, self.test, self.fraction = train, test, float(fraction)

    def sizes(self, sc):
        """(fraction sc, (1 - fraction) sc): the size factors of the two parts, so that a mean at unit size is the same in
        both."""
        sc = np.asarray(sc, dtype=np.float64)
        return self.fraction * sc, (1.0 - self.fraction) * sc

    def __repr__(self):
        return "Split(fraction=%r)" % self.fraction


class Heldout(NamedTuple):
    """``per_cell``: (N,) the quasi-log-likelihood of every cell's held-out counts, in plan order; ``total``: their sum."""
    per_cell: np.ndarray
    total: float


class RankCurve(NamedTuple):
    """``ks``; ``heldout`` and ``train``: per k the quasi-log-likelihood of the fit on the test and on the train part;
    ``best``: the k with the largest ``heldout`` (the first of equals).  Exact for Poisson counts (alpha = 0, beta = 1); with
    alpha > 0 the two parts of an entry share its gamma rate, so they are dependent given the means and ``best`` leans to a
    larger k than the truth: DESIGN.md, section 37, has the measurement."""
    ks: tuple
    heldout: np.ndarray
    train: np.ndarray
    best: int


# ----------------------------------------------------------------------------------------------------- the argument checks

def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _seed(seed):
    if not _is_int(seed) or not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64) (got %r)" % (seed,))
    return int(seed)


def _offset(value, name):
    if not _is_int(value) or not 0 <= int(value) < 1 << 62:
        raise ValueError("%s must be an integer in [0, 2^62) (got %r)" % (name, value))
    return int(value)


def _bound(value, n_cells, name):
    """(the one value or None, the per-cell uint32 array or None) of a bound of the interval, or raise."""
    torch = _torch()
    if _is_int(value):
        if not 0 <= int(value) <= GRID:
            raise ValueError("%s must lie on the grid 0 .. %d (got %d)" % (name, GRID, int(value)))
        return int(value), None
    if isinstance(value, (float, np.floating, bool, np.bool_)) or value is None:
        raise TypeError("%s is a grid integer 0 .. %d or one per cell, not %s" % (name, GRID, type(value).__name__))
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    a = np.asarray(value)
    if a.dtype.kind not in "iu":
        raise TypeError("%s is a grid integer 0 .. %d or one per cell, not an array of %s" % (name, GRID, a.dtype))
    if a.shape != (n_cells,):
        raise ValueError("%s needs one entry per cell: shape (%d,), not %s" % (name, n_cells, a.shape))
    if a.size and (int(a.min()) < 0 or int(a.max()) > GRID):
        raise ValueError("%s must lie on the grid 0 .. %d" % (name, GRID))
    return None, a.astype(np.uint32)


def _interval(lo, hi, n_cells):
    lo1, lo_n = _bound(lo, n_cells, "lo")
    hi1, hi_n = _bound(hi, n_cells, "hi")
    low = lo_n if lo_n is not None else lo1
    high = hi_n if hi_n is not None else hi1
    if np.any(np.asarray(low, dtype=np.int64) > np.asarray(high, dtype=np.int64)):
        raise ValueError("need lo <= hi: [lo, hi) is a half-open interval of the grid")
    return lo1, lo_n, hi1, hi_n


def _fraction_to_grid(fraction, what="fraction"):
    if isinstance(fraction, (bool, np.bool_)) or not isinstance(fraction, (int, float, np.integer, np.floating)):
        raise TypeError("%s is a number, not %s" % (what, type(fraction).__name__))
    if not 0.0 < float(fraction) < 1.0:
        raise ValueError("need 0 < %s < 1 (got %r)" % (what, fraction))
    return int(min(GRID - 1, max(1, round(float(fraction) * GRID))))


def fold_interval(K, fold):
    """(lo, hi) of the test part of fold ``fold`` of ``K``: [floor(fold 65536 / K), floor((fold + 1) 65536 / K)).  The K
    intervals tile the grid."""
    if not _is_int(K) or not 2 <= int(K) <= MAX_FOLDS:
        raise ValueError("need an integer 2 <= K <= %d folds (got %r)" % (MAX_FOLDS, K))
    if not _is_int(fold) or not 0 <= int(fold) < int(K):
        raise ValueError("need an integer 0 <= fold < %d (got %r)" % (int(K), fold))
    K, fold = int(K), int(fold)
    return fold * GRID // K, (fold + 1) * GRID // K


def downsample_grid(totals, total):
    """Per cell the grid value of p = min(1, total / totals), floored: min(65536, floor(65536 total / totals)) in integers; a cell
    without counts keeps p = 1."""
    t = np.asarray(totals)
    if t.ndim != 1 or t.dtype.kind not in "iu":
        raise TypeError("the cells' totals are a one-dimensional integer array")
    if t.size and int(t.min()) < 0:
        raise ValueError("a cell's total is negative")
    if not _is_int(total) or int(total) < 0:
        raise ValueError("total must be an integer >= 0 (got %r)" % (total,))
    total = int(total)
    return np.array([GRID if v <= total else (GRID * total) // v for v in t.tolist()], dtype=np.uint32).reshape(t.shape)


def _matrix(counts, who):
    m = _device.CountMatrix(counts, who)
    if m.N < 1 or m.G < 1:
        raise ValueError("%s needs at least one cell and one gene (got %d x %d)" % (who, m.N, m.G))
    if m.N >= 1 << 31:
        raise ValueError("%s takes fewer than 2^31 cells" % who)
    return m


def check_status(bits):
    if bits & NEGATIVE:
        raise ValueError(_device.NEGATIVE_ENTRY)
    if bits & OVER:
        raise ValueError(OVER_ENTRY)
    if bits:
        raise RuntimeError("the pass refused a row of its lo / hi tables (status %d)" % bits)


# ------------------------------------------------------------------------------------------------------- the device pass

def plan(N, G, x_ptr, ld, y_ptr, ldy, r_ptr=0, ldr=0):
    """(vec, strips, row_blocks, rows_per_block) of a call with these sizes and addresses (integers; ``r_ptr`` 0: no
    complement), as the library lays it out: ``vec`` is True when rows go in 16-byte pieces.  Needs the built library, not a
    device."""
    vec, strips, blocks, rows = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _native.check(_native.load("thin").prosstt_amd_thin_plan(
        int(N), int(G), ctypes.c_void_p(int(x_ptr)), int(ld), ctypes.c_void_p(int(y_ptr)), int(ldy),
        ctypes.c_void_p(int(r_ptr)) if r_ptr else None, int(ldr), ctypes.byref(vec), ctypes.byref(strips), ctypes.byref(blocks),
        ctypes.byref(rows)), "thin")
    return bool(vec.value), int(strips.value), int(blocks.value), int(rows.value)


def _enqueue(m, lo1, lo_n, hi1, hi_n, seed, complement, cell_offset, gene_offset, out=None):
    """The pass over the checked device view ``m``: (Y, R or None, status), int32 device tensors.  Per-cell bounds are in
    plan order.  ``out``: (Y, R) to write instead of new tensors (the ABI refuses an overlap with the input)."""
    L = _device.need_device("thin")
    torch = _torch()
    with torch.cuda.device(m.device):
        ids = None
        if m.cell_of_row is not None:
            ids = torch.as_tensor(m.cell_of_row + cell_offset).to(m.device)
            lo_n = None if lo_n is None else lo_n[m.cell_of_row]
            hi_n = None if hi_n is None else hi_n[m.cell_of_row]
        lo_t = None if lo_n is None else torch.as_tensor(lo_n.astype(np.int64)).to(device=m.device, dtype=torch.int32)
        hi_t = None if hi_n is None else torch.as_tensor(hi_n.astype(np.int64)).to(device=m.device, dtype=torch.int32)
        if out is None:
            Y = torch.empty((m.N, m.G), dtype=torch.int32, device=m.device)
            R = torch.empty((m.N, m.G), dtype=torch.int32, device=m.device) if complement else None
        else:
            Y, R = out
        status = torch.zeros(1, dtype=torch.int32, device=m.device)
        _native.check(L.prosstt_amd_thin_interval(
            m.stream(), _ptr(m.X), m.N, m.G, m.ld, ctypes.c_uint64(seed), _ptr(ids), cell_offset, gene_offset,
            lo1 if lo1 is not None else 0, hi1 if hi1 is not None else GRID, _ptr(lo_t), _ptr(hi_t), _ptr(Y),
            Y.stride(0) if m.N > 1 else m.G, _ptr(R), (R.stride(0) if m.N > 1 else m.G) if R is not None else 0, _ptr(status)),
            "thin")
    return Y, R, status


def _wrap(m, Y):
    return Y if m.cell_of_row is None or Y is None else _device.PresentedCounts(Y, m.cell_of_row)


def interval(X, lo, hi, *, seed=0, complement=False, cell_offset=0, gene_offset=0):
    """The part [lo, hi) of every count of an int32 device count matrix (a (cells, genes) torch tensor with unit column
    stride, or a ``device.PresentedCounts``) by THIN-1: a new contiguous int32 device tensor Y with
    Y[i][j] ~ Binomial(X[i][j], (hi - lo) / 65 536), and with ``complement=True`` the pair (Y, X - Y) from the same pass.  Both
    are wrapped in a ``device.PresentedCounts`` with the same ``cell_of_row`` when ``X`` was one.

    ``lo``, ``hi``: grid integers 0 <= lo <= hi <= 65 536, one for all cells or one per cell in plan order (a host array or a
    tensor of integers).  ``seed``: 0 .. 2^64 - 1.  The cell of row r is ``cell_offset`` + r (+ ``cell_of_row[r]`` for a
    presented matrix), the gene of column j is ``gene_offset`` + j: a chunk of cells or a slice of genes gets the bits it has
    in the whole matrix.  Runs on the current stream; waits for the pass's status word.

    Raises TypeError for a host matrix, another dtype or bounds that are not integers; ValueError for a CPU tensor, a
    non-unit column stride, no cells or genes, a bound off the grid, lo > hi, a per-cell array of another length, a bad
    seed or offset, a negative count and a count above 2^24."""
    m = _matrix(X, "thin.interval")
    bounds = _interval(lo, hi, m.N)
    seed, cell_offset, gene_offset = _seed(seed), _offset(cell_offset, "cell_offset"), _offset(gene_offset, "gene_offset")
    m.on_device()
    Y, R, status = _enqueue(m, *bounds, seed, bool(complement), cell_offset, gene_offset)
    check_status(int(status.item()))
    return (_wrap(m, Y), _wrap(m, R)) if complement else _wrap(m, Y)


def split(X, fraction=0.5, *, seed=0):
    """``Split`` of an int32 device count matrix: ``train`` is the part [0, k) with k = round(fraction 65 536) clipped to
    1 .. 65 535, ``test`` the rest, ``fraction`` the realised k / 65 536.  One pass: one read and two writes of the matrix.

    Raises what ``interval`` raises, TypeError for a fraction that is not a number and ValueError unless 0 < fraction < 1."""
    k = _fraction_to_grid(fraction)
    train, test = interval(X, 0, k, seed=seed, complement=True)
    return Split(train, test, k / GRID)


def fold(X, K, fold, *, seed=0):
    """The ``Split`` of fold ``fold`` of ``K`` (2 <= K <= 64): ``test`` is the part ``fold_interval(K, fold)``, ``train`` the
    rest, ``fraction`` the train part's share.  The K test parts of one seed add up to the matrix, entry by entry.

    Raises what ``interval`` raises and ValueError for K outside 2 .. 64 or a fold outside 0 .. K - 1."""
    lo, hi = fold_interval(K, fold)
    test, train = interval(X, lo, hi, seed=seed, complement=True)
    return Split(train, test, 1.0 - (hi - lo) / GRID)


def downsample(X, *, total=None, fraction=None, seed=0, totals=None):
    """(Y, p): the matrix with every cell i thinned by p_i, and the realised p (N,) in plan order, multiples of 1 / 65 536.

    ``total``: p_i = min(1, total / total_i) floored to the grid, with total_i from ``summary.count_summary(X)`` or from
    ``totals`` (one integer per cell in plan order).  ``fraction``: instead, one p for all cells or one per cell, floored to
    the grid.  This is BINOMIAL thinning: every molecule is kept with probability p_i on its own, so a cell's expected depth
    is p_i total_i (``total`` for a deeper cell) and its realised depth varies around it.  scanpy's
    ``pp.downsample_counts`` draws without replacement and makes the totals exact; that draw is not provided.

    Raises what ``interval`` raises, ValueError unless exactly one of ``total`` and ``fraction`` is given, for a fraction
    outside [0, 1] and for arrays of another length than the cells."""
    if (total is None) == (fraction is None):
        raise ValueError("give exactly one of total and fraction")
    m = _matrix(X, "thin.downsample")
    if total is not None:
        if totals is None:
            if not _is_int(total) or int(total) < 0:
                raise ValueError("total must be an integer >= 0 (got %r)" % (total,))
            from . import summary
            totals = summary.count_summary(X).cell_total
        totals = np.asarray(totals)
        if totals.shape != (m.N,):
            raise ValueError("totals needs one entry per cell: shape (%d,), not %s" % (m.N, totals.shape))
        hi = downsample_grid(totals, total)
    else:
        f = np.asarray(fraction, dtype=np.float64)
        if f.ndim > 1 or (f.ndim == 1 and f.shape != (m.N,)):
            raise ValueError("fraction is one number or one per cell: shape (%d,), not %s" % (m.N, f.shape))
        if not np.all((f >= 0.0) & (f <= 1.0)):
            raise ValueError("need 0 <= fraction <= 1")
        hi = np.broadcast_to(np.floor(f * GRID).astype(np.uint32), (m.N,)).copy()
    return interval(X, 0, hi, seed=seed), hi.astype(np.float64) / GRID


# --------------------------------------------------------------------------------------------- held-out likelihood, rank curve

def heldout(f, test, sc_test):
    """``Heldout`` of a ``factors.Factors`` on a held-out part: ``factors.cell_equations``' Q of ``test`` (an int32 device count
    matrix over the fit's cells and genes) with the size factors ``sc_test`` at the fit's intercept, scores and loadings, that
    is with the loadings (intercept | loadings) and the coefficients (1 | scores), every gene taken.  No pass of its own."""
    from . import factors
    if not isinstance(f, factors.Factors):
        raise TypeError("heldout takes a factors.Factors, not %s" % type(f).__name__)
    loadings = np.concatenate([np.asarray(f.intercept, dtype=np.float64)[:, None], f.loadings], axis=1)
    coef = np.concatenate([np.ones((f.scores.shape[0], 1)), f.scores], axis=1)
    q = np.asarray(factors.cell_equations(test, sc_test, loadings, coef, f.alpha, f.beta).q, dtype=np.float64)
    return Heldout(q, float(q.sum()))


def rank_curve(X, sc, ks, *, alpha, beta, fraction=0.5, seed=0, **glmpca_kwargs):
    """``RankCurve`` of an int32 device count matrix with size factors ``sc``: one ``split`` at ``fraction`` by ``seed``, then per
    k of ``ks`` one ``factors.glmpca`` on the train part with ``sizes(sc)[0]`` (``glmpca_kwargs`` go to it), scored by
    ``heldout`` on the test part with ``sizes(sc)[1]`` and on the train part.

    Raises what ``split`` and ``factors.glmpca`` raise, and ValueError for no k."""
    from . import factors
    ks = tuple(int(k) for k in ks)
    if not ks:
        raise ValueError("rank_curve needs at least one k")
    _fraction_to_grid(fraction)
    s = split(X, fraction, seed=seed)
    sc_train, sc_test = s.sizes(sc)
    held, train = [], []
    for k in ks:
        f = factors.glmpca(s.train, sc_train, k, alpha=alpha, beta=beta, **glmpca_kwargs)
        held.append(heldout(f, s.test, sc_test).total)
        train.append(heldout(f, s.train, sc_train).total)
    held = np.array(held)
    return RankCurve(ks, held, np.array(train), ks[int(np.argmax(held))])
