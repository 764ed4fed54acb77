"""
Highly variable genes, chosen where the count matrix lies: on the device.  The step of scanpy's tutorial between
normalisation and PCA (``pp.highly_variable_genes``), in its two usual flavours:

    hv = hvg.highly_variable_genes(X, n_top_genes=2000)                        # "seurat_v3": on the counts
    hv = hvg.highly_variable_genes(X, sc, n_top_genes=2000, flavor="seurat")   # on x / s, binned dispersions
    Xs = hvg.select_genes(X, hv.genes)                                         # a new (cells, 2000) device matrix
    pca = embed.pca(Xs, sc)                                                    # ... with the FULL matrix's size factors

libprosstt_amd_hvg.so (include/prosstt_amd_hvg.h) makes the passes over the int32 matrix: the exact sums of every gene's
counts on either side of the gene's own clip threshold, the binary64 sums of y = x / s and y^2, and the gather of the
chosen columns.  Everything else is O(genes) and runs on the host in binary64, except the local regression's weighted sums
(binary64 torch operations, on the matrix's device inside ``highly_variable_genes``).  Per-gene results do not depend on
the order of the rows, so a ``device.PresentedCounts`` is read as it lies.  There is no CPU fallback for the passes: host
arrays are refused.

``seurat_v3`` (N cells; needs counts, takes no size factors)
    1. from ``summary.count_summary``'s exact integers S1, S2, as Python ints rounded once:
       mean = S1 / N,  var = (N S2 - S1^2) / (N (N - 1))
    2. on the n genes with var > 0: x = log10(mean), y = log10(var) and a loess of y on x, fitted AT EACH GENE'S x:
       q = min(n, max(3, floor(span n + 1e-5))) neighbours, h the q-th smallest |x_i - x0|, tricube weights
       (1 - (d / h)^3)^3 inside h and 0 outside, weighted least squares on (1, u, u^2) with u = x - x0, the fitted value is
       the intercept; h = 0: the mean of y at the ties; a singular system: its minimum-norm solution (the intercept is the
       same for every least-squares solution, because x0 itself carries weight 1); no robustness iterations
    3. reg_std = sqrt(10^fit), 1 for constant genes;  clip = reg_std sqrt(N) + mean;  threshold = min(floor(clip), 2^31 - 1)
    4. with the device's ``ClippedSums`` for these thresholds (counts are integers: min(x, clip) is x up to the threshold and
       clip above it):  sum_c = sum_le + n_over clip,  sq_c = sumsq_le + n_over clip^2,
       variances_norm = (N mean^2 + sq_c - 2 sum_c mean) / ((N - 1) reg_std^2), 0 for constant genes
    5. the top ``n_top_genes`` by variances_norm; ties go to the lower gene index

``seurat`` (scanpy's default; needs ``size_factors``)
    1. from ``NormalizedMoments`` S1, S2 of y = x / s:  mean = S1 / N,  var = max(0, (S2 - S1 mean) / (N - 1)),  a mean of 0
       is replaced by 1e-12
    2. d = log(var / mean), NaN where var = 0;  m = log1p(mean)
    3. m in ``n_bins`` equal-width, right-closed bins over [min m, max m], the first edge lowered by 0.001 (max - min):
       ``pd.cut``'s edges
    4. per bin the mean and the ddof-1 standard deviation of the finite d; a bin with one gene: std = its mean, mean = 0
    5. dispersions_norm = (d - mean_bin) / std_bin
    6. the top ``n_top_genes`` by dispersions_norm with NaN last, or with ``n_top_genes=None`` the genes with
       min_mean < m < max_mean and min_disp < dispersions_norm < max_disp (a NaN fails both)

scanpy and skmisc are not installed here and were not run: the definitions are as remembered.  skmisc's loess interpolates
a fit made at the vertices of a kd-tree; this one fits directly at every gene.  The ``cell_ranger`` flavour and
``batch_key`` are not provided.

A matrix that arrives in chunks of cells is handled piece by piece (the pattern of ``markers.GroupMoments.concat``):

    cs = summary.CountSummary.concat([summary.count_summary(c) for c in chunks])
    fit = hvg.seurat_v3_fit(cs)
    clipped = hvg.ClippedSums.concat([hvg.clipped_sums(c, fit.thresholds) for c in chunks])
    hv = hvg.seurat_v3(cs, fit, clipped, 2000)
"""
from typing import NamedTuple

import numpy as np

from . import _native, embed, summary
from . import device as _device
from .device import _ptr, _torch

NEGATIVE, RANGE = 1, 2          # the bits of the status word (PROSSTT_AMD_HVG_NEGATIVE, PROSSTT_AMD_HVG_RANGE)
MAX_THRESHOLD = 2 ** 31 - 1
FLAVORS = ("seurat_v3", "seurat")
LOESS_CHUNK = 1 << 22           # entries of a (targets, neighbours) slab of the regression's weighted sums
LOESS_RCOND = 1e-13             # eigenvalues of the 3 x 3 normal matrix below this share of the largest count as 0


class HighlyVariable(NamedTuple):
    """``highly_variable``: (G,) bool; ``genes``: the selected indices, ascending; ``rank``: (G,) float, 0 for the best
    gene, NaN where not selected; ``means``, ``variances``: (G,) binary64 (of the counts for "seurat_v3", of x / s for
    "seurat", ddof 1); ``variances_norm`` for "seurat_v3", ``dispersions`` and ``dispersions_norm`` for "seurat" (None for
    the other flavour); ``flavor``."""
    highly_variable: np.ndarray
    genes: np.ndarray
    rank: np.ndarray
    means: np.ndarray
    variances: np.ndarray
    variances_norm: object
    dispersions: object
    dispersions_norm: object
    flavor: str


class SeuratV3Fit(NamedTuple):
    """``reg_std``, ``clip``: (G,) binary64; ``thresholds``: (G,) int64, floor(clip) capped at 2^31 - 1."""
    reg_std: np.ndarray
    clip: np.ndarray
    thresholds: np.ndarray


class ClippedSums:
    """Per gene the exact sums of the counts against the gene's threshold: ``n_over`` (int64: entries above it), ``sum_le``
    (int64: the sum of the others) and ``sumsq_le`` (their sum of squares: an object array of Python ints -- it can
    exceed 64 bits), over ``n_cells`` cells."""

    def __init__(self, n_cells, n_over, sum_le, sumsq_le):
        self.n_cells = int(n_cells)
        self.n_over = np.asarray(n_over, dtype=np.int64)
        self.sum_le = np.asarray(sum_le, dtype=np.int64)
        self.sumsq_le = np.array([int(v) for v in sumsq_le], dtype=object)
        self.n_genes = int(self.n_over.shape[0])
        if self.n_over.ndim != 1 or self.sum_le.shape != (self.n_genes,) or self.sumsq_le.shape != (self.n_genes,):
            raise ValueError("n_over, sum_le and sumsq_le must have one entry per gene")

    @classmethod
    def concat(cls, parts):
        """The sums of the matrices of ``parts`` stacked over cells (the same thresholds in every part): exact."""
        parts = _parts(parts, cls)
        sum_le = sum((p.sum_le.astype(object) for p in parts[1:]), parts[0].sum_le.astype(object))
        if len(sum_le) and max(sum_le) >= 1 << 63:
            raise OverflowError("a gene's sum exceeds int64")
        return cls(sum(p.n_cells for p in parts), sum((p.n_over for p in parts[1:]), parts[0].n_over),
                   [int(v) for v in sum_le], sum((p.sumsq_le for p in parts[1:]), parts[0].sumsq_le))

    def __repr__(self):
        return "ClippedSums(n_cells=%d, n_genes=%d)" % (self.n_cells, self.n_genes)


class NormalizedMoments:
    """Per gene the binary64 sums ``s1`` of y = x / s and ``s2`` of y^2 over ``n_cells`` cells."""

    def __init__(self, n_cells, s1, s2):
        self.n_cells = int(n_cells)
        self.s1 = np.asarray(s1, dtype=np.float64)
        self.s2 = np.asarray(s2, dtype=np.float64)
        self.n_genes = int(self.s1.shape[0])
        if self.s1.ndim != 1 or self.s2.shape != (self.n_genes,):
            raise ValueError("s1 and s2 must have one entry per gene")

    @classmethod
    def concat(cls, parts):
        """The sums of the matrices of ``parts`` stacked over cells: added in the order of the parts."""
        parts = _parts(parts, cls)
        s1, s2 = parts[0].s1.copy(), parts[0].s2.copy()
        for p in parts[1:]:
            s1 += p.s1
            s2 += p.s2
        return cls(sum(p.n_cells for p in parts), s1, s2)

    def __repr__(self):
        return "NormalizedMoments(n_cells=%d, n_genes=%d)" % (self.n_cells, self.n_genes)


def _parts(parts, cls):
    parts = list(parts)
    if not parts:
        raise ValueError("concat needs at least one part")
    for p in parts:
        if not isinstance(p, cls):
            raise TypeError("concat takes %s, not %s" % (cls.__name__, type(p).__name__))
    if len({p.n_genes for p in parts}) != 1:
        raise ValueError("the parts cover different numbers of genes")
    return parts


# ------------------------------------------------------------------------------------------------- the device passes

def _matrix(counts, who):
    """The checked device view (device.CountMatrix) of an accepted input, within the library's limits, or raise."""
    m = _device.CountMatrix(counts, who)
    if m.N < 1 or m.G < 1:
        raise ValueError("%s needs at least one cell and one gene (got %d x %d)" % (who, m.N, m.G))
    if m.N >= 1 << 31:
        raise ValueError("%s takes fewer than 2^31 cells" % who)
    return m.on_device()


def _thresholds(thresholds, n_genes):
    t = np.asarray(thresholds)
    if t.shape != (n_genes,):
        raise ValueError("need one threshold per gene: shape (%d,), not %s" % (n_genes, t.shape))
    if t.dtype.kind not in "iu":
        raise TypeError("thresholds are integers (floor of the clip value), not %s" % t.dtype)
    if t.size and (int(t.min()) < 0 or int(t.max()) > MAX_THRESHOLD):
        raise ValueError("thresholds must lie in [0, 2^31 - 1]")
    return t.astype(np.int32)


def clipped_sums(counts, thresholds):
    """``ClippedSums`` of an int32 device count matrix (a (cells, genes) torch tensor with unit column stride, or a
    ``device.PresentedCounts``) for one integer threshold per gene (a host array, each in [0, 2^31 - 1]).  Runs on the
    current stream; returns after one copy of O(genes) numbers.

    Raises TypeError for a host matrix, another dtype or non-integer thresholds, ValueError for a CPU tensor, a non-unit
    column stride, no cells or genes, a threshold outside its range or a negative count."""
    m = _matrix(counts, "clipped_sums")
    t = _thresholds(thresholds, m.G)
    L = _device.need_device("hvg")
    torch = _torch()
    with torch.cuda.device(m.device):
        ws = m.workspace("hvg", "prosstt_amd_hvg_workspace_bytes")
        thr = torch.as_tensor(t).to(m.device)
        G = m.G
        out = torch.empty(4 * G, dtype=torch.int64, device=m.device)           # n_over, sum_le, sumsq_le (low, high)
        status = torch.zeros(1, dtype=torch.int32, device=m.device)
        _native.check(L.prosstt_amd_hvg_clipped_sums(
            m.stream(), _ptr(m.X), m.N, G, m.ld, _ptr(thr), _ptr(ws), ws.numel(), _ptr(out[:G]), _ptr(out[G:2 * G]),
            _ptr(out[2 * G:]), _ptr(status)), "hvg")
        host = torch.cat([out, status.to(torch.int64)]).cpu().numpy()          # one synchronising copy
    _check_status(int(host[4 * G]))
    sq = host[2 * G:4 * G].view(np.uint64).reshape(G, 2)
    return ClippedSums(m.N, host[:G], host[G:2 * G], [(int(hi) << 64) | int(lo) for lo, hi in sq.tolist()])


def _check_status(bits):
    if bits & NEGATIVE:
        raise ValueError(_device.NEGATIVE_ENTRY)
    if bits:
        raise RuntimeError("the pass refused its thresholds or columns (status %d)" % bits)


def normalized_moments(counts, size_factors):
    """``NormalizedMoments`` of an int32 device count matrix and its size factors (one per cell in plan order, as for
    ``embed.LogNormalized``): y = (float)x * fl32(1 / s), the float32 product that embed's log1p entry starts from.  Runs on
    the current stream.

    Raises what ``embed.LogNormalized`` raises for the same arguments, and ValueError for a negative count."""
    op = embed.LogNormalized(counts, size_factors)
    L = _device.need_device("hvg")
    torch = _torch()
    N, G = op.shape
    with torch.cuda.device(op.device):
        ws = op.matrix.workspace("hvg", "prosstt_amd_hvg_workspace_bytes")
        S = torch.empty(2, G, dtype=torch.float64, device=op.device)
        _native.check(L.prosstt_amd_hvg_normalized_moments(
            op.matrix.stream(), _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(ws), ws.numel(), _ptr(S[0]),
            _ptr(S[1]), _ptr(op.status)), "hvg")
        _check_status(int(op.status.item()))
        S = S.cpu().numpy()
    return NormalizedMoments(N, S[0].copy(), S[1].copy())


def _gene_indices(genes, n_genes):
    """int32 indices of a bool mask over the genes or of an index array, or raise."""
    torch = _torch()
    if isinstance(genes, torch.Tensor):
        genes = genes.detach().cpu().numpy()
    g = np.asarray(genes)
    if g.ndim != 1:
        raise ValueError("genes must be one-dimensional, not %s" % (g.shape,))
    if g.size == 0:
        raise ValueError("no gene is selected")
    if g.dtype == np.bool_:
        if g.shape != (n_genes,):
            raise ValueError("a gene mask needs one entry per gene: shape (%d,), not %s" % (n_genes, g.shape))
        g = np.flatnonzero(g)
    elif g.dtype.kind not in "iu":
        raise TypeError("genes must be a bool mask or integer indices, not %s" % g.dtype)
    if g.size == 0:
        raise ValueError("no gene is selected")
    if int(g.min()) < 0 or int(g.max()) >= n_genes:
        raise ValueError("gene indices must lie in [0, %d)" % n_genes)
    return g.astype(np.int32)


def select_genes(counts, genes):
    """The columns ``genes`` (a bool mask over the genes, or indices in any order, repeats allowed) of an int32 device
    count matrix as a new contiguous (cells, n_sel) int32 device tensor -- wrapped in a ``device.PresentedCounts`` with the
    same ``cell_of_row`` when it was given one.  It is what ``embed.pca``, ``markers`` and ``ranks`` then take, with the FULL
    matrix's size factors.  Runs on the current stream and does not synchronise.

    Raises TypeError for a host matrix or another dtype, ValueError for a CPU tensor, a non-unit column stride, no cells,
    an empty selection or an index outside the genes."""
    m = _matrix(counts, "select_genes")
    idx = _gene_indices(genes, m.G)
    L = _device.need_device("hvg")
    torch = _torch()
    with torch.cuda.device(m.device):
        cols = torch.as_tensor(idx).to(m.device)
        Y = torch.empty((m.N, idx.size), dtype=torch.int32, device=m.device)
        status = torch.zeros(1, dtype=torch.int32, device=m.device)      # (the indices were checked on the host)
        _native.check(L.prosstt_amd_hvg_gather_columns(
            m.stream(), _ptr(m.X), m.N, m.G, m.ld, _ptr(cols), idx.size, _ptr(Y), idx.size, _ptr(status)), "hvg")
    return Y if m.cell_of_row is None else _device.PresentedCounts(Y, m.cell_of_row)


# --------------------------------------------------------------------------------------------------- host: seurat_v3

def _windows(xs, q):
    """For every entry of the ascending ``xs`` the start of a window of ``q`` consecutive entries that holds its q
    nearest: every entry outside the window is at least as far as the farthest inside.  It is the first start l at which
    the entry on the window's left end is no farther than the one just past its right end (the condition holds from some
    l on): a binary search for all entries at once."""
    n = xs.size
    lo = np.zeros(n, dtype=np.int64)
    hi = np.full(n, n - q, dtype=np.int64)
    while True:
        open_ = np.flatnonzero(lo < hi)
        if open_.size == 0:
            return lo
        mid = (lo[open_] + hi[open_]) // 2
        right = xs[open_] - xs[mid] > xs[mid + q] - xs[open_]
        lo[open_[right]] = mid[right] + 1
        hi[open_[~right]] = mid[~right]


def loess_fit(x, y, span=0.3, device=None):
    """The local quadratic regression of the module docstring of ``y`` on ``x``, fitted at every ``x``: binary64 numpy in
    and out.  The weighted sums run as binary64 torch operations on ``device`` (None: the host); the 3 x 3 normal equations
    of every point, in u / h, are solved on the host by a pseudo-inverse."""
    torch = _torch()
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 1 or y.shape != x.shape:
        raise ValueError("x and y must be one-dimensional and of equal length")
    if not 0 < span <= 1:
        raise ValueError("need 0 < span <= 1 (got %r)" % (span,))
    n = x.size
    if n == 0:
        return np.empty(0)
    q = min(n, max(3, int(np.floor(span * n + 1e-5))))
    order = np.argsort(x, kind="stable")
    xs, ys = x[order], y[order]
    left = _windows(xs, q)
    h = np.maximum(xs - xs[left], xs[left + q - 1] - xs)
    fit = np.empty(n)
    flat = h == 0
    if flat.any():                                     # the mean of y over the entries with this very x
        first = np.r_[True, xs[1:] != xs[:-1]]
        start = np.flatnonzero(first)
        mean = np.add.reduceat(ys, start) / np.diff(np.r_[start, n])
        fit[flat] = mean[(np.cumsum(first) - 1)[flat]]
    todo = np.flatnonzero(~flat)
    if todo.size:
        dev = torch.device("cpu") if device is None else device
        xt, yt = torch.as_tensor(xs).to(dev), torch.as_tensor(ys).to(dev)
        span_q = torch.arange(q, device=dev)
        sums = []
        rows = max(1, LOESS_CHUNK // q)
        for lo in range(0, todo.size, rows):
            at = torch.as_tensor(todo[lo:lo + rows]).to(dev)
            win = torch.as_tensor(left[todo[lo:lo + rows]]).to(dev)[:, None] + span_q[None, :]
            u = (xt[win] - xt[at][:, None]) / torch.as_tensor(h[todo[lo:lo + rows]]).to(dev)[:, None]
            w = (1.0 - u.abs() ** 3).clamp_min(0.0) ** 3
            yw = yt[win] * w
            wu = w * u
            wu2 = wu * u
            sums.append(torch.stack([w.sum(1), wu.sum(1), wu2.sum(1), (wu2 * u).sum(1), (wu2 * u * u).sum(1),
                                     yw.sum(1), (yw * u).sum(1), (yw * u * u).sum(1)], dim=1).cpu())
        s = torch.cat(sums).numpy()
        gram = s[:, [0, 1, 2, 1, 2, 3, 2, 3, 4]].reshape(-1, 3, 3)
        coef = np.einsum("kij,kj->ki", np.linalg.pinv(gram, rcond=LOESS_RCOND, hermitian=True), s[:, 5:8])
        fit[todo] = coef[:, 0]
    out = np.empty(n)
    out[order] = fit
    return out


def _count_moments(cs):
    """(N, mean, var) of a CountSummary: var with ddof 1, both from Python ints rounded once."""
    if not isinstance(cs, summary.CountSummary):
        raise TypeError("need a summary.CountSummary, not %s" % type(cs).__name__)
    n = cs.n_cells
    if n < 2:
        raise ValueError("highly variable genes need at least two cells (got %d)" % n)
    s1 = [int(v) for v in cs.gene_sum.tolist()]
    mean = np.array([v / n for v in s1], dtype=np.float64).reshape(cs.n_genes)
    var = np.array([(n * s2 - v * v) / (n * (n - 1)) for v, s2 in zip(s1, cs.gene_sumsq)],
                   dtype=np.float64).reshape(cs.n_genes)
    return n, mean, var


def seurat_v3_fit(count_summary, span=0.3, device=None):
    """``SeuratV3Fit`` (reg_std, clip, thresholds) of a ``summary.CountSummary``: steps 1 to 3 of "seurat_v3".  ``device``:
    where the regression's weighted sums run (None: the host)."""
    n, mean, var = _count_moments(count_summary)
    varying = var > 0
    reg_std = np.ones(mean.shape)
    if varying.any():
        fitted = loess_fit(np.log10(mean[varying]), np.log10(var[varying]), span, device)
        reg_std[varying] = np.sqrt(10.0 ** fitted)
    clip = reg_std * np.sqrt(n) + mean
    thresholds = np.minimum(np.floor(clip), float(MAX_THRESHOLD)).astype(np.int64)
    return SeuratV3Fit(reg_std, clip, thresholds)


def _check_top(n_top_genes, n_genes):
    if isinstance(n_top_genes, bool) or not isinstance(n_top_genes, (int, np.integer)) or not 1 <= n_top_genes <= n_genes:
        raise ValueError("need an integer 1 <= n_top_genes <= %d genes (got %r)" % (n_genes, n_top_genes))
    return int(n_top_genes)


def _top(score, n_top):
    """(mask, genes, rank) of the ``n_top`` largest scores: NaN last, ties to the lower index."""
    key = np.where(np.isnan(score), -np.inf, score)
    order = np.argsort(-key, kind="stable")[:n_top]
    return _selection(order, score.size)


def _selection(order, n_genes):
    mask = np.zeros(n_genes, dtype=bool)
    mask[order] = True
    rank = np.full(n_genes, np.nan)
    rank[order] = np.arange(order.size, dtype=np.float64)
    return mask, np.flatnonzero(mask), rank


def seurat_v3(count_summary, fit, clipped, n_top_genes):
    """``HighlyVariable`` by steps 4 and 5 of "seurat_v3": ``count_summary`` and ``clipped`` (the ``ClippedSums`` for
    ``fit.thresholds``) cover the same cells."""
    n, mean, var = _count_moments(count_summary)
    if not isinstance(fit, SeuratV3Fit):
        raise TypeError("fit must be a SeuratV3Fit, not %s" % type(fit).__name__)
    if not isinstance(clipped, ClippedSums):
        raise TypeError("clipped must be a ClippedSums, not %s" % type(clipped).__name__)
    G = count_summary.n_genes
    if clipped.n_genes != G or clipped.n_cells != n or fit.clip.shape != (G,) or fit.reg_std.shape != (G,):
        raise ValueError("the summary, the fit and the clipped sums cover different cells or genes")
    n_top = _check_top(n_top_genes, G)
    over = clipped.n_over.astype(np.float64)
    sum_c = clipped.sum_le.astype(np.float64) + over * fit.clip
    sq_c = np.array([float(v) for v in clipped.sumsq_le], dtype=np.float64).reshape(G) + over * fit.clip ** 2
    vn = (n * mean ** 2 + sq_c - 2.0 * sum_c * mean) / ((n - 1) * fit.reg_std ** 2)
    vn[~(var > 0)] = 0.0
    mask, genes, rank = _top(vn, n_top)
    return HighlyVariable(mask, genes, rank, mean, var, vn, None, None, "seurat_v3")


# ------------------------------------------------------------------------------------------------------ host: seurat

def _bin_of(m, n_bins):
    """``pd.cut(m, n_bins)``'s bin of every entry (right-closed; equal entries: pandas widens the range by 0.1 %)."""
    lo, hi = float(m.min()), float(m.max())
    if lo == hi:
        lo -= 0.001 * abs(lo) if lo != 0 else 0.001
        hi += 0.001 * abs(hi) if hi != 0 else 0.001
        edges = np.linspace(lo, hi, n_bins + 1)
    else:
        edges = np.linspace(lo, hi, n_bins + 1)
        edges[0] -= 0.001 * (hi - lo)
    return edges.searchsorted(m, side="left") - 1


def seurat(moments, n_top_genes=2000, *, n_bins=20, min_mean=0.0125, max_mean=3.0, min_disp=0.5, max_disp=np.inf):
    """``HighlyVariable`` by the "seurat" definition from a ``NormalizedMoments``; ``n_top_genes=None`` selects by the four
    cutoffs."""
    if not isinstance(moments, NormalizedMoments):
        raise TypeError("seurat takes a NormalizedMoments, not %s" % type(moments).__name__)
    n, G = moments.n_cells, moments.n_genes
    if n < 2:
        raise ValueError("highly variable genes need at least two cells (got %d)" % n)
    if G < 1:
        raise ValueError("no genes")
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or n_bins < 1:
        raise ValueError("need an integer n_bins >= 1 (got %r)" % (n_bins,))
    n_top = None if n_top_genes is None else _check_top(n_top_genes, G)
    mean = moments.s1 / n
    var = np.maximum(0.0, (moments.s2 - moments.s1 * mean) / (n - 1))
    mean_d = np.where(mean == 0, 1e-12, mean)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(var == 0, np.nan, np.log(var / mean_d))
    m = np.log1p(mean_d)
    which = _bin_of(m, int(n_bins))
    finite = np.isfinite(d)
    count = np.bincount(which[finite], minlength=int(n_bins)).astype(np.float64)
    total = np.bincount(which[finite], weights=d[finite], minlength=int(n_bins))
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_bin = total / count
        dev = np.where(finite, d - mean_bin[which], 0.0)
        std_bin = np.sqrt(np.bincount(which, weights=dev * dev, minlength=int(n_bins)) / (count - 1))
        std_bin[count < 2] = np.nan
        lone = np.isnan(std_bin)
        std_bin[lone] = mean_bin[lone]
        mean_bin = np.where(lone, 0.0, mean_bin)
        dn = (d - mean_bin[which]) / std_bin[which]
    if n_top is not None:
        mask, genes, rank = _top(dn, n_top)
    else:
        keep = (m > min_mean) & (m < max_mean) & (dn > min_disp) & (dn < max_disp)
        idx = np.flatnonzero(keep)
        mask, genes, rank = _selection(idx[np.argsort(-dn[idx], kind="stable")], G)
    return HighlyVariable(mask, genes, rank, mean, var, None, d, dn, "seurat")


# ---------------------------------------------------------------------------------------------------- the whole call

def highly_variable_genes(counts, size_factors=None, n_top_genes=2000, flavor="seurat_v3", *, span=0.3, n_bins=20,
                          min_mean=0.0125, max_mean=3.0, min_disp=0.5, max_disp=np.inf):
    """``HighlyVariable`` of an int32 device count matrix (a (cells, genes) torch tensor with unit column stride, or a
    ``device.PresentedCounts``) by the module docstring's definitions.

    ``flavor``: "seurat_v3" (on the counts; ``size_factors`` is not used; ``span``: the regression's share of the genes) or
    "seurat" (needs ``size_factors``, one per cell in plan order as for ``embed.pca``; ``n_bins`` and, with
    ``n_top_genes=None``, the four cutoffs).  Runs on the current stream.

    Raises TypeError for a host matrix or another dtype, ValueError for an unknown flavour, fewer than two cells, an
    ``n_top_genes`` outside [1, genes] (None is for "seurat" alone), "seurat" without size factors, and whatever the passes
    raise for the matrix (a CPU tensor, a non-unit column stride, a negative count)."""
    if flavor not in FLAVORS:
        raise ValueError("flavor must be one of %s (got %r)" % (", ".join(FLAVORS), flavor))
    m = _device.CountMatrix(counts, "highly_variable_genes")
    if m.N < 2:
        raise ValueError("highly variable genes need at least two cells (got %d)" % m.N)
    if m.G < 1:
        raise ValueError("highly_variable_genes needs at least one gene")
    if n_top_genes is None:
        if flavor != "seurat":
            raise ValueError("n_top_genes=None (selection by cutoffs) is for flavor='seurat' alone")
    else:
        _check_top(n_top_genes, m.G)
    if flavor == "seurat":
        if size_factors is None:
            raise ValueError("flavor='seurat' works on x / s: it needs size_factors")
        return seurat(normalized_moments(counts, size_factors), n_top_genes, n_bins=n_bins, min_mean=min_mean,
                      max_mean=max_mean, min_disp=min_disp, max_disp=max_disp)
    m.on_device()
    cs = summary.count_summary(counts)
    fit = seurat_v3_fit(cs, span, m.device)
    return seurat_v3(cs, fit, clipped_sums(counts, fit.thresholds), n_top_genes)
