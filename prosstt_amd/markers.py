"""
Marker genes of groups of cells, computed where the count matrix lies: on the device.  The step after ``dpt.dpt`` or any
clustering (scanpy's ``tl.rank_genes_groups`` with a t-test): which genes distinguish this arm from the rest?

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    mk = markers.rank_genes_groups(X, sc, br)             # or res.groups of dpt.dpt
    mk.names[k][:10]                                      # the ten genes that mark group mk.groups[k]
    gm = markers.group_moments(X, sc, br); gm.pseudobulk(sc)   # per-group sums, to compare with tree.means

The one pass over the cells x genes matrix runs in libprosstt_amd_markers.so (include/prosstt_amd_markers.h): per group and
gene the number of non-zero counts, the exact sum of counts and the binary64 sums of a and a^2, a = the float32 entry
log1p(x / s) of ``embed.LogNormalized``, bit for bit.  The sort by group, ``bincount`` and ``cumsum`` are torch's on the
input's stream.  The statistics are host numpy in binary64 on the K x G sums.  There is no CPU fallback for the pass.

scanpy is not installed here and was not run: the formulas are Welch's t-test as scipy states it (``scipy.stats.ttest_ind``
with ``equal_var=False``) and scanpy's conventions from memory (the "rest" of a group, ``t-test_overestim_var``, the fold
change of ``expm1`` of the means with 1e-9 added, Benjamini-Hochberg per group).

The statistics, for group 1 against group 2 -- the ``reference`` group or, for "rest", all other labelled cells (their sums
are the totals over every group minus group 1's, n2 = n_total - n1):

    m = S1 / n;  v = max((S2 - S1 S1 / n) / (n - 1), 0)
    vn1 = v1 / n1;  vn2 = v2 / n2 ("t-test") or v2 / n1 ("t-test_overestim_var")
    t = (m1 - m2) / sqrt(vn1 + vn2);  df = (vn1 + vn2)^2 / (vn1^2 / (n1 - 1) + vn2^2 / (n2 - 1))
    where vn1 + vn2 == 0: t = 0 and p = 1;  pvals = 2 scipy.stats.t.sf(|t|, df)
    pvals_adj: Benjamini-Hochberg over the genes of one group
    logfoldchanges = log2((expm1(m1) + 1e-9) / (expm1(m2) + 1e-9));  pts = nz1 / n1, pts_rest = nz2 / n2

Every group keeps its row (with a reference group, that group's own row compares it with itself: t = 0).

``method="wilcoxon"`` (``RANK_METHODS``) ranks by the Wilcoxon rank-sum z instead.  It cannot be computed from these sums: it
needs every gene's entries ranked, which ``prosstt_amd.ranks`` does on the device; ``rank_genes_groups`` runs both.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, embed
from . import device as _device
from .device import _ptr, _torch
from .layout import _number

MAX_GROUPS = 1024               # PROSSTT_AMD_MARKERS_MAX_GROUPS
METHODS = ("t-test", "t-test_overestim_var")
RANK_METHODS = ("wilcoxon",)    # ranked from the matrix itself, not from a GroupMoments: prosstt_amd/ranks.py
NEGATIVE, ROW_RANGE, GROUP_RANGE = 1, 2, 4       # the bits of the pass's status word


# --------------------------------------------------------------------------------------------------------- labels

def encode_labels(labels, n_cells):
    """(groups, codes): the categories and, per cell, the index of its category (int64; -1: the cell is left out).

    Integer labels are their own codes: the categories are 0 .. max, a value that no cell has is an empty category and a
    label below 0 leaves the cell out.  Any other labels (the simulation's branch names) are encoded with
    ``np.unique(return_inverse=True)``.  ValueError unless there is one label per cell."""
    torch = _torch()
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    arr = np.asarray(labels)
    if arr.shape != (n_cells,):
        raise ValueError("need one label per cell: shape (%d,), not %s" % (n_cells, arr.shape))
    if arr.dtype.kind in "iu":
        codes = np.where(arr < 0, -1, arr).astype(np.int64)
        groups = np.arange(int(codes.max()) + 1 if codes.size else 0, dtype=np.int64)
    elif arr.dtype.kind == "b" or arr.dtype.kind == "f":
        raise ValueError("labels must be integers or names, not %s" % arr.dtype)
    else:
        groups, codes = np.unique(arr, return_inverse=True)
        codes = codes.astype(np.int64).reshape(-1)
    if len(groups) < 1:
        raise ValueError("no cell has a label")
    if len(groups) > MAX_GROUPS:
        raise ValueError("at most %d groups (got %d)" % (MAX_GROUPS, len(groups)))
    return groups, codes


def codes_in_row_order(codes, cell_of_row):
    """The code of every ROW of a count input whose row i is cell ``cell_of_row[i]`` of the plan (None: row i is cell i):
    the labels are permuted, never the matrix."""
    return codes if cell_of_row is None else codes[np.asarray(cell_of_row, dtype=np.int64)]


# ----------------------------------------------------------------------------------------------------------- sums

def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


class GroupMoments:
    """The per-group sums of one call (or of several chunks, ``concat``).

    ``groups``: the K categories; ``n``: (K,) int64 cells per group; ``nonzero`` and ``count_sum``: (K, G) int64, the
    cells with a count above 0 and the exact sum of counts; ``s1``, ``s2``: (K, G) float64 sums of a and a^2, a =
    log1p(x / s) as ``embed.LogNormalized`` forms it; ``codes``: (cells,) int64, the group of every cell in plan order (-1:
    left out).  The four matrices are numpy arrays, or device tensors for ``out="torch"``; the rest lives on the host."""

    def __init__(self, groups, n, nonzero, count_sum, s1, s2, codes):
        self.groups = np.asarray(groups)
        self.n = np.asarray(n, dtype=np.int64)
        self.nonzero, self.count_sum, self.s1, self.s2 = nonzero, count_sum, s1, s2
        self.codes = np.asarray(codes, dtype=np.int64)
        K = len(self.groups)
        if self.n.shape != (K,):
            raise ValueError("n must have one entry per group")
        shapes = {tuple(a.shape) for a in (nonzero, count_sum, s1, s2)}
        if len(shapes) != 1 or len(next(iter(shapes))) != 2 or next(iter(shapes))[0] != K:
            raise ValueError("nonzero, count_sum, s1 and s2 must be (groups, genes) alike")

    @property
    def n_genes(self):
        return int(self.s1.shape[1])

    @staticmethod
    def concat(parts):
        """The sums over the cells of all ``parts`` (chunks of one matrix over cells, e.g. of ``sample_density_chunks``,
        with equal groups): added in list order, ``codes`` appended."""
        parts = list(parts)
        if not parts:
            raise ValueError("concat needs at least one GroupMoments")
        first = parts[0]
        for p in parts[1:]:
            if not np.array_equal(p.groups, first.groups):
                raise ValueError("the parts have different groups")
            if p.n_genes != first.n_genes:
                raise ValueError("the parts cover different numbers of genes")
        total = [first.n.copy(), first.nonzero, first.count_sum, first.s1, first.s2]
        for p in parts[1:]:
            for i, a in enumerate((p.n, p.nonzero, p.count_sum, p.s1, p.s2)):
                total[i] = total[i] + a
        return GroupMoments(first.groups, *total, np.concatenate([p.codes for p in parts]))

    def _columns(self):
        return self.n.astype(np.float64)[:, None]

    def means(self):
        """(K, G) mean of a per group (NaN for an empty group)."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return _host(self.s1) / self._columns()

    def variances(self):
        """(K, G) variance of a per group, ddof = 1, not below 0 (NaN for a group of fewer than two cells)."""
        n = self._columns()
        s1, s2 = _host(self.s1), _host(self.s2)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 1, np.maximum((s2 - s1 * s1 / n) / (n - 1), 0.0), np.nan)

    def fractions(self):
        """(K, G) share of a group's cells with a count above 0."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return _host(self.nonzero) / self._columns()

    def pseudobulk(self, size_factors):
        """(K, G) ``count_sum`` over the sum of the size factors of the group's cells (one factor per cell in plan order):
        the group's mean expression at unit size, what ``tree.means`` holds for a branch."""
        s = np.asarray(_host(size_factors), dtype=np.float64)
        if s.shape != self.codes.shape:
            raise ValueError("need one size factor per cell: shape %s, not %s" % (self.codes.shape, s.shape))
        keep = self.codes >= 0
        total = np.bincount(self.codes[keep], weights=s[keep], minlength=len(self.groups))
        with np.errstate(invalid="ignore", divide="ignore"):
            return _host(self.count_sum) / total[:, None]

    def __repr__(self):
        return "GroupMoments(groups=%d, genes=%d, cells=%d)" % (len(self.groups), self.n_genes, int(self.n.sum()))


def _rows_per_block(v):
    if not _number(v) or int(v) != v or not 0 <= v < 1 << 31:
        raise ValueError("need an integer 0 <= rows_per_block < 2^31 (got %r)" % (v,))
    return int(v)


def _row_list(codes, K, cell_of_row, dev):
    """(n, rows, start): the cells per group (host int64), and on ``dev`` the rows of the labelled cells sorted by group (int32,
    in the matrix's order within a group) with the K + 1 offsets of the groups in it (int64).  torch's sort, ``bincount`` and
    ``cumsum`` on the current stream."""
    torch = _torch()
    keep = codes >= 0
    n = np.bincount(codes[keep], minlength=K).astype(np.int64)
    n_sel = int(n.sum())
    key = torch.as_tensor(codes_in_row_order(np.where(keep, codes, K), cell_of_row)).to(dev)   # left out: last
    rows = torch.sort(key, stable=True).indices[:n_sel].to(torch.int32)
    start = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(torch.bincount(key, minlength=K + 1)[:K], 0)
    return n, rows, start


def group_moments(counts, size_factors, labels, *, rows_per_block=0, out="numpy"):
    """``GroupMoments`` of an int32 device count matrix for one label per cell.

    ``counts`` and ``size_factors``: as for ``embed.LogNormalized`` (a device tensor with unit column stride or a
    ``device.PresentedCounts``; positive host size factors per cell in plan order).  ``labels``: one per cell in plan order
    (``encode_labels``).  ``rows_per_block``: rows of the matrix per block of the pass, 0 for the library's rule; the
    integer sums do not depend on it, the float sums are equal to the bit for equal values.  ``out``: "numpy", or "torch"
    for device tensors.  Runs on the current stream.

    Raises TypeError for a host array or another dtype; ValueError for a CPU tensor, bad size factors, labels of another
    length, more than 1024 groups, a bad ``rows_per_block`` or ``out``, or a negative count."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    m = embed._counts(counts)
    groups, codes = encode_labels(labels, m.N)
    rows_per_block = _rows_per_block(rows_per_block)
    op = embed.LogNormalized(counts, size_factors)
    L = _device.need_device("markers")
    torch = _torch()
    N, G = op.shape
    K = len(groups)
    dev = op.device
    with torch.cuda.device(dev):
        n, rows, start = _row_list(codes, K, m.cell_of_row, dev)
        n_sel = int(n.sum())
        ws = _device.workspace("markers", "prosstt_amd_markers_workspace_bytes", dev, n_sel, G, K, rows_per_block)
        ints = torch.empty((2, K, G), dtype=torch.int64, device=dev)
        sums = torch.empty((2, K, G), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_markers_group_moments(
            _device.current_stream(dev), _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(rows) if n_sel else None, n_sel,
            _ptr(start), K, rows_per_block, _ptr(ws), ws.numel(), _ptr(ints[0]), _ptr(ints[1]), _ptr(sums[0]), _ptr(sums[1]),
            _ptr(status)), "markers")
        bits = int(status.item())
        if bits & NEGATIVE:
            raise ValueError(_device.NEGATIVE_ENTRY)
        if bits:
            raise RuntimeError("the grouped pass refused its row list (status %d)" % bits)
        if out == "numpy":
            ints, sums = ints.cpu().numpy(), sums.cpu().numpy()
    return GroupMoments(groups, n, ints[0], ints[1], sums[0], sums[1], codes)


# ------------------------------------------------------------------------------------------------------ statistics

class Statistics(NamedTuple):
    """(K, G) binary64 arrays per group and gene: ``scores`` (t), ``df``, ``pvals``, ``pvals_adj``, ``logfoldchanges``,
    ``pts``, ``pts_rest``; ``groups``: the K categories."""
    groups: np.ndarray
    scores: np.ndarray
    df: np.ndarray
    pvals: np.ndarray
    pvals_adj: np.ndarray
    logfoldchanges: np.ndarray
    pts: np.ndarray
    pts_rest: np.ndarray


def benjamini_hochberg(p):
    """Benjamini-Hochberg adjusted p-values along the last axis: p_(i) G / i, made monotone from the largest down, at
    most 1."""
    p = np.asarray(p, dtype=np.float64)
    G = p.shape[-1]
    order = np.argsort(p, axis=-1, kind="stable")
    ranked = np.take_along_axis(p, order, -1) * G / np.arange(1, G + 1)
    ranked = np.minimum(np.minimum.accumulate(ranked[..., ::-1], axis=-1)[..., ::-1], 1.0)
    adj = np.empty_like(p)
    np.put_along_axis(adj, order, ranked, -1)
    return adj


def _reference_index(groups, reference):
    if isinstance(reference, str) and reference == "rest":
        return None
    at = [] if isinstance(reference, bool) else [i for i, g in enumerate(groups.tolist()) if g == reference]
    if len(at) != 1:
        raise ValueError("reference must be 'rest' or one of the groups (got %r)" % (reference,))
    return at[0]


def _bad_method(method, allowed=METHODS):
    if method in RANK_METHODS:
        return ("method %r is a rank test: it needs the matrix, not the sums of a GroupMoments "
                "(rank_genes_groups(counts, size_factors, labels, method=%r))" % (method, method))
    return "method must be one of %s (got %r)" % (", ".join(allowed), method)


def statistics(gm, reference="rest", method="t-test"):
    """``Statistics`` of a ``GroupMoments`` by the module docstring's formulas, host numpy in binary64.

    Raises ValueError for an unknown ``method`` or ``reference``, and for a group, or a rest, of fewer than two cells."""
    import scipy.stats
    if not isinstance(gm, GroupMoments):
        raise TypeError("statistics takes a GroupMoments, not %s" % type(gm).__name__)
    if method not in METHODS:
        raise ValueError(_bad_method(method))
    ref = _reference_index(gm.groups, reference)
    n1 = gm.n.astype(np.float64)
    if np.any(gm.n < 2):
        raise ValueError("every group needs at least two cells (group %r has %d)"
                         % (gm.groups[int(np.argmax(gm.n < 2))], int(gm.n[int(np.argmax(gm.n < 2))])))
    s1, s2, nz = _host(gm.s1), _host(gm.s2), _host(gm.nonzero).astype(np.float64)
    if ref is None:
        n2 = n1.sum() - n1
        if np.any(n2 < 2):
            raise ValueError("the rest of every group needs at least two cells")
        r1, r2, rz = s1.sum(0)[None, :] - s1, s2.sum(0)[None, :] - s2, nz.sum(0)[None, :] - nz
    else:
        n2 = np.full_like(n1, n1[ref])
        r1, r2, rz = (np.broadcast_to(a[ref], a.shape) for a in (s1, s2, nz))
    n1, n2 = n1[:, None], n2[:, None]
    m1, m2 = s1 / n1, r1 / n2
    v1 = np.maximum((s2 - s1 * s1 / n1) / (n1 - 1), 0.0)
    v2 = np.maximum((r2 - r1 * r1 / n2) / (n2 - 1), 0.0)
    vn1 = v1 / n1
    vn2 = v2 / (n2 if method == "t-test" else n1)
    flat = vn1 + vn2 == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(flat, 0.0, (m1 - m2) / np.sqrt(vn1 + vn2))
        df = (vn1 + vn2) ** 2 / (vn1 ** 2 / (n1 - 1) + vn2 ** 2 / (n2 - 1))
        p = np.where(flat, 1.0, 2.0 * scipy.stats.t.sf(np.abs(t), np.where(flat, 1.0, df)))
    lfc = np.log2((np.expm1(m1) + 1e-9) / (np.expm1(m2) + 1e-9))
    return Statistics(gm.groups, t, df, p, benjamini_hochberg(p), lfc, nz / n1, rz / n2)


class RankGenesGroups(NamedTuple):
    """``groups``: the K categories; ``names``: (K, n) int64 gene indices by score descending, ties to the lower index;
    ``scores``, ``logfoldchanges``, ``pvals``, ``pvals_adj``, ``pts``, ``pts_rest``: (K, n) float64 in ``names`` order;
    ``moments``: the ``GroupMoments`` they come from."""
    groups: np.ndarray
    names: np.ndarray
    scores: np.ndarray
    logfoldchanges: np.ndarray
    pvals: np.ndarray
    pvals_adj: np.ndarray
    pts: np.ndarray
    pts_rest: np.ndarray
    moments: Any


def rank_genes_groups(counts, size_factors=None, labels=None, *, reference="rest", method="t-test", tie_correct=False,
                      n_genes=None, out="numpy"):
    """The genes of every group ranked by their score against ``reference`` (the module docstring's t, or for
    ``method="wilcoxon"`` the z of ``prosstt_amd.ranks``): ``RankGenesGroups``.

    ``counts``, ``size_factors``, ``labels``, ``out``: as for ``group_moments`` (``out`` names where the moments stay; the
    ranking is host numpy); or a ``GroupMoments`` as the only positional argument (t-tests only: a rank test needs the
    matrix).  ``reference``: "rest" or a group; ``method``: "t-test", "t-test_overestim_var" or "wilcoxon"; ``tie_correct``:
    for "wilcoxon" against the rest, the variance with its tie term (``ranks.wilcoxon``); ``n_genes``: how many to keep per
    group, 1 .. genes (None: all).

    Raises what ``group_moments``, ``statistics``, ``ranks.rank_sums`` and ``ranks.wilcoxon`` raise, and ValueError for
    ``n_genes`` out of range; the argument checks come before any device use."""
    if method not in METHODS + RANK_METHODS:
        raise ValueError(_bad_method(method, METHODS + RANK_METHODS))
    ranked = method in RANK_METHODS
    if not isinstance(tie_correct, (bool, np.bool_)):
        raise ValueError("tie_correct must be True or False (got %r)" % (tie_correct,))
    if tie_correct and not ranked:
        raise ValueError("tie_correct belongs to method='wilcoxon', not to %r" % (method,))
    if isinstance(counts, GroupMoments):
        if ranked:
            raise ValueError(_bad_method(method))
        if size_factors is not None or labels is not None:
            raise ValueError("a GroupMoments comes without size factors and labels")
        gm, G = counts, counts.n_genes
    else:
        gm, G = None, embed._counts(counts).G
    if n_genes is None:
        n_genes = G
    elif not _number(n_genes) or int(n_genes) != n_genes or not 1 <= n_genes <= G:
        raise ValueError("need an integer 1 <= n_genes <= genes = %d (got %r)" % (G, n_genes))
    if gm is None:
        groups, _ = encode_labels(labels, embed._counts(counts).N)
        ref = _reference_index(groups, reference)
        if ranked and tie_correct and ref is not None:
            raise ValueError(_ranks().TIE_CORRECT_NEEDS_REST)
        gm = group_moments(counts, size_factors, labels, out=out)
    if ranked:
        st = _ranks().wilcoxon(_ranks().rank_sums(counts, size_factors, labels, reference=reference), gm,
                               tie_correct=bool(tie_correct))
    else:
        st = statistics(gm, reference, method)
    names = np.argsort(-st.scores, axis=1, kind="stable")[:, :int(n_genes)]
    take = lambda a: np.take_along_axis(a, names, 1)                     # noqa: E731
    return RankGenesGroups(gm.groups, names.astype(np.int64), take(st.scores), take(st.logfoldchanges), take(st.pvals),
                           take(st.pvals_adj), take(st.pts), take(st.pts_rest), gm)


def _ranks():
    from . import ranks                 # (ranks imports this module)
    return ranks
