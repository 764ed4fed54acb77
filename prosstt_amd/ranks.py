"""
Wilcoxon rank-sum (Mann-Whitney) marker genes, computed where the count matrix lies: on the device.  The rank test of
scanpy's ``tl.rank_genes_groups(method="wilcoxon")``, for matrices whose entries are half zeros and far from normal:

    mk = markers.rank_genes_groups(X, sc, labels, method="wilcoxon")          # or tie_correct=True
    rs = ranks.rank_sums(X, sc, labels); st = ranks.wilcoxon(rs)              # the two steps on their own

A rank test needs every gene's entries ranked across all labelled cells.  libprosstt_amd_ranks.so
(include/prosstt_amd_ranks.h) forms the float32 entries a = log1p(x / s) of ``embed.LogNormalized``, bit for bit, sorts each
gene's column of them (a radix sort of the bit patterns, one block per gene) and folds the sorted column into two exact
integers per gene.  With C the counting set -- all labelled cells, or the cells of the ``reference`` group:

    Q[k][j] = sum over the cells q of group k of ( #{c in C: a_c < a_q} + #{c in C: a_c <= a_q} )
    T[j]    = sum over the maximal runs of equal a among all labelled cells of (t^3 - t), t the run's length

They depend on no order of evaluation, so every call gives the same integers.  There is no CPU fallback for the pass.  The
row list sorted by group is ``markers``' own (torch's sort, ``bincount`` and ``cumsum`` on the input's stream).

The statistics are host numpy in binary64 on Q and T (n the labelled cells, n_k those of group k):

    against the rest: the rank sum of group k with midranks is R_k = (Q_k + n_k) / 2, and
        z = (R_k - n_k (n + 1) / 2) / sqrt(n_k (n - n_k) (n + 1) / 12 * c)
        c = 1, or with tie_correct 1 - T / (n^3 - n)  (``scipy.stats.tiecorrect``)
    against group r: U = Q_k / 2 is the Mann-Whitney U of k against r with half counts for ties, and
        z = (U - n_k n_r / 2) / sqrt(n_k n_r (n_k + n_r + 1) / 12)
    where the denominator is 0: z = 0 and p = 1 (the t-test's rule for a flat gene)
    pvals = 2 scipy.stats.norm.sf(|z|);  pvals_adj: Benjamini-Hochberg over the genes of one group;  df: NaN

There is no continuity correction.  ``tie_correct`` with a reference group is refused: the pairwise tie term needs the runs'
lengths within k and r together, per pair of groups, which the fold does not keep.  scanpy is not installed here and was not
run: its conventions (the z score as the ranking score, no continuity correction, ``tie_correct`` off by default, the
normal approximation for the p-values) are as remembered, like the t-tests' in ``markers``; the formulas themselves are
checked against scipy (``rankdata``, ``tiecorrect``, ``mannwhitneyu``) in tests/test_ranks_model.py.
"""
from typing import NamedTuple

import numpy as np

from . import _native, embed, markers
from . import device as _device
from .device import _ptr, _torch
from .layout import _number

MAX_ROWS = 1 << 20              # PROSSTT_AMD_RANKS_MAX_ROWS: labelled cells in one call
SORT_TILE = 1024                # PROSSTT_AMD_RANKS_SORT_TILE: positions per tile of the sort kernel
NEGATIVE, ROW_RANGE, GROUP_RANGE = 1, 2, 4       # the bits of the status word
TIE_CORRECT_NEEDS_REST = "tie_correct needs reference='rest': the tie term of a pair of groups is not computed"


class RankSums(NamedTuple):
    """``groups``: the K categories; ``n``: (K,) int64 cells per group; ``q``: (K, G) int64 and ``ties``: (G,) int64, the Q
    and T of the module docstring (numpy arrays, or device tensors for ``out="torch"``); ``reference``: "rest" or the
    reference group; ``codes``: (cells,) int64, the group of every cell in plan order (-1: left out)."""
    groups: np.ndarray
    n: np.ndarray
    q: object
    ties: object
    reference: object
    codes: np.ndarray


def _genes_per_pass(v):
    if isinstance(v, bool) or not _number(v) or int(v) != v or not 0 <= v < 1 << 31:
        raise ValueError("need an integer 0 <= genes_per_pass < 2^31 (got %r)" % (v,))
    return int(v)


def rank_sums(counts, size_factors, labels, *, reference="rest", genes_per_pass=0, out="numpy"):
    """``RankSums`` of an int32 device count matrix for one label per cell.

    ``counts``, ``size_factors``, ``labels``, ``out``: as for ``markers.group_moments``.  ``reference``: "rest" (every
    labelled cell counts) or one of the groups.  ``genes_per_pass``: genes sorted at a time (12 bytes of workspace per cell
    and gene), 0 for the library's rule, a workspace of at most 1 GiB; the results do not depend on it.  Runs on the current
    stream.

    Raises what ``markers.group_moments`` raises for the same arguments, ValueError for an unknown ``reference``, a bad
    ``genes_per_pass``, more than 2^20 labelled cells or a negative count."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    m = embed._counts(counts)
    groups, codes = markers.encode_labels(labels, m.N)
    ref = markers._reference_index(groups, reference)
    genes_per_pass = _genes_per_pass(genes_per_pass)
    if int((codes >= 0).sum()) > MAX_ROWS:
        raise ValueError("at most 2^20 labelled cells in one call (got %d)" % int((codes >= 0).sum()))
    op = embed.LogNormalized(counts, size_factors)
    L = _device.need_device("ranks")
    torch = _torch()
    N, G = op.shape
    K = len(groups)
    dev = op.device
    with torch.cuda.device(dev):
        n, rows, start = markers._row_list(codes, K, m.cell_of_row, dev)
        n_sel = int(n.sum())
        ws = _device.workspace("ranks", "prosstt_amd_ranks_workspace_bytes", dev, n_sel, G, genes_per_pass)
        q = torch.empty((K, G), dtype=torch.int64, device=dev)
        ties = torch.empty(G, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_ranks_rank_sums(
            _device.current_stream(dev), _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(rows) if n_sel else None, n_sel,
            _ptr(start), K, -1 if ref is None else ref, genes_per_pass, _ptr(ws), ws.numel(), _ptr(q), _ptr(ties),
            _ptr(status)), "ranks")
        bits = int(status.item())
        if bits & NEGATIVE:
            raise ValueError(_device.NEGATIVE_ENTRY)
        if bits:
            raise RuntimeError("the rank pass refused its row list (status %d)" % bits)
        if out == "numpy":
            q, ties = q.cpu().numpy(), ties.cpu().numpy()
    return RankSums(groups, n, q, ties, reference, codes)


def wilcoxon(rs, gm=None, *, tie_correct=False):
    """``markers.Statistics`` of a ``RankSums`` by the module docstring's formulas, host numpy in binary64: ``scores`` is z,
    ``df`` is NaN; ``logfoldchanges``, ``pts`` and ``pts_rest`` are those of ``markers.statistics`` for the ``GroupMoments``
    ``gm`` of the same cells and labels, or NaN without one.

    Raises TypeError for another type, ValueError for ``tie_correct`` with a reference group, for a ``gm`` of other groups
    or genes, and for a group, or a rest, of fewer than two cells."""
    import scipy.stats
    if not isinstance(rs, RankSums):
        raise TypeError("wilcoxon takes a RankSums, not %s" % type(rs).__name__)
    if gm is not None and not isinstance(gm, markers.GroupMoments):
        raise TypeError("gm must be a GroupMoments, not %s" % type(gm).__name__)
    groups = np.asarray(rs.groups)
    ref = markers._reference_index(groups, rs.reference)
    if tie_correct and ref is not None:
        raise ValueError(TIE_CORRECT_NEEDS_REST)
    n_k = np.asarray(rs.n, dtype=np.int64)
    q = markers._host(rs.q).astype(np.float64)
    ties = markers._host(rs.ties).astype(np.float64)
    K, G = q.shape
    if n_k.shape != (K,) or len(groups) != K or ties.shape != (G,):
        raise ValueError("q must be (groups, genes), n one entry per group and ties one per gene")
    if gm is not None and (not np.array_equal(gm.groups, groups) or gm.n_genes != G or not np.array_equal(gm.n, n_k)):
        raise ValueError("gm covers other groups, cells or genes than the rank sums")
    if np.any(n_k < 2):
        at = int(np.argmax(n_k < 2))
        raise ValueError("every group needs at least two cells (group %r has %d)" % (groups[at], int(n_k[at])))
    n1 = n_k.astype(np.float64)[:, None]
    n = float(n_k.sum())
    if ref is None:
        if np.any(n - n1 < 2):
            raise ValueError("the rest of every group needs at least two cells")
        c = 1.0 - ties / (n ** 3 - n) if tie_correct else np.ones(G)
        above = (q + n1) / 2.0 - n1 * (n + 1.0) / 2.0
        var = n1 * (n - n1) * (n + 1.0) / 12.0 * c[None, :]
    else:
        n2 = float(n_k[ref])
        above = q / 2.0 - n1 * n2 / 2.0
        var = np.broadcast_to(n1 * n2 * (n1 + n2 + 1.0) / 12.0, q.shape)
    flat = ~(var > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(flat, 0.0, above / np.sqrt(np.where(flat, 1.0, var)))
    p = np.where(flat, 1.0, 2.0 * scipy.stats.norm.sf(np.abs(z)))
    nan = np.full((K, G), np.nan)
    lfc, pts, pts_rest = nan, nan, nan
    if gm is not None:
        t = markers.statistics(gm, rs.reference)
        lfc, pts, pts_rest = t.logfoldchanges, t.pts, t.pts_rest
    return markers.Statistics(groups, z, nan.copy(), p, markers.benjamini_hochberg(p), lfc, pts, pts_rest)
