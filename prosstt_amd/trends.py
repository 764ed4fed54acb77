"""
Expression trends along the lineage tree, computed where the count matrix lies: on the device.  The other half of the way
back from counts to what the simulator is given: the mean expression of every gene at every node of the tree
(``Tree.add_genes``), the density of the cells along it (``Tree.set_density``), and the node means and variances that a fit
of the count model starts from -- what the reference's ``examples/reproduce_axolotl.ipynb`` computes in R around the nodes of
an elastic tree.

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    tr = trends.expression_trends(X, sc, t, pt, br, bandwidth=3.0)   # tr.means (nodes, genes), tr.density, tr.labels
    f = fit.count_model(X, sc, tr.labels, tr.means)                  # alpha and beta per gene
    t2 = tr.to_tree()                                                # a Tree that sample_density simulates again

The one pass over the cells x genes matrix runs in libprosstt_amd_trends.so (include/prosstt_amd_trends.h): a node-by-cell
matrix of integer weights times the int32 count matrix, exact in integers.  The weights, the G-independent sums and the
divisions are host numpy in binary64.  There is no CPU fallback for the pass.

Definitions.

Nodes.  A ``Tree`` is the descriptor; only ``topology``, ``time``, ``branches`` and ``root`` are read (it needs no means).  The
nodes are the integer time steps of every branch in the row order of ``Tree.row_offsets()`` / ``simulation.cell_rows``:
R = sum_b T_b rows; node (b, j) has the absolute pseudotime ``branch_times()[b][0] + j``.

Cells.  Each cell has a branch label and a float64 absolute pseudotime within its branch's [first, last]; anything outside
is a ValueError.  The integer pseudotimes of a simulation are the special case.

Tree distance of the positions (b, t) and (b', t'), in binary64, each operation rounded on its own: if one branch is an
ancestor of the other, or they are the same, d = |t - t'|; otherwise d = (t - e) + (t' - e), e the last absolute time of the
deepest common ancestor branch.  This is the graph distance on the node tree, whose junction is the parent's last node.

Weight (``kernel="tricube"``, bandwidth h > 0 in pseudotime units): u = d / h; if u >= 1 there is no entry; c = (u * u) * u,
v = 1 - c, w = (v * v) * v; q = floor(w * 4096 + 0.5), an integer in 0 .. 4096; q = 0 is dropped.  ``kernel="nearest"``: a
cell's only entry is q = 4096 at its own branch's node j = floor((t - first) + 0.5), clipped to 0 .. T_b - 1: the hard bin.

``NodeWeights``: a CSR matrix of R rows x N cells: ``indptr`` int64, ``indices`` int32 ascending within a row, ``weights``
int32; ``labels`` (N,) int32, the "nearest" node of every cell for either kernel (for integer pseudotimes it is
``cell_rows(tree, pt, br)``).

Sums, exact integers: S1[r][g] = sum_e q_e x[c_e][g] (int64) and S2[r][g] = sum_e q_e x[c_e][g]^2 (128 bits, as (low, high)
uint64 words in ``summary.count_summary``'s format).  A row holds at most 2^20 - 1 entries; then S1 < 2^63 for counts up to
2^31 - 1.

Host, independent of the genes, from the CSR matrix and the float32 size factors s (``sc=None``: all ones):
weight_r = sum q; weight_sq_r = sum q^2; exposure_r = sum q_e s_e in binary64, the row's entries in their order from 0;
effective_cells_r = weight_r^2 / weight_sq_r.

Results.  means[r][g] = float(S1) / exposure_r (one rounding of the integer, one division): the ratio estimator of m in
mu = s m, the quantity ``fit`` takes as ``means``.  variances = S2 / weight - (S1 / weight)^2, the biased weighted variance
of the raw counts, which the notebook fits.  density_r = (cells whose label is r) / N.  A node with exposure 0 has NaN means
and is listed in ``empty``.

Out of scope: inferring the topology, turning ``dpt``'s groups into a tree, a matrix in chunks of cells, log-normalised
trends, several devices.
"""
from typing import Any, NamedTuple, Optional

import numpy as np

from . import _native
from . import device as _device
from .device import _ptr, _torch

ONE = 4096                              # PROSSTT_AMD_TRENDS_ONE
MAX_ROW_ENTRIES = (1 << 20) - 1         # PROSSTT_AMD_TRENDS_MAX_ROW_ENTRIES
KERNELS = ("tricube", "nearest")
NEGATIVE, INDEX_RANGE, WEIGHT_RANGE, ROW_RANGE = 1, 2, 4, 8        # the bits of the pass's status word
STATUS_MESSAGES = (
    (NEGATIVE, "NEGATIVE", _device.NEGATIVE_ENTRY),
    (INDEX_RANGE, "INDEX_RANGE", "a cell index of the node weights is outside the matrix"),
    (WEIGHT_RANGE, "WEIGHT_RANGE", "a node weight is outside 0 .. %d" % ONE),
    (ROW_RANGE, "ROW_RANGE", "indptr does not ascend from 0 to the number of entries, or a node holds more than %d entries"
     % MAX_ROW_ENTRIES),
)


class NodeWeights(NamedTuple):
    """The node-by-cell weights of the module docstring as a CSR matrix: ``indptr`` (R + 1,) int64, ``indices`` (nnz,) int32
    (the CELL in plan order, ascending within a row as ``node_weights`` builds it), ``weights`` (nnz,) int32 in 0 .. 4096 --
    host arrays, or device tensors, which ``node_sums`` does not check on the host; ``n_cells``; ``labels`` (N,) int32 host
    array, the nearest node of every cell (None for hand-made weights); ``bandwidth`` and ``kernel`` as given."""
    indptr: Any
    indices: Any
    weights: Any
    n_cells: int
    labels: Optional[np.ndarray] = None
    bandwidth: Optional[float] = None
    kernel: Optional[str] = None

    @property
    def n_nodes(self):
        return int(self.indptr.shape[0]) - 1


class NodeSums(NamedTuple):
    """``s1`` (R, G) int64 and ``s2_words`` (R, G, 2): the (low, high) 64-bit words of S2 -- numpy (uint64 words), or device
    tensors for ``out="torch"`` (int64 bit patterns: torch has no arithmetic on uint64)."""
    s1: Any
    s2_words: Any

    def s2(self):
        """S2 as an (R, G) object array of exact Python integers."""
        w = _words(self.s2_words)
        flat = [(int(hi) << 64) | int(lo) for lo, hi in w.reshape(-1, 2).tolist()]
        out = np.empty(len(flat), dtype=object)
        out[:] = flat
        return out.reshape(w.shape[:2])

    def s2_float(self):
        """S2 as (R, G) float64, each the exact integer rounded once."""
        w = _words(self.s2_words)
        lo, hi = w[..., 0], w[..., 1]
        out = lo.astype(np.float64)
        for r, g in zip(*np.nonzero(hi)):
            out[r, g] = float((int(hi[r, g]) << 64) | int(lo[r, g]))
        return out


def _words(a):
    torch = _torch()
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint64)


def check_status(bits):
    """ValueError naming every bit of the pass's status word that is set."""
    said = ["status bit %s (%d): %s" % (name, bit, text) for bit, name, text in STATUS_MESSAGES if bits & bit]
    if said:
        raise ValueError("; ".join(said))
    if bits:
        raise RuntimeError("the pass set an unknown status bit (status %d)" % bits)


# ------------------------------------------------------------------------------------------------------- the tree

class _Nodes:
    """What the definitions read of a tree: per branch (in ``tree.branches`` order) ``first``, ``last``, ``length``, ``offset``
    (its first row), the chain of ancestors, and R."""

    def __init__(self, tree):
        self.names = list(tree.branches)
        if list(tree.resident_branches()) != self.names:
            raise ValueError("the tree is sharded over processes: trends needs every branch")
        bt = tree.branch_times()
        offsets, self.R = tree.row_offsets()
        self.length = np.array([int(tree.time[b]) for b in self.names], dtype=np.int64)
        if np.any(self.length < 1):
            raise ValueError("every branch needs at least one time step")
        self.first = np.array([int(bt[b][0]) for b in self.names], dtype=np.int64)
        self.last = self.first + self.length - 1
        self.offset = np.array([offsets[b] for b in self.names], dtype=np.int64)
        index = {b: i for i, b in enumerate(self.names)}
        parent = {}
        for pair in tree.topology:
            parent[index[pair[1]]] = index[pair[0]]
        self.chain = []                              # branch -> [itself, its parent, ..., the root]
        for i in range(len(self.names)):
            c, at = [i], i
            while at in parent:
                at = parent[at]
                c.append(at)
            self.chain.append(c)
        self.node_time = np.concatenate([np.arange(f, f + n, dtype=np.float64) for f, n in zip(self.first, self.length)])

    def junction(self, a, b):
        """None when branch ``a`` is ``b``, its ancestor or its descendant; otherwise the last absolute time of their deepest
        common ancestor branch, as a float."""
        if a in self.chain[b] or b in self.chain[a]:
            return None
        common = next(c for c in self.chain[a] if c in self.chain[b])
        return float(self.last[common])

    def codes(self, branches, n=None):
        """The index in ``tree.branches`` of every cell's label (int64)."""
        arr = np.asarray(branches)
        if arr.ndim != 1 or (n is not None and arr.shape[0] != n):
            raise ValueError("need one branch label per cell")
        out = np.full(arr.shape[0], -1, dtype=np.int64)
        for i, b in enumerate(self.names):
            out[arr == b] = i
        if np.any(out < 0):
            raise ValueError("branch %r is not a branch of the tree" % (arr[np.argmax(out < 0)],))
        return out


def _cells(nodes, pseudotime, branches):
    """(t float64, codes int64) of the cells, or ValueError."""
    t = np.asarray(pseudotime)
    if t.ndim != 1 or t.dtype.kind not in "iuf":
        raise ValueError("pseudotime must be a 1-D array of numbers")
    t = t.astype(np.float64)
    if not np.all(np.isfinite(t)):
        raise ValueError("a pseudotime value is not finite")
    codes = nodes.codes(branches, t.shape[0])
    if np.any(t < nodes.first[codes]) or np.any(t > nodes.last[codes]):
        raise ValueError("a pseudotime value lies outside its branch")
    return t, codes


def _bandwidth(h):
    if isinstance(h, (bool, np.bool_)) or not isinstance(h, (int, float, np.integer, np.floating)):
        raise ValueError("bandwidth must be a positive number (got %r)" % (h,))
    h = float(h)
    if not (np.isfinite(h) and h > 0):
        raise ValueError("bandwidth must be positive and finite (got %r)" % (h,))
    return h


def _kernel(kernel):
    if kernel not in KERNELS:
        raise ValueError("kernel must be 'tricube' or 'nearest' (got %r)" % (kernel,))
    return kernel


def tricube(d, h):
    """q of the module docstring for distances ``d`` (binary64 array): 0 where u >= 1."""
    u = np.asarray(d, dtype=np.float64) / h
    c = (u * u) * u
    v = 1.0 - c
    w = (v * v) * v
    q = np.floor(w * float(ONE) + 0.5)
    return np.where(u >= 1.0, 0.0, q).astype(np.int32)


def _nearest(nodes, t, codes):
    j = np.floor((t - nodes.first[codes].astype(np.float64)) + 0.5).astype(np.int64)
    return (nodes.offset[codes] + np.clip(j, 0, nodes.length[codes] - 1)).astype(np.int32)


def _pairs(lo, hi):
    """For windows [lo_k, hi_k) of positions: (k of every pair, position of every pair), window after window."""
    n = np.maximum(hi - lo, 0)
    total = int(n.sum())
    k = np.repeat(np.arange(len(n), dtype=np.int64), n)
    start = np.cumsum(n) - n
    pos = np.arange(total, dtype=np.int64) - np.repeat(start, n) + np.repeat(lo, n)
    return k, pos


def node_weights(tree, pseudotime, branches, bandwidth=3.0, *, kernel="tricube"):
    """``NodeWeights`` of the cells around every node of ``tree`` (the module docstring's definition), host numpy.

    Windowed: the cells of every branch are sorted by pseudotime once and every node looks only at the cells of a branch
    that can lie within the bandwidth (a window a little wider than the bandwidth, found by bisection; the weight itself
    decides), never at an R x N dense table.  ``pseudotime``: (N,) numbers, ``branches``: (N,) labels of ``tree.branches``.

    Raises ValueError for a bad bandwidth or kernel, a label that is no branch, and a pseudotime that is not finite or
    outside its branch."""
    h = _bandwidth(bandwidth)
    kernel = _kernel(kernel)
    nodes = _Nodes(tree)
    t, codes = _cells(nodes, pseudotime, branches)
    N, R = t.shape[0], nodes.R
    if N >= 1 << 31:
        raise ValueError("trends takes fewer than 2^31 cells")
    labels = _nearest(nodes, t, codes)
    if kernel == "nearest":
        rows = labels.astype(np.int64)
        cells = np.arange(N, dtype=np.int64)
        q = np.full(N, ONE, dtype=np.int32)
    else:
        slack = 1e-9 * (1.0 + h + float(nodes.last.max()))       # far above the rounding of the window's bounds
        B = len(nodes.names)
        order = [np.flatnonzero(codes == b) for b in range(B)]
        order = [o[np.argsort(t[o], kind="stable")] for o in order]
        sorted_t = [t[o] for o in order]
        rows_l, cells_l, q_l = [], [], []
        for nb in range(B):                          # the nodes' branch
            tn = nodes.first[nb] + np.arange(nodes.length[nb], dtype=np.float64)
            for cb in range(B):                      # the cells' branch
                if not len(order[cb]):
                    continue
                e = nodes.junction(cb, nb)
                if e is None:
                    lo = np.searchsorted(sorted_t[cb], tn - h - slack, side="left")
                    hi = np.searchsorted(sorted_t[cb], tn + h + slack, side="right")
                else:
                    # (t - e) + (t' - e) < h: t below e + h - (t' - e)
                    lo = np.zeros(len(tn), dtype=np.int64)
                    hi = np.searchsorted(sorted_t[cb], e + (h - (tn - e)) + slack, side="right")
                k, pos = _pairs(lo.astype(np.int64), hi.astype(np.int64))
                if not len(k):
                    continue
                tc = sorted_t[cb][pos]
                d = np.abs(tc - tn[k]) if e is None else (tc - e) + (tn[k] - e)
                q = tricube(d, h)
                keep = q > 0
                rows_l.append(nodes.offset[nb] + k[keep])
                cells_l.append(order[cb][pos[keep]])
                q_l.append(q[keep])
        rows = np.concatenate(rows_l) if rows_l else np.zeros(0, dtype=np.int64)
        cells = np.concatenate(cells_l) if cells_l else np.zeros(0, dtype=np.int64)
        q = np.concatenate(q_l) if q_l else np.zeros(0, dtype=np.int32)
    by = np.lexsort((cells, rows))
    indptr = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=R), out=indptr[1:])
    return NodeWeights(indptr, cells[by].astype(np.int32), q[by].astype(np.int32), N, labels, h, kernel)


# ----------------------------------------------------------------------------------------------------------- sums

def _entries_per_block(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v < 1 << 31:
        raise ValueError("need an integer 0 <= entries_per_block < 2^31 (got %r)" % (v,))
    return int(v)


def _check_weights(w, n_cells):
    """(on_device, R, nnz) of a ``NodeWeights`` after the refusals that need no device: dtypes and shapes always; for host
    arrays also the CSR structure, the row limit and the ranges of indices and weights."""
    torch = _torch()
    if not isinstance(w, NodeWeights):
        raise TypeError("node_sums takes a NodeWeights, not %s" % type(w).__name__)
    arrays = (w.indptr, w.indices, w.weights)
    on_device = [isinstance(a, torch.Tensor) and a.device.type != "cpu" for a in arrays]
    if any(on_device) and not all(on_device):
        raise ValueError("indptr, indices and weights must all be host arrays or all device tensors")
    names = (("indptr", np.int64, torch.int64), ("indices", np.int32, torch.int32), ("weights", np.int32, torch.int32))
    host = []
    for arr, (name, np_dtype, t_dtype) in zip(arrays, names):
        if isinstance(arr, torch.Tensor) and arr.device.type == "cpu":
            arr = arr.detach().numpy()
        want = t_dtype if isinstance(arr, torch.Tensor) else np.dtype(np_dtype)
        if not isinstance(arr, (torch.Tensor, np.ndarray)) or arr.dtype != want or len(arr.shape) != 1:
            raise ValueError("%s must be a 1-D %s array" % (name, np.dtype(np_dtype).name))
        host.append(arr)
    R, nnz = int(host[0].shape[0]) - 1, int(host[1].shape[0])
    if R < 1:
        raise ValueError("indptr needs at least two entries")
    if int(host[2].shape[0]) != nnz:
        raise ValueError("indices and weights differ in length")
    if int(w.n_cells) != n_cells:
        raise ValueError("the weights are over %d cells, the matrix has %d" % (int(w.n_cells), n_cells))
    if not on_device[0]:
        indptr, indices, weights = host
        if indptr[0] != 0 or indptr[-1] != nnz or np.any(np.diff(indptr) < 0):
            raise ValueError("indptr must ascend from 0 to the number of entries")
        if np.any(np.diff(indptr) > MAX_ROW_ENTRIES):
            raise ValueError("a node holds %d entries, more than %d: lower the bandwidth"
                             % (int(np.diff(indptr).max()), MAX_ROW_ENTRIES))
        if nnz and (indices.min() < 0 or indices.max() >= n_cells):
            raise ValueError("a cell index of the node weights is outside the matrix")
        if nnz and (weights.min() < 0 or weights.max() > ONE):
            raise ValueError("a node weight is outside 0 .. %d" % ONE)
    return on_device[0], host, R, nnz


def node_sums(X, weights, *, entries_per_block=0, out="numpy"):
    """``NodeSums`` of an int32 device count matrix and a ``NodeWeights`` over its cells.

    ``X``: anything ``device.CountMatrix`` accepts (a device tensor with unit column stride, column slices included, or a
    ``device.PresentedCounts``), read in place; for a presented matrix the cell indices are translated through its
    ``cell_of_row``.  ``weights``: host arrays are checked here; device tensors are not looked at on the host, the pass
    itself guards them (nothing is read out of bounds) and its verdict is raised.  ``entries_per_block``: the entries of one
    node per block of the pass, 0 for the library's rule; the sums do not depend on it.  ``out``: "numpy", or "torch" for
    device tensors.  Runs on the current stream.

    Raises TypeError for a host matrix or another dtype; ValueError for a CPU tensor, weights that are no CSR matrix over
    the matrix's cells, a node of more than 2^20 - 1 entries, a bad ``entries_per_block`` or ``out``, and for each bit of
    the pass's status word, with the bit named.  The argument checks come before any device use."""
    sums, bits = _node_sums(X, weights, entries_per_block, out)
    check_status(bits)
    return sums


def _node_sums(X, weights, entries_per_block=0, out="numpy"):
    """``node_sums`` up to the verdict: (NodeSums, the pass's status word)."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    entries_per_block = _entries_per_block(entries_per_block)
    m = _device.CountMatrix(X, "trends.node_sums")
    if m.N < 1 or m.G < 1:
        raise ValueError("trends.node_sums needs at least one cell and one gene (got %d x %d)" % (m.N, m.G))
    if m.N >= 1 << 31:
        raise ValueError("trends.node_sums takes fewer than 2^31 cells")
    on_device, (indptr, indices, wts), R, nnz = _check_weights(weights, m.N)
    m = m.on_device()
    if on_device and any(a.device != m.device for a in (indptr, indices, wts)):
        raise ValueError("the weights lie on another device than the matrix")
    L = _device.need_device("trends")
    torch = _torch()
    dev = m.device
    with torch.cuda.device(dev):
        if not on_device:
            if m.cell_of_row is not None and nnz:
                indices = _device.inverse_permutation(m.cell_of_row)[indices].astype(np.int32)
            indptr, indices, wts = (torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (indptr, indices, wts))
        else:
            indptr, indices, wts = (a.contiguous() for a in (indptr, indices, wts))
            if m.cell_of_row is not None and nnz:
                row_of_cell = torch.as_tensor(_device.inverse_permutation(m.cell_of_row).astype(np.int32)).to(dev)
                inside = (indices >= 0) & (indices < m.N)            # (one outside stays as it is: the pass reports it)
                indices = torch.where(inside, row_of_cell[indices.clamp(0, m.N - 1).to(torch.int64)], indices)
        ws = _device.workspace("trends", "prosstt_amd_trends_workspace_bytes", dev, R, m.G, nnz, entries_per_block)
        s1 = torch.empty((R, m.G), dtype=torch.int64, device=dev)
        s2 = torch.empty((R, m.G, 2), dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_trends_node_sums(
            m.stream(), _ptr(m.X), m.N, m.G, m.ld, _ptr(indptr), _ptr(indices) if nnz else None, _ptr(wts) if nnz else None,
            R, nnz, entries_per_block, _ptr(ws), ws.numel(), _ptr(s1), _ptr(s2), _ptr(status)), "trends")
        bits = int(status.item())
        if out == "numpy":
            return NodeSums(s1.cpu().numpy(), s2.cpu().numpy().view(np.uint64)), bits
    return NodeSums(s1, s2), bits


# --------------------------------------------------------------------------------------------------------- results

def row_constants(weights, sc=None):
    """(weight, weight_sq, exposure, effective_cells), each (R,), of host ``NodeWeights`` and float32 size factors per cell
    in plan order (None: all ones), by the module docstring's definitions."""
    indptr, indices, q = (np.asarray(a) for a in (weights.indptr, weights.indices, weights.weights))
    R = indptr.shape[0] - 1
    s = np.ones(weights.n_cells, dtype=np.float32) if sc is None else np.asarray(sc, dtype=np.float32)
    rows = np.repeat(np.arange(R, dtype=np.int64), np.diff(indptr))
    q64 = q.astype(np.int64)
    run, run_sq = (np.concatenate([[0], np.cumsum(v)]) for v in (q64, q64 * q64))      # exact: below 2^63
    weight = run[indptr[1:]] - run[indptr[:-1]]
    weight_sq = run_sq[indptr[1:]] - run_sq[indptr[:-1]]
    # (bincount adds a row's terms one after the other in the order of the entries)
    exposure = np.bincount(rows, weights=q.astype(np.float64) * s[indices].astype(np.float64), minlength=R)
    with np.errstate(invalid="ignore", divide="ignore"):
        effective = weight.astype(np.float64) ** 2 / weight_sq.astype(np.float64)
    return weight, weight_sq, exposure, effective


def _size_factors(sc, n_cells):
    if sc is None:
        return None
    torch = _torch()
    if isinstance(sc, torch.Tensor):
        sc = sc.detach().cpu().numpy()
    s = np.asarray(sc)
    if s.shape != (n_cells,) or s.dtype.kind not in "iuf":
        raise ValueError("need one size factor per cell: shape (%d,), not %s" % (n_cells, s.shape))
    s = s.astype(np.float32)
    if not np.all(np.isfinite(s)) or np.any(s < 0):
        raise ValueError("size factors must be finite and not negative")
    return s


class Trends:
    """What ``expression_trends`` returns.  Per node (the rows of ``simulation.cell_rows``): ``means`` and ``variances``
    (R, G) float64, ``density``, ``weight`` (int64), ``exposure``, ``effective_cells`` (R,); ``labels`` (N,) int32 the nearest
    node of every cell; ``empty``: the nodes with exposure 0 (their means are NaN); ``sums``: the ``NodeSums``;
    ``node_weights``, ``bandwidth``, ``kernel``, ``tree``."""

    def __init__(self, tree, node_weights, sums, means, variances, density, weight, exposure, effective_cells):
        self.tree, self.node_weights, self.sums = tree, node_weights, sums
        self.means, self.variances, self.density = means, variances, density
        self.weight, self.exposure, self.effective_cells = weight, exposure, effective_cells
        self.labels = node_weights.labels
        self.bandwidth, self.kernel = node_weights.bandwidth, node_weights.kernel
        self.empty = np.flatnonzero(exposure == 0)

    def _per_branch(self, per_node):
        offsets, _ = self.tree.row_offsets()
        return {b: per_node[offsets[b]:offsets[b] + int(self.tree.time[b])] for b in self.tree.branches}

    def average_expression(self, floor=1e-7):
        """dict branch -> (T_b, G) means for ``Tree.add_genes``; values that are not positive become ``floor``, as the
        reference's notebook does.  ValueError if a node is empty, naming the nodes and the bandwidth."""
        if len(self.empty):
            raise ValueError("nodes %s have no cells within the bandwidth %r (kernel %r): raise the bandwidth"
                             % (self.empty.tolist(), self.bandwidth, self.kernel))
        return self._per_branch(np.where(self.means <= 0, float(floor), self.means))

    def branch_density(self):
        """dict branch -> (T_b,) share of the cells whose nearest node it is, for ``Tree.set_density``; sums to 1."""
        return self._per_branch(self.density)

    def to_tree(self):
        """A new ``Tree`` of the same topology, times and root with ``modules=0``, these means and this density."""
        from .tree import Tree
        t = self.tree
        new = Tree(topology=[list(pair) for pair in t.topology], time={b: int(t.time[b]) for b in t.branches},
                   num_branches=t.num_branches, branch_points=t.branch_points, modules=0, G=int(self.means.shape[1]),
                   root=t.root)
        new.add_genes(self.average_expression())
        new.set_density(self.branch_density())
        return new

    def __repr__(self):
        return "Trends(nodes=%d, genes=%d, cells=%d, kernel=%r, bandwidth=%r)" % (
            self.means.shape[0], self.means.shape[1], len(self.labels), self.kernel, self.bandwidth)


def results(tree, weights, sums, sc=None):
    """``Trends`` from host ``NodeWeights`` (with labels), a ``NodeSums`` of host arrays and the size factors: the host half of
    ``expression_trends``, which needs no device."""
    weight, _, exposure, effective = row_constants(weights, sc)
    s1 = np.asarray(sums.s1).astype(np.float64)
    s2 = sums.s2_float()
    wf = weight.astype(np.float64)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        means = np.where(exposure[:, None] == 0, np.nan, s1 / exposure[:, None])
        m1 = s1 / wf
        variances = s2 / wf - m1 * m1
    R = weights.n_nodes
    density = np.bincount(weights.labels, minlength=R).astype(np.float64) / float(weights.n_cells)
    return Trends(tree, weights, sums, means, variances, density, weight, exposure, effective)


def expression_trends(X, sc, tree, pseudotime, branches, bandwidth=3.0, *, kernel="tricube"):
    """``Trends`` of an int32 device count matrix whose cells have a branch and a pseudotime on ``tree``.

    ``X``: as for ``node_sums``.  ``sc``: one size factor per cell in plan order (host array or tensor, used as float32), or
    None for all ones.  ``tree``, ``pseudotime``, ``branches``, ``bandwidth``, ``kernel``: as for ``node_weights``.

    Raises what ``node_weights`` and ``node_sums`` raise; every argument refusal comes before any device use."""
    m = _device.CountMatrix(X, "trends.expression_trends")
    s = _size_factors(sc, m.N)
    t = np.asarray(pseudotime)
    if t.ndim != 1 or t.shape[0] != m.N:
        raise ValueError("need one pseudotime per cell: shape (%d,), not %s" % (m.N, t.shape))
    weights = node_weights(tree, pseudotime, branches, bandwidth, kernel=kernel)
    sums = node_sums(X, weights)
    return results(tree, weights, sums, s)
