"""
Louvain (modularity) clustering of the connectivities of the kNN graph of cells, computed on the device: scanpy's
``tl.louvain`` on ``obsp["connectivities"]``, the step between ``graph.connectivities`` and ``markers.rank_genes_groups``.

    nb = neighbors.knn(p.scores, 14, out="torch")
    cl = cluster.louvain(nb)                         # cl.labels (N,) int32, label 0 the largest cluster; cl.modularity
    res = markers.rank_genes_groups(X, sc, cl.labels)

Everything runs in libprosstt_amd_cluster.so (include/prosstt_amd_cluster.h) and in torch's device plumbing (a sort and
prefix sums per level); there is no CPU fallback.  The host decides once per round, from the two int64 arrays of the
communities, whether the round is kept.

The definition.  It is a synchronous, reproducible form of the algorithm: equal calls give equal labels on every run,
every stream and every kernel path.

  Input.  W symmetric, CSR as ``graph.Connectivities`` holds it: ``indptr`` int64, ``indices`` int32 ascending within a
  row, ``data`` binary64 with 0 <= w <= 1.  3 <= N < 2^31, nnz < 2^30.  gamma = ``resolution`` > 0, finite.

  Quantisation.  u_ij = (int64) floor(w_ij * 2^32 + 0.5): every weight is at most 2^32 and every sum below stays under
  2^62.  W is symmetric to the bit, so u is.  From here on every sum of weights is an int64 and exact: no order of
  summation shows.

  Level graph.  n nodes, symmetric integer CSR; from the second level on with a diagonal entry u_ii, the weight inside the
  merged community, both directions counted.  k_i = sum_j u_ij (the diagonal included), M2 = sum_i k_i; M2 = 0 raises.

  State.  c_i, the community of node i, is a node index and starts as c_i = i.  tot[d] = sum_{c_i = d} k_i.
  in[d] = sum_{c_i = c_j = d} u_ij, the diagonal included.

  Gain.  g(e, T) = (double)e - (gamma * ((double)k_i * (double)T)) / (double)M2; every operation rounded on its own (no
  fused multiply-add), the int64 -> binary64 conversions to nearest.

  Sweep of parity p (synchronous: every node reads the c and tot from before the sweep).  For node i and a community d,
  e_i(d) = sum_{j != i, c_j = d} u_ij.  stay = g(e_i(c_i), tot[c_i] - k_i), the subtraction in integers.  The candidates
  are the communities d != c_i of the stored entries j != i (entries of weight 0 count); for p = 0 only d < c_i, for p = 1
  only d > c_i.  Node i moves to the candidate of largest g(e_i(d), tot[d]), the lowest d among equals, and only if that
  gain is strictly greater than stay.  (The one-direction rule keeps a synchronous sweep from swapping two nodes forever.)

  Round.  A sweep of parity 0, the totals recomputed, a sweep of parity 1, the totals recomputed.  Then the quality
  Q = math.fsum over d of (double)in[d] / (double)M2 - gamma * (t * t), t = (double)tot[d] / (double)M2, every operation
  rounded on its own and the sum exact.  A round is accepted if it moved at least one node and Q > Q_before + ``tol``;
  otherwise the state from before the round is restored and the level ends.  A level also ends after ``max_rounds``
  accepted rounds.

  Aggregation.  The level's communities are renumbered 0 .. n' - 1 by ascending community id; U'_ab = sum_{c_i = a,
  c_j = b} u_ij, the diagonal included; columns ascend within a row.  If n' = n the call ends, otherwise the next level
  starts on U'; there are at most ``max_levels`` levels.  A node's final community is the composition of the levels.

  Result labels.  Communities are numbered by size in cells, descending; equal sizes go to the community that holds the
  lowest cell index.  Label 0 is the largest cluster (scanpy's convention, as remembered).

Differences from python-louvain / networkx (read, not derived from a run of scanpy): synchronous sweeps with the parity
rule instead of a sequential random order; weights quantised to 2^-32; the quality is checked per round, not per node
move; equal calls give equal labels.
"""
import math
from typing import Any, NamedTuple

import numpy as np

from . import _native, device, graph
from .device import _ptr, _torch

PATHS = (0, 1, 2, 3, 4)         # of a sweep: 0 the library's choice, 1 .. 4 one kernel for every row (prosstt_amd_cluster.h)
PATH_ROWS = (16, 64, 512)       # the longest row (stored entries) that paths 1, 2 and 3 hold; path 4 holds every row
BAD_WEIGHT, BAD_GRAPH, BAD_COMMUNITY, BAD_BINS, BAD_SORT = 1, 2, 4, 8, 16          # bits of the status word
MAX_NNZ = 1 << 30
MAX_SUM = 1 << 62            # every sum of weights stays below: the int64 sums cannot overflow

BAD_VALUES = ((BAD_WEIGHT, "a weight of the graph is NaN, negative or above 1"),
              (BAD_GRAPH, "indptr and indices are not those of a CSR matrix of nodes x nodes"),
              (BAD_COMMUNITY, "a community lies outside [0, nodes)"),
              (BAD_BINS, "a row is longer than the sweep path it was binned into holds"),
              (BAD_SORT, "the sort of the aggregation is inconsistent"))


def _raise_bits(bits):
    if bits:
        raise ValueError("; ".join(text for bit, text in BAD_VALUES if bits & bit))


class LevelGraph(NamedTuple):
    """A level graph on the device: symmetric integer CSR (``indptr`` int64 (n + 1,), ``indices`` int32 ascending within
    a row, ``u`` int64), ``k`` (n,) its row sums, ``M2`` their sum (a Python int), and the bins of a sweep: ``rows`` (n,)
    int32, the nodes by ascending row length, and ``bins``, how many rows have at most 16, 64 and 512 entries."""
    indptr: Any
    indices: Any
    u: Any
    k: Any
    M2: int
    rows: Any
    bins: tuple

    @property
    def n(self):
        return int(self.indptr.shape[0]) - 1

    @classmethod
    def from_csr(cls, indptr, indices, u):
        """The level graph of caller-given integer CSR arrays (numpy arrays or tensors; copied to the current device):
        ``indptr`` int64, ``indices`` int32, ``u`` int64 with u >= 0 and max(u) * entries < 2^62 (what a quantisation
        gives, u <= 2^32, always is).  ValueError for other dtypes or shapes, before a device is used, and for arrays
        that are no CSR matrix or weights outside that range."""
        _check_level_arrays(indptr, indices, u)
        device.need_device("cluster")
        torch = _torch()
        indptr = graph._on_device(indptr)
        indices, u = graph._on_device(indices, indptr.device), graph._on_device(u, indptr.device)
        with torch.cuda.device(indptr.device):
            n, nnz = indptr.numel() - 1, indices.numel()
            ok = (indptr[0] == 0) & (indptr[-1] == nnz) & (indptr[1:] >= indptr[:-1]).all()
            ok = ok & (indices >= 0).all() & (indices < n).all()
            if not bool(ok):
                raise ValueError("indptr and indices are not those of a CSR matrix of nodes x nodes")
            if int(u.min()) < 0 or int(u.max()) * nnz >= MAX_SUM:
                raise ValueError("need u >= 0 and max(u) * stored entries < 2^62, so that no sum overflows")
            return _level(indptr, indices, u, _row_sums(indptr, u))


def _check_level_arrays(indptr, indices, u):
    torch = _torch()
    for name, arr, np_dtype, t_dtype in (("indptr", indptr, np.int64, torch.int64), ("indices", indices, np.int32, torch.int32),
                                         ("u", u, np.int64, torch.int64)):
        want = t_dtype if isinstance(arr, torch.Tensor) else np.dtype(np_dtype)
        if not isinstance(arr, (torch.Tensor, np.ndarray)) or arr.dtype != want or len(arr.shape) != 1:
            raise ValueError("%s must be a 1-D %s array" % (name, np.dtype(np_dtype).name))
    n, nnz = int(indptr.shape[0]) - 1, int(indices.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("need 1 <= nodes < 2^31 (got %d)" % n)
    if int(u.shape[0]) != nnz:
        raise ValueError("indices and u differ in length")
    if not 1 <= nnz < MAX_NNZ:
        raise ValueError("need 1 <= stored entries < 2^30 (got %d)" % nnz)


def _row_sums(indptr, u):
    torch = _torch()
    n = indptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(n, device=u.device), indptr[1:] - indptr[:-1])
    return torch.zeros(n, dtype=torch.int64, device=u.device).index_add_(0, rows, u)     # (integers: exact in any order)


def _level(indptr, indices, u, k):
    """The LevelGraph of device arrays: M2 and the bins of the rows by length (one host copy per level)."""
    torch = _torch()
    lengths = indptr[1:] - indptr[:-1]
    rows = torch.sort(lengths, stable=True)[1].to(torch.int32)
    counts = torch.stack([(lengths <= b).sum() for b in PATH_ROWS] + [k.sum()]).tolist()
    return LevelGraph(indptr, indices, u, k, int(counts[3]), rows, tuple(int(v) for v in counts[:3]))


class Clusters(NamedTuple):
    """``labels`` (N,) int32, 0 the largest cluster; ``sizes`` (clusters,) int64, the cells of each label; ``modularity``,
    the last accepted Q; ``levels``, a tuple of (nodes, communities, rounds, Q) per level; ``level_labels``, one (N,)
    int32 array per level: every cell's community in that level's renumbering (the last is the finest cut that ``labels``
    reorders, the earlier ones are finer).  numpy arrays, or device tensors for ``out="torch"``."""
    labels: Any
    sizes: Any
    modularity: float
    levels: tuple
    level_labels: tuple


# ------------------------------------------------------------------------------------------------- argument checks

def _positive_int(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError("%s must be a positive integer (got %r)" % (name, v))
    return int(v)


def _check_resolution(resolution):
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float, np.integer, np.floating)) \
            or not 0 < resolution < float("inf"):
        raise ValueError("resolution must be a positive finite number (got %r)" % (resolution,))
    return float(resolution)


def _check_path(path):
    if isinstance(path, bool) or path not in PATHS:
        raise ValueError("path must be one of %r (got %r)" % (PATHS, path))
    return int(path)


def _check_louvain(resolution, tol, max_rounds, max_levels, path, out):
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)) or not 0 <= tol < float("inf"):
        raise ValueError("tol must be a non-negative finite number (got %r)" % (tol,))
    return (_check_resolution(resolution), float(tol), _positive_int("max_rounds", max_rounds),
            _positive_int("max_levels", max_levels), _check_path(path))


def order_labels(communities):
    """(labels int32, sizes int64) of any host array of community ids, one per cell: the communities numbered by size in
    cells, descending; equal sizes by the lowest cell index they hold."""
    communities = np.asarray(communities)
    if communities.ndim != 1 or communities.size == 0:
        raise ValueError("need one community per cell")
    ids, first, inverse, sizes = np.unique(communities, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -sizes))
    rank = np.empty(len(ids), dtype=np.int64)
    rank[order] = np.arange(len(ids))
    return rank[inverse.ravel()].astype(np.int32), sizes[order].astype(np.int64)


def quality(tot, inn, M2, resolution):
    """Q of the definition from the host int64 arrays ``tot`` and ``inn``."""
    t = tot.astype(np.float64) / np.float64(M2)
    terms = inn.astype(np.float64) / np.float64(M2) - np.float64(resolution) * (t * t)
    return math.fsum(terms.tolist())


# ---------------------------------------------------------------------------------------------------- the kernels

def _status(dev):
    """[status word, moved counter] on ``dev``, zeroed."""
    return _torch().zeros(2, dtype=_torch().int32, device=dev)


def _quantize(L, g):
    """The level-0 LevelGraph of a ``graph.Connectivities`` of device tensors."""
    torch = _torch()
    dev = g.indptr.device
    N, nnz = g.indptr.numel() - 1, g.indices.numel()
    if nnz == 0:
        raise ValueError("the graph has no weight: every cell is its own cluster")
    if nnz >= MAX_NNZ:
        raise ValueError("need stored entries < 2^30 (got %d)" % nnz)
    flags = _status(dev)
    u = torch.empty(nnz, dtype=torch.int64, device=dev)
    k = torch.empty(N, dtype=torch.int64, device=dev)
    _native.check(L.prosstt_amd_cluster_quantize(device.current_stream(dev), _ptr(g.indptr), _ptr(g.indices), _ptr(g.data), N,
                                                 nnz, _ptr(u), _ptr(k), _ptr(flags)), "cluster")
    _raise_bits(int(flags[0].item()))
    level = _level(g.indptr, g.indices, u, k)
    if level.M2 == 0:
        raise ValueError("the graph has no weight: every cell is its own cluster")
    return level


def _sweep(L, level, c, tot, parity, resolution, path, flags):
    """c_new of one sweep, enqueued; the status word and the moved counter are ``flags``."""
    c_new = _torch().empty_like(c)
    dev = c.device
    _native.check(L.prosstt_amd_cluster_sweep(device.current_stream(dev), _ptr(level.indptr), _ptr(level.indices), _ptr(level.u),
                                              _ptr(level.k), level.n, level.indices.numel(), _ptr(level.rows), *level.bins,
                                              _ptr(c), _ptr(tot), level.M2, resolution, parity, path, _ptr(c_new),
                                              _ptr(flags[1:]), _ptr(flags)), "cluster")
    return c_new


def _totals(L, level, c, flags):
    """A (2, n) int64 tensor, tot in row 0 and in in row 1, enqueued."""
    dev = c.device
    both = _torch().empty((2, level.n), dtype=_torch().int64, device=dev)
    _native.check(L.prosstt_amd_cluster_totals(device.current_stream(dev), _ptr(level.indptr), _ptr(level.indices), _ptr(level.u),
                                               _ptr(level.k), level.n, level.indices.numel(), _ptr(c), _ptr(both[0]),
                                               _ptr(both[1]), _ptr(flags)), "cluster")
    return both


def _aggregate(L, level, c, always=False):
    """(the next LevelGraph, the renumbered community of every node); unless ``always``, None stands for the next graph
    when no two nodes share a community."""
    torch = _torch()
    dev = c.device
    st = device.current_stream(dev)
    n, nnz = level.n, level.indices.numel()
    taken = torch.zeros(n, dtype=torch.int64, device=dev)
    taken[c.long()] = 1
    new_id = torch.cumsum(taken, 0) - 1
    cnew = new_id[c.long()].to(torch.int32)
    n_new = int(new_id[-1].item()) + 1
    if n_new == n and not always:
        return None, cnew
    flags = _status(dev)
    ws = device.workspace("cluster", "prosstt_amd_cluster_workspace_bytes", dev, n, nnz)
    _native.check(L.prosstt_amd_cluster_aggregate_emit(st, _ptr(level.indptr), _ptr(level.indices), n, nnz, _ptr(cnew), n_new,
                                                       _ptr(ws), ws.numel(), _ptr(flags)), "cluster")
    sorted_keys, perm, pos, nnz_new = graph._sorted_runs(ws[:8 * nnz].view(torch.int64))
    indptr = torch.empty(n_new + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(nnz_new, dtype=torch.int32, device=dev)
    u = torch.empty(nnz_new, dtype=torch.int64, device=dev)
    _native.check(L.prosstt_amd_cluster_aggregate_fold(st, _ptr(sorted_keys), _ptr(perm), _ptr(pos), _ptr(level.u), nnz, n_new,
                                                       nnz_new, _ptr(indptr), _ptr(indices), _ptr(u), _ptr(flags)), "cluster")
    k = torch.zeros(n_new, dtype=torch.int64, device=dev).index_add_(0, cnew.long(), level.k)
    _raise_bits(int(flags[0].item()))
    return _level(indptr, indices, u, k), cnew


def _run_level(L, level, resolution, tol, max_rounds, path):
    """(c, rounds, Q) of one level: rounds until one moves nothing or does not raise Q by more than tol."""
    torch = _torch()
    dev = level.indptr.device
    flags = _status(dev)
    c = torch.arange(level.n, dtype=torch.int32, device=dev)
    both = _totals(L, level, c, flags)
    host = both.cpu().numpy()
    Q = quality(host[0], host[1], level.M2, resolution)
    rounds = 0
    while rounds < max_rounds:
        c1 = _sweep(L, level, c, both[0], 0, resolution, path, flags)
        both1 = _totals(L, level, c1, flags)
        c2 = _sweep(L, level, c1, both1[0], 1, resolution, path, flags)
        both2 = _totals(L, level, c2, flags)
        host = both2.cpu().numpy()                    # the round's one copy of arrays; it synchronises
        bits, moved = flags.tolist()
        _raise_bits(bits)
        Q2 = quality(host[0], host[1], level.M2, resolution)
        if moved == 0 or not Q2 > Q + tol:
            break
        flags[1] = 0
        c, both, Q = c2, both2, Q2
        rounds += 1
    _raise_bits(int(flags[0].item()))
    return c, rounds, Q


def _device_level(level):
    if not isinstance(level, LevelGraph) or not _torch().is_tensor(level.indptr) or level.indptr.device.type != "cuda":
        raise ValueError("need a LevelGraph of device tensors (cluster.quantize or LevelGraph.from_csr)")
    return level.indptr.device


def _communities(level, c, dev):
    torch = _torch()
    if isinstance(c, np.ndarray):
        c = torch.from_numpy(np.ascontiguousarray(c))
    if not isinstance(c, torch.Tensor) or tuple(c.shape) != (level.n,) or c.dtype not in (torch.int32, torch.int64):
        raise ValueError("c must hold one int32 community per node (%d)" % level.n)
    return c.to(device=dev, dtype=torch.int32).contiguous()


# ------------------------------------------------------------------------------------------------ public functions

def quantize(graph_):
    """The level-0 ``LevelGraph`` of a ``Neighbors`` or a ``graph.Connectivities``: u, k and M2 of the definition."""
    graph._host_checks(graph_)
    L = device.need_device("cluster")
    g = graph._as_connectivities(device.need_device("graph"), graph_)
    with _torch().cuda.device(g.indptr.device):
        return _quantize(L, g)


def totals(level, c):
    """(tot, in) of the definition, int64 device tensors (n,), for the communities ``c`` (one node index per node)."""
    dev = _device_level(level)
    L = device.need_device("cluster")
    c = _communities(level, c, dev)
    with _torch().cuda.device(dev):
        flags = _status(dev)
        both = _totals(L, level, c, flags)
        _raise_bits(int(flags[0].item()))
    return both[0], both[1]


def sweep(level, c, parity, resolution=1.0, path=0):
    """(c_new, moved) of one sweep of ``parity`` (0 or 1) from the communities ``c``: an int32 device tensor and the
    number of nodes that changed community.  ``path``: 0 lets the library choose per row; 1 .. 4 force one kernel for
    every row (``_native.NativeError`` if it cannot hold the longest).  Every path gives the same c_new."""
    if parity not in (0, 1):
        raise ValueError("parity must be 0 or 1 (got %r)" % (parity,))
    resolution, path = _check_resolution(resolution), _check_path(path)
    dev = _device_level(level)
    L = device.need_device("cluster")
    c = _communities(level, c, dev)
    with _torch().cuda.device(dev):
        flags = _status(dev)
        both = _totals(L, level, c, flags)
        c_new = _sweep(L, level, c, both[0], int(parity), resolution, path, flags)
        bits, moved = flags.tolist()
        _raise_bits(bits)
    return c_new, moved


def aggregate(level, c):
    """(the next ``LevelGraph``, map): the communities ``c`` merged into nodes, and the new node (int32, ascending with
    the community id) of every node of ``level``."""
    dev = _device_level(level)
    L = device.need_device("cluster")
    c = _communities(level, c, dev)
    with _torch().cuda.device(dev):
        if not bool(((c >= 0) & (c < level.n)).all()):
            raise ValueError("a community lies outside [0, nodes)")
        return _aggregate(L, level, c, always=True)


def louvain(graph_, resolution=1.0, *, tol=1e-7, max_rounds=1000, max_levels=32, path=0, out="numpy"):
    """Louvain clusters of a kNN graph (the module docstring's definition): ``Clusters(labels, sizes, modularity, levels,
    level_labels)``.

    ``graph_``: a ``neighbors.Neighbors`` (numpy arrays or device tensors, as ``graph.connectivities`` takes them) or a
    ``graph.Connectivities``.  ``resolution``: gamma, larger for more and smaller clusters.  ``tol``: a round must raise Q
    by more than this to be kept.  ``max_rounds``: accepted rounds per level.  ``max_levels``: levels.  ``path``: the
    sweep kernel, 0 the library's choice per row, 1 .. 4 one kernel for every row (the labels are the same).  ``out``:
    "numpy" (host arrays) or "torch" (device tensors).

    Raises ValueError, before any device use where the input allows, for what ``graph.diffmap`` refuses in a graph and for
    a bad resolution, tol, max_rounds, max_levels, path or out; ValueError, from the device's check, for a weight
    outside [0, 1] and for a graph without weight; ``_native.NativeError`` for a forced path that cannot hold a row."""
    graph._host_checks(graph_)
    resolution, tol, max_rounds, max_levels, path = _check_louvain(resolution, tol, max_rounds, max_levels, path, out)
    L = device.need_device("cluster")
    torch = _torch()
    g = graph._as_connectivities(device.need_device("graph"), graph_)
    dev = g.indptr.device
    with torch.cuda.device(dev):
        level = _quantize(L, g)
        comp = None
        levels, level_labels = [], []
        Q = None
        for _ in range(max_levels):
            c, rounds, Q = _run_level(L, level, resolution, tol, max_rounds, path)
            nxt, cnew = _aggregate(L, level, c)
            comp = cnew if comp is None else cnew[comp.long()]
            levels.append((level.n, level.n if nxt is None else nxt.n, rounds, Q))
            level_labels.append(comp)
            if nxt is None:
                break
            level = nxt
        labels, sizes = order_labels(comp.cpu().numpy())
        if out == "torch":
            return Clusters(torch.from_numpy(labels).to(dev), torch.from_numpy(sizes).to(dev), Q, tuple(levels),
                            tuple(level_labels))
        return Clusters(labels, sizes, Q, tuple(levels), tuple(t.cpu().numpy() for t in level_labels))


def modularity(graph_, labels, resolution=1.0):
    """The exact Q of the definition (of the quantised weights) for any labelling of the cells: ``labels`` holds one
    label per cell, of any type ``numpy.unique`` orders."""
    N = graph._host_checks(graph_)
    resolution = _check_resolution(resolution)
    torch = _torch()
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    labels = np.asarray(labels)
    if labels.shape != (N,):
        raise ValueError("need one label per cell (%d), not shape %s" % (N, labels.shape))
    codes = np.unique(labels, return_inverse=True)[1].ravel().astype(np.int32)
    L = device.need_device("cluster")
    g = graph._as_connectivities(device.need_device("graph"), graph_)
    dev = g.indptr.device
    with torch.cuda.device(dev):
        level = _quantize(L, g)
        flags = _status(dev)
        both = _totals(L, level, torch.from_numpy(codes).to(dev), flags)
        host = both.cpu().numpy()
        _raise_bits(int(flags[0].item()))
    return quality(host[0], host[1], level.M2, resolution)
