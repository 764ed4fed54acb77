"""
Principal-tree inference of the lineage topology in a reduced space: the step that gives a bare count matrix a tree.
``mapping``, ``trends`` and ``fit`` need a ``Tree``; the reference's ``examples/reproduce_axolotl.ipynb`` reads one from an
elastic principal tree fitted outside Python.  Here the tree is fitted where the coordinates lie, on the device:

    p = embed.pca(X, sc, 10)                                                  # or the eigenvectors of graph.diffmap
    pt = ptree.principal_tree(p.scores)
    lf = pt.to_tree(root=start_cell, G=X.shape[1])                            # lf.tree, lf.branches, lf.pseudotime, lf.node
    tr = trends.expression_trends(X, sc, lf.tree, lf.pseudotime, lf.branches)
    counts = sim.sample_density(tr.to_tree(), 3000, alpha=0.2, beta=2.0)[0]

The method is a regularised principal tree (SimplePPT: Mao et al., "SimplePPT: a simple principal tree algorithm", SDM 2015):
R centres c_k, a spanning tree T over them and soft assignments r_ik of the cells lower one energy

    E(r, T, C) = sum_ik r_ik d2(i, k) + sigma sum_ik r_ik log r_ik + lambda sum_{(a, b) in T} |c_a - c_b|^2

in three closed-form steps: r = softmax(-d2 / sigma) (then sum_k r_ik (d2 + sigma log r_ik) = F_i, the free energy), T = the
minimum spanning tree of the centres, C = the solution of (diag Gamma + lambda L) C = S with L the tree's Laplacian.  The
hard limit sigma = 0 is Lloyd's k-means step.  The two passes over the cells run in libprosstt_amd_ptree.so
(include/prosstt_amd_ptree.h); the spanning tree and the solve are host numpy in binary64.  There is no CPU fallback for
the passes.

Definitions.

Inputs.  Y: N x d binary32 coordinates (a host array or a float64 tensor is rounded once, to nearest); C: R x d binary32
centres.  1 <= N < 2^31, 1 <= d <= 128, 1 <= R <= 4096, sigma >= 0 and finite; everything finite.

    d2(i, k) = acc_d,  acc_0 = 0,  acc_{c+1} = fl32(acc_c + fl32(t_c * t_c)),  t_c = fl32(Y[i][c] - C[k][c]),  c = 0 .. d-1

exactly ``neighbors``' distance: a separate binary32 subtract, multiply and add per coordinate; nothing fused.

``assign``.  best_i: the node of the smallest key (bits(d2), k): ties go to the lower index.  m_i = d2(i, best_i).  Then in
binary64, every operation rounded on its own:
    sigma > 0:  w_ik = exp(-(((double)d2_ik - (double)m_i) / sigma));  Z_i = sum_k w_ik, in the order below;
                r_ik = w_ik / Z_i;  F_i = m_i - sigma log Z_i
    sigma = 0:  r_ik = [k = best_i];  F_i = m_i
    Gamma_k = sum_i r_ik,  S_kc = sum_i r_ik (double)Y_ic
Z_i: lane l = 0 .. 63 adds w_ik over k = l, l + 64, ... in ascending k from 0.0; the 64 partial sums are folded by the six
butterfly stages off = 32, 16, 8, 4, 2, 1, each replacing p_l by p_l + p_(l xor off).  Gamma and S: consecutive chunks of 128
cells from cell 0, the terms of a chunk added in ascending i from 0.0, the chunk sums added in ascending chunk from 0.0.
No floating-point atomic; the bits do not depend on the stream; the per-cell outputs of a cell depend on that cell and the
centres alone.

``project``.  For edges (a, b), per cell and edge in binary64 from the binary32 inputs, ascending c, nothing fused:
    u = sum_c (y_c - a_c)(b_c - a_c),  l = sum_c (b_c - a_c)^2,  t = clamp(u / l, 0, 1) (0 when l = 0),
    q = sum_c ((y_c - a_c) - t (b_c - a_c))^2
and the edge with the smallest (bits(q), e): ties to the lower edge.  Every step is IEEE.

Host (binary64 numpy, this file; tests/ptree_model.py runs the same code over its own numpy passes).
    ``spanning_tree(C)``: Prim's minimum spanning tree on D[a][b] = sum_c ((double)C_ac - (double)C_bc)^2 (ascending c),
        from node 0; the next edge is the smallest (distance, parent, child), so the tree is unique.  Edges (parent, child)
        in the order they are added.
    ``centre_step``: solves (diag Gamma + lambda L) C = S; a node with Gamma_k = 0 and lambda deg_k = 0 (an empty cluster of
        k-means, a lone node) keeps its centre: its row of the system is the identity.  The new C is rounded once to binary32.
    ``energy``: E = fsum(F_i) + lambda sum_edges |c_a - c_b|^2 (binary64 from the binary32 centres).
    ``lam`` is given in units of N / R: lambda = lam N / R sits on Gamma's scale.

Out of scope: growing or shrinking the node set (ElPiGraph's grammars); several devices; a principal tree on the count matrix
itself, without a reduced space; alternating ``map_cells`` and ``expression_trends`` after the first fit; a device MST.
"""
import math
from typing import Any, NamedTuple, Optional

import numpy as np

from . import _native
from . import device as _device
from .device import _ptr, _torch

MAX_DIM = 128                   # PROSSTT_AMD_PTREE_MAX_DIM
MAX_NODES = 4096                # PROSSTT_AMD_PTREE_MAX_NODES
MAX_EDGES = 8192                # PROSSTT_AMD_PTREE_MAX_EDGES
CHUNK = 128                     # PROSSTT_AMD_PTREE_CHUNK: the cells of one chunk of the per-node sums
NONFINITE, EDGE_RANGE = 1, 2    # the bits of the passes' status word
STATUS_MESSAGES = (
    (NONFINITE, "NONFINITE", "a coordinate or a centre is not finite"),
    (EDGE_RANGE, "EDGE_RANGE", "an edge names a node outside 0 .. R-1"),
)
OUT_CHOICES = "out must be 'numpy' or 'torch'"
NOT_FINITE = "ptree needs finite coordinates and centres"

# The defaults of principal_tree and to_tree (DESIGN section 28 has what was tried).
N_NODES = 40
LAM = 1.0
N_ITER = 30
TOL = 1e-5
KMEANS_ITER = 10
MIN_BRANCH_NODES = 3


class Assignment(NamedTuple):
    """``best`` (N,) int32, ``sq_distance`` (N,) float32 (the bits of m_i), ``free_energy`` (N,) float64, ``gamma`` (R,) and
    ``sums`` (R, d) float64, ``resp`` (N, R) float64 or None -- numpy arrays, or device tensors for ``out="torch"``."""
    best: Any
    sq_distance: Any
    free_energy: Any
    gamma: Any
    sums: Any
    resp: Any = None

    @staticmethod
    def concat(parts):
        """The ``Assignment`` of a panel passed in chunks of cells (host arrays): the per-cell fields concatenated, ``gamma``
        and ``sums`` added in the order given.  The per-cell fields are the bits of one call on the whole panel; gamma and
        sums are another order of the same sums."""
        parts = list(parts)
        gamma = np.array(parts[0].gamma, dtype=np.float64)
        sums = np.array(parts[0].sums, dtype=np.float64)
        for p in parts[1:]:
            gamma = gamma + p.gamma
            sums = sums + p.sums
        resp = None if any(p.resp is None for p in parts) else np.concatenate([p.resp for p in parts])
        return Assignment(np.concatenate([p.best for p in parts]), np.concatenate([p.sq_distance for p in parts]),
                          np.concatenate([p.free_energy for p in parts]), gamma, sums, resp)


class Projection(NamedTuple):
    """Per cell: ``edge`` (N,) int32 the nearest edge, ``t`` (N,) float64 the position along it from its first node, and
    ``sq_distance`` (N,) float64 the squared distance to it."""
    edge: Any
    t: Any
    sq_distance: Any


class KMeans(NamedTuple):
    """``centres`` (k, d) float32, ``labels`` (N,) int32 and ``inertia`` (the sum of the squared distances) for these centres,
    ``n_iter`` the centre updates made, ``converged``: the labels stopped changing."""
    centres: np.ndarray
    labels: np.ndarray
    inertia: float
    n_iter: int
    converged: bool


class LineageFit(NamedTuple):
    """What ``PrincipalTree.to_tree`` returns: ``tree`` a ``prosstt_amd.tree.Tree`` with its density set from the cells per
    node; per cell ``branches`` (the label), ``pseudotime`` (int64, the node's absolute time), ``position`` (float64,
    continuous, from the projection on the tree's edges), ``node`` (int32, the row ``simulation.cell_rows`` returns);
    ``kept`` the principal-tree nodes that survived the pruning, ``node_rows`` (len(kept),) the row of each of them."""
    tree: Any
    branches: np.ndarray
    pseudotime: np.ndarray
    position: np.ndarray
    node: np.ndarray
    kept: np.ndarray
    node_rows: np.ndarray


def check_status(bits):
    """ValueError naming every bit of the passes' status word that is set."""
    said = ["status bit %s (%d): %s" % (name, bit, text) for bit, name, text in STATUS_MESSAGES if bits & bit]
    if said:
        raise ValueError("; ".join(said))
    if bits:
        raise RuntimeError("the pass set an unknown status bit (status %d)" % bits)


# ------------------------------------------------------------------------------------------------------- the host steps

def centre_distances(C):
    """D[a][b] = sum_c ((double)C_ac - (double)C_bc)^2 in ascending c: (R, R) float64, symmetric to the bit."""
    C = np.asarray(C, dtype=np.float32).astype(np.float64)
    D = np.zeros((C.shape[0], C.shape[0]), dtype=np.float64)
    for c in range(C.shape[1]):
        t = C[:, None, c] - C[None, :, c]
        D += t * t
    return D


def spanning_tree(C):
    """Prim's minimum spanning tree of the centres (the module docstring's rule): (R - 1, 2) int32 edges (parent, child)."""
    return prim(centre_distances(C))


def prim(D):
    """Prim's tree on a symmetric (R, R) matrix of weights from node 0; the next edge is the smallest (weight, parent,
    child).  (R - 1, 2) int32."""
    D = np.asarray(D, dtype=np.float64)
    R = D.shape[0]
    edges = np.zeros((R - 1, 2), dtype=np.int32)
    outside = np.ones(R, dtype=bool)
    outside[0] = False
    key = D[0].copy()                               # the lightest edge from the tree to every node, and its lowest parent
    parent = np.zeros(R, dtype=np.int64)
    index = np.arange(R)
    for step in range(R - 1):
        low = key[outside].min()
        ties = outside & (key == low)
        p = parent[ties].min()
        v = int(index[ties & (parent == p)][0])
        edges[step] = (p, v)
        outside[v] = False
        better = outside & ((D[v] < key) | ((D[v] == key) & (v < parent)))
        key[better] = D[v][better]
        parent[better] = v
    return edges


def laplacian(R, edges):
    L = np.zeros((R, R), dtype=np.float64)
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        L[a, a] += 1.0
        L[b, b] += 1.0
        L[a, b] -= 1.0
        L[b, a] -= 1.0
    return L


def centre_step(gamma, sums, edges, lam, centres):
    """The centres that solve (diag gamma + lam L) C = sums, rounded once to binary32; a node with gamma 0 and lam deg 0
    keeps its row of ``centres``."""
    gamma = np.asarray(gamma, dtype=np.float64)
    S = np.array(sums, dtype=np.float64)
    R = gamma.shape[0]
    A = np.diag(gamma) + float(lam) * laplacian(R, edges)
    lone = np.diag(A) == 0.0
    if np.any(lone):
        A[lone, lone] = 1.0
        S[lone] = np.asarray(centres, dtype=np.float32).astype(np.float64)[lone]
    return np.linalg.solve(A, S).astype(np.float32)


def tree_length(centres, edges):
    """sum over the edges of |c_a - c_b|^2, binary64 from the binary32 centres, by ``math.fsum``."""
    C = np.asarray(centres, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    diff = C[e[:, 0]] - C[e[:, 1]]
    return math.fsum((diff * diff).ravel().tolist())


def energy(free_energy, centres, edges, lam):
    """E = fsum(F_i) + lam sum_edges |c_a - c_b|^2."""
    return math.fsum(np.asarray(free_energy, dtype=np.float64).tolist()) + float(lam) * tree_length(centres, edges)


def lloyd(Y, centres, hard_pass, n_iter):
    """Lloyd iterations from ``centres`` (k, d) float32: ``hard_pass(centres)`` is an ``Assignment`` of the sigma = 0 pass.
    A centre is sums / gamma rounded once to binary32; an empty cluster keeps its centre.  Stops when the labels no longer
    change.  ``KMeans``."""
    C = np.array(centres, dtype=np.float32)
    a = hard_pass(C)
    done, converged = 0, False
    while done < n_iter:
        new = C.copy()
        full = a.gamma > 0
        new[full] = (a.sums[full] / a.gamma[full, None]).astype(np.float32)
        C = new
        done += 1
        b = hard_pass(C)
        same = np.array_equal(a.best, b.best)
        a = b
        if same:
            converged = True
            break
    inertia = math.fsum(np.asarray(a.sq_distance, dtype=np.float64).tolist())
    return KMeans(C, np.asarray(a.best), inertia, done, converged)


def fit_tree(N, centres, soft_pass, lam, n_iter, tol):
    """The alternation from ``centres``: per iteration the soft pass, the spanning tree and the centre step; ``lam`` is the
    absolute lambda.  ``soft_pass(C)`` is an ``Assignment``.  Returns (centres, edges, energies, the last Assignment, the
    centre steps made, converged): the edges, the last energy and the assignment belong to the returned centres.  Converged
    when an iteration lowers E by at most tol |E|."""
    C = np.array(centres, dtype=np.float32)
    energies = []
    steps, converged = 0, False
    while True:
        a = soft_pass(C)
        edges = spanning_tree(C)
        energies.append(energy(a.free_energy, C, edges, lam))
        if len(energies) > 1 and energies[-2] - energies[-1] <= tol * abs(energies[-1]):
            converged = True
            break
        if steps >= n_iter:
            break
        C = centre_step(a.gamma, a.sums, edges, lam, C)
        steps += 1
    return C, edges, np.array(energies, dtype=np.float64), a, steps, converged


# ------------------------------------------------------------------------------------------------------- the lineage

def _adjacency(R, edges):
    adj = [set() for _ in range(R)]
    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2):
        adj[int(a)].add(int(b))
        adj[int(b)].add(int(a))
    return adj


def _check_tree(R, edges):
    e = np.asarray(edges)
    if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
        raise ValueError("edges must be an (E, 2) integer array")
    if e.shape[0] != R - 1 or (e.size and (e.min() < 0 or e.max() >= R)) or np.any(e[:, 0] == e[:, 1]):
        raise ValueError("the edges are not a spanning tree of the %d nodes" % R)
    adj = _adjacency(R, e)
    seen, stack = {0}, [0]
    while stack:
        for v in adj[stack.pop()]:
            if v not in seen:
                seen.add(v)
                stack.append(v)
    if len(seen) != R:
        raise ValueError("the edges are not a spanning tree of the %d nodes" % R)
    return adj


def prune(R, edges, min_branch_nodes):
    """The nodes that survive the pruning, ascending, and the adjacency among them: while the tree has a fork, the tip branch
    (a tip and the nodes of degree 2 behind it, up to but without the fork) with the fewest nodes, if fewer than
    ``min_branch_nodes``, is removed; ties go to the lower tip."""
    adj = _check_tree(R, edges)
    alive = set(range(R))
    while True:
        twigs = []
        for tip in sorted(alive):
            if len(adj[tip]) != 1:
                continue
            chain, prev, at = [tip], tip, next(iter(adj[tip]))
            while len(adj[at]) == 2:
                chain.append(at)
                prev, at = at, next(v for v in adj[at] if v != prev)
            if len(adj[at]) >= 3:                   # (a chain that ends in another tip has no fork: nothing to prune)
                twigs.append((len(chain), tip, chain))
        twigs = [t for t in twigs if t[0] < min_branch_nodes]
        if not twigs:
            break
        _, _, chain = min(twigs)
        for v in chain:
            for w in adj[v]:
                adj[w].discard(v)
            adj[v] = set()
            alive.discard(v)
    return np.array(sorted(alive), dtype=np.int64), adj


def lineage(R, edges, root_node, min_branch_nodes):
    """The branches of the pruned tree walked from the tip nearest (in edges, ties to the lower node) to ``root_node``, or
    to the kept node nearest to it if it was pruned: (kept, names, topology, time, row_of_node (R,), -1 for a pruned node;
    branch_of_row, time_of_row).  Branches are the maximal chains between nodes of degree != 2, a fork is the last node of
    its parent branch, children are visited in ascending order of their first node, parents are listed before children."""
    kept, adj = prune(R, edges, min_branch_nodes)
    full = _adjacency(R, edges)
    # hops from root_node over the whole tree: the nearest kept tip
    hops, frontier = {int(root_node): 0}, [int(root_node)]
    while frontier:
        nxt = []
        for u in frontier:
            for v in full[u]:
                if v not in hops:
                    hops[v] = hops[u] + 1
                    nxt.append(v)
        frontier = nxt
    tips = [int(v) for v in kept if len(adj[int(v)]) <= 1]
    start = min(tips, key=lambda v: (hops[v], v))
    names, topology, time, chains = [], [], {}, []
    queue = [(None, None, start)]                   # (parent branch, the fork it hangs on, its first node)
    while queue:
        parent, fork, first = queue.pop(0)
        name = "B%d" % len(names)
        names.append(name)
        chain, prev, at = [first], fork, first
        while True:
            ahead = sorted(v for v in adj[at] if v != prev)
            if len(ahead) != 1:
                break
            prev, at = at, ahead[0]
            chain.append(at)
        chains.append(chain)
        time[name] = len(chain)
        if parent is not None:
            topology.append([parent, name])
        for v in ahead:
            queue.append((name, at, v))
    row_of_node = np.full(R, -1, dtype=np.int64)
    branch_of_row, time_of_row = [], []
    first_time = {names[0]: 0}
    for pair in topology:
        first_time[pair[1]] = first_time[pair[0]] + time[pair[0]]
    at = 0
    for name, chain in zip(names, chains):
        for j, v in enumerate(chain):
            row_of_node[v] = at
            branch_of_row.append(name)
            time_of_row.append(first_time[name] + j)
            at += 1
    return kept, names, topology, time, row_of_node, np.array(branch_of_row), np.array(time_of_row, dtype=np.int64)


def lineage_fit(R, edges, root_node, min_branch_nodes, G, reassign, reproject):
    """``LineageFit`` of a principal tree of R nodes.  ``reassign(kept)``: (N,) the index INTO ``kept`` of every cell's
    nearest kept node; ``reproject(kept_edges)``: (edge (N,), t (N,)) of the cells on the (E, 2) edges given as node indices."""
    from .tree import Tree
    kept, names, topology, time, row_of_node, branch_of_row, time_of_row = lineage(R, edges, root_node, min_branch_nodes)
    node_of_cell = kept[np.asarray(reassign(kept), dtype=np.int64)]
    rows = row_of_node[node_of_cell]
    n_rows = len(branch_of_row)
    counts = np.bincount(rows, minlength=n_rows).astype(np.float64)
    share = counts / counts.sum()
    density, at = {}, 0
    for name in names:
        density[name] = share[at:at + time[name]]
        at += time[name]
    forks = sum(1 for name in names if any(pair[0] == name for pair in topology))
    tree = Tree(topology=topology, time=time, num_branches=len(names), branch_points=forks, modules=0, G=int(G),
                density=density, root=names[0])
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    kept_edges = e[(row_of_node[e[:, 0]] >= 0) & (row_of_node[e[:, 1]] >= 0)] if len(e) else e
    if len(kept_edges):
        edge, t = reproject(kept_edges)
        ta = time_of_row[row_of_node[kept_edges[:, 0]]].astype(np.float64)
        tb = time_of_row[row_of_node[kept_edges[:, 1]]].astype(np.float64)
        edge = np.asarray(edge, dtype=np.int64)
        position = ta[edge] + np.asarray(t, dtype=np.float64) * (tb[edge] - ta[edge])
    else:
        position = np.zeros(len(rows), dtype=np.float64)
    return LineageFit(tree, branch_of_row[rows], time_of_row[rows], position, rows.astype(np.int32), kept,
                      row_of_node[kept])


# ------------------------------------------------------------------------------------------------------- the checks

def _check_sizes(shape, what, lo=1, hi=(1 << 31) - 1):
    """(rows, d) of an accepted panel shape, or ValueError; touches no device."""
    if len(shape) != 2:
        raise ValueError("ptree needs a (%s, coordinates) panel, not %d dimensions" % (what, len(shape)))
    n, d = (int(v) for v in shape)
    if not lo <= n <= hi:
        raise ValueError("ptree needs %d <= %s <= %d (got %d)" % (lo, what, hi, n))
    if not 1 <= d <= MAX_DIM:
        raise ValueError("ptree needs 1 <= coordinates <= %d (got %d)" % (MAX_DIM, d))
    return n, d


def _host_panel(points, what, hi):
    """A host array as C-contiguous float32 (rounded once, to nearest) after the checks; None for a device tensor."""
    torch = _torch()
    if isinstance(points, torch.Tensor):
        if points.device.type != "cpu":
            return None
        if not points.dtype.is_floating_point:
            raise TypeError("ptree needs floating-point %s, not %s" % (what, points.dtype))
        points = points.detach().numpy()
    host = np.asarray(points)
    if host.dtype.kind != "f":
        raise TypeError("ptree needs floating-point %s, not %s" % (what, host.dtype))
    _check_sizes(host.shape, what, 1, hi)
    if not np.all(np.isfinite(host)):
        raise ValueError(NOT_FINITE)
    with np.errstate(over="ignore"):
        host = np.ascontiguousarray(host, dtype=np.float32)
    if not np.all(np.isfinite(host)):
        raise ValueError(NOT_FINITE)
    return host


def _device_panel(points, what, hi, dev=None):
    """(float32 device tensor with unit column stride, rows, d, row stride) of an accepted panel.  Everything that can be
    refused without a device is refused before one is used; a device tensor's values are the status word's to judge."""
    torch = _torch()
    host = _host_panel(points, what, hi)
    if host is None:
        if points.dtype not in (torch.float32, torch.float64):
            raise TypeError("ptree needs float32 or float64 %s, not %s" % (what, points.dtype))
        n, d = _check_sizes(tuple(points.shape), what, 1, hi)
        P = points.detach()
        if P.dtype != torch.float32:
            P = P.to(torch.float32)
        if (d > 1 and P.stride(1) != 1) or (n > 1 and P.stride(0) < d):
            P = P.contiguous()
        return P, n, d, (P.stride(0) if n > 1 else d)
    _device.need_device("ptree")
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    P = torch.from_numpy(host).to(dev)
    return P, host.shape[0], host.shape[1], host.shape[1]


def _sigma(sigma):
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)):
        raise ValueError("sigma must be a number >= 0 (got %r)" % (sigma,))
    sigma = float(sigma)
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError("sigma must be finite and >= 0 (got %r)" % (sigma,))
    return sigma


def _edges(edges, R):
    e = np.asarray(edges)
    if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
        raise ValueError("edges must be an (E, 2) integer array")
    if not 1 <= e.shape[0] <= MAX_EDGES:
        raise ValueError("ptree.project takes 1 .. %d edges (got %d)" % (MAX_EDGES, e.shape[0]))
    if e.min() < 0 or e.max() >= R:
        raise ValueError("an edge names a node outside 0 .. %d" % (R - 1))
    return np.ascontiguousarray(e, dtype=np.int32)


def _count(value, name, lo, hi):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= value <= hi:
        raise ValueError("%s must be an integer in %d .. %d (got %r)" % (name, lo, hi, value))
    return int(value)


# ------------------------------------------------------------------------------------------------------- the passes

def assign(Y, centres, sigma=0.0, *, responsibilities=False, out="numpy"):
    """The assign pass (the module docstring's definition): ``Assignment``.

    ``Y``: (cells, coordinates), 1 <= coordinates <= 128 -- ``PCA.scores`` usually.  A host array is rounded to binary32 (to
    nearest) and copied to the current device; a float32 device tensor is read where it lies (unit column stride, any row
    stride and base alignment); a float64 device tensor is rounded once.  ``centres``: (nodes, coordinates) likewise,
    1 <= nodes <= 4096.  ``sigma`` > 0 is the soft pass, 0 the hard one.  ``responsibilities=True`` also returns the N x R
    matrix r.  ``out``: "numpy", or "torch" for device tensors.  Runs on the current stream.

    Rows are independent: the per-cell fields of a panel in chunks of cells are the bits of one call on the whole
    (``Assignment.concat``).

    Raises TypeError for a dtype that is not floating; ValueError, before any device use, for a shape that is not 2-D, sizes
    outside the limits, panels of different widths, a bad ``sigma`` or ``out`` and non-finite host values; ValueError for
    each bit of the status word (a non-finite value in a device tensor)."""
    result, bits = _assign(Y, centres, sigma, responsibilities, out)
    check_status(bits)
    return result


def _assign(Y, centres, sigma=0.0, responsibilities=False, out="numpy"):
    """``assign`` up to the verdict: (Assignment, the status word)."""
    if out not in ("numpy", "torch"):
        raise ValueError(OUT_CHOICES)
    sigma = _sigma(sigma)
    torch = _torch()
    y_host, c_host = _host_panel(Y, "cells", (1 << 31) - 1), _host_panel(centres, "nodes", MAX_NODES)
    shapes = [tuple(a.shape) for a in (Y if y_host is None else y_host, centres if c_host is None else c_host)]
    _check_sizes(shapes[0], "cells")
    _check_sizes(shapes[1], "nodes", 1, MAX_NODES)
    if shapes[0][1] != shapes[1][1]:
        raise ValueError("the cells have %d coordinates, the centres %d" % (shapes[0][1], shapes[1][1]))
    P, N, d, ld = _device_panel(Y if y_host is None else y_host, "cells", (1 << 31) - 1)
    C, R, _, ldc = _device_panel(centres if c_host is None else c_host, "nodes", MAX_NODES, P.device)
    if C.device != P.device:
        raise ValueError("the centres lie on another device than the cells")
    L = _device.need_device("ptree")
    dev = P.device
    with torch.cuda.device(dev):
        ws = _device.workspace("ptree", "prosstt_amd_ptree_workspace_bytes", dev, N, d, R, int(sigma > 0))
        best = torch.empty(N, dtype=torch.int32, device=dev)
        d2min = torch.empty(N, dtype=torch.float32, device=dev)
        free = torch.empty(N, dtype=torch.float64, device=dev)
        gamma = torch.empty(R, dtype=torch.float64, device=dev)
        sums = torch.empty((R, d), dtype=torch.float64, device=dev)
        resp = torch.empty((N, R), dtype=torch.float64, device=dev) if responsibilities else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_ptree_assign(
            _device.current_stream(dev), _ptr(P), N, d, ld, _ptr(C), R, ldc, sigma, _ptr(ws), ws.numel(), _ptr(best),
            _ptr(d2min), _ptr(free), _ptr(gamma), _ptr(sums), _ptr(resp), _ptr(status)), "ptree")
        bits = int(status.item())
        fields = (best, d2min, free, gamma, sums, resp)
        if out == "numpy":
            fields = tuple(None if a is None else a.cpu().numpy() for a in fields)
    return Assignment(*fields), bits


def project(Y, centres, edges, *, out="numpy"):
    """The project pass (the module docstring's definition): ``Projection``.  ``Y``, ``centres``, ``out``: as for ``assign``;
    ``edges``: (E, 2) integers, 1 <= E <= 8192, node indices into ``centres``.

    Raises what ``assign`` raises, and ValueError for edges of another shape or dtype, too many of them, or a node index
    outside the centres, before any device use."""
    if out not in ("numpy", "torch"):
        raise ValueError(OUT_CHOICES)
    torch = _torch()
    y_host, c_host = _host_panel(Y, "cells", (1 << 31) - 1), _host_panel(centres, "nodes", MAX_NODES)
    shapes = [tuple(a.shape) for a in (Y if y_host is None else y_host, centres if c_host is None else c_host)]
    _check_sizes(shapes[0], "cells")
    _check_sizes(shapes[1], "nodes", 1, MAX_NODES)
    if shapes[0][1] != shapes[1][1]:
        raise ValueError("the cells have %d coordinates, the centres %d" % (shapes[0][1], shapes[1][1]))
    e = _edges(edges, shapes[1][0])
    P, N, d, ld = _device_panel(Y if y_host is None else y_host, "cells", (1 << 31) - 1)
    C, R, _, ldc = _device_panel(centres if c_host is None else c_host, "nodes", MAX_NODES, P.device)
    if C.device != P.device:
        raise ValueError("the centres lie on another device than the cells")
    L = _device.need_device("ptree")
    dev = P.device
    with torch.cuda.device(dev):
        e_d = torch.from_numpy(e).to(dev)
        edge = torch.empty(N, dtype=torch.int32, device=dev)
        t = torch.empty(N, dtype=torch.float64, device=dev)
        q = torch.empty(N, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_ptree_project(
            _device.current_stream(dev), _ptr(P), N, d, ld, _ptr(C), R, ldc, _ptr(e_d), e.shape[0], _ptr(edge), _ptr(t),
            _ptr(q), _ptr(status)), "ptree")
        check_status(int(status.item()))
        if out == "torch":
            return Projection(edge, t, q)
        return Projection(edge.cpu().numpy(), t.cpu().numpy(), q.cpu().numpy())


# ------------------------------------------------------------------------------------------------------- the fits

def _given_centres(init, k, d):
    """The (k, d) float32 host array of given initial centres, or ValueError; touches no device but to read a device tensor."""
    c = _host_panel(init, "centres", MAX_NODES)
    if c is None:
        c = _host_panel(init.detach().cpu(), "centres", MAX_NODES)
    if c.shape[0] != k:
        raise ValueError("init has %d centres, %d were asked for" % (c.shape[0], k))
    if c.shape[1] != d:
        raise ValueError("the cells have %d coordinates, init %d" % (d, c.shape[1]))
    return c


def _prepare(Y, k, what, init=None):
    """(the device panel as ``assign`` takes it, N, k, (k, d) float32 host centres to start from) after the refusals: the
    given ``init``, or k distinct cells drawn with ``np.random.default_rng(seed)``, in ascending order of the cell."""
    init, seed = init
    host = _host_panel(Y, "cells", (1 << 31) - 1)
    N, d = _check_sizes(tuple((Y if host is None else host).shape), "cells")
    k = _count(k, what, 1, MAX_NODES)
    if k > N:
        raise ValueError("%s = %d exceeds the %d cells" % (what, k, N))
    centres = None if init is None else _given_centres(init, k, d)
    P = _device_panel(Y if host is None else host, "cells", (1 << 31) - 1)[0]
    if centres is None:
        picks = np.sort(np.random.default_rng(seed).choice(N, size=k, replace=False))
        centres = host[picks].copy() if host is not None else P[_torch().as_tensor(picks, device=P.device)].cpu().numpy()
    return P, N, k, centres


def kmeans(Y, k, *, n_iter=100, seed=0, init=None):
    """Lloyd's k-means of the cells on the hard pass: ``KMeans``.  ``Y``: as for ``assign``.  The initial centres are ``k``
    distinct cells drawn with ``np.random.default_rng(seed)`` (sorted), or ``init`` (k, d).  A centre is the mean of its
    cells rounded once to binary32; an empty cluster keeps its centre; at most ``n_iter`` updates.

    Raises what ``assign`` raises, and ValueError for k outside 1 .. min(cells, 4096), a bad ``n_iter`` or an ``init`` of
    another shape, before any device use."""
    n_iter = _count(n_iter, "n_iter", 0, 1 << 20)
    P, N, k, centres = _prepare(Y, k, "k", (init, seed))
    return lloyd(P, centres, lambda C: assign(P, C, 0.0), n_iter)


class PrincipalTree:
    """What ``principal_tree`` returns: ``centres`` (R, d) float32, ``edges`` (R - 1, 2) int32 (their minimum spanning tree),
    ``energy`` (one value per soft pass), ``sigma``, ``lam`` (in units of N / R), ``n_iter`` (the centre steps made),
    ``converged``, ``best`` (N,) int32 the nearest node of every cell."""

    def __init__(self, panel, centres, edges, energies, sigma, lam, n_iter, converged, best):
        self._panel = panel
        self.centres, self.edges, self.energy = centres, edges, energies
        self.sigma, self.lam, self.n_iter, self.converged, self.best = sigma, lam, n_iter, converged, best

    def responsibilities(self):
        """(N, R) float64: the soft assignment of the fitted cells to the final centres."""
        return assign(self._panel, self.centres, self.sigma, responsibilities=True).resp

    def project(self, Y=None):
        """``Projection`` of ``Y`` (the fitted cells by default) on the tree's edges."""
        return project(self._panel if Y is None else Y, self.centres, self.edges)

    def to_tree(self, root, *, min_branch_nodes=MIN_BRANCH_NODES, G=500):
        """``LineageFit``: the lineage tree read from the principal tree, rooted at the tip nearest along the tree to the
        node of cell ``root``.  Tip branches with fewer than ``min_branch_nodes`` nodes are pruned, shortest first (ties to the
        lower tip); the cells are assigned again by one hard pass over the kept nodes.  Branches are the maximal chains
        between nodes of degree != 2, a fork is the last node of its parent branch, ``time[b]`` is the number of nodes of
        the chain, and the density is the share of the cells per node.  ``G``: the genes of the new ``Tree``.

        ``branches``, ``pseudotime`` and ``node`` are what ``trends.expression_trends``, ``simulation.cell_rows`` and
        ``fit.count_model`` take."""
        N = len(self.best)
        root = _count(root, "root", 0, N - 1)
        min_branch_nodes = _count(min_branch_nodes, "min_branch_nodes", 0, MAX_NODES)
        G = _count(G, "G", 1, (1 << 31) - 1)
        R = self.centres.shape[0]
        return lineage_fit(R, self.edges, int(self.best[root]), min_branch_nodes, G,
                           lambda kept: assign(self._panel, self.centres[kept], 0.0).best,
                           lambda kept_edges: project(self._panel, self.centres, kept_edges)[:2])

    def __repr__(self):
        return "PrincipalTree(nodes=%d, cells=%d, sigma=%r, lam=%r, n_iter=%d, converged=%r)" % (
            self.centres.shape[0], len(self.best), self.sigma, self.lam, self.n_iter, self.converged)


def _positive(value, name, zero_ok=False):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a number (got %r)" % (name, value))
    value = float(value)
    if not np.isfinite(value) or value < 0 or (value == 0 and not zero_ok):
        raise ValueError("%s must be finite and %s 0 (got %r)" % (name, ">=" if zero_ok else ">", value))
    return value


def principal_tree(Y, n_nodes=N_NODES, *, sigma=None, lam=LAM, n_iter=N_ITER, tol=TOL, seed=0, init="kmeans"):
    """A regularised principal tree of the cells (the module docstring's alternation): ``PrincipalTree``.

    ``Y``: as for ``assign``.  ``n_nodes``: R.  ``init``: "kmeans" (``KMEANS_ITER`` Lloyd updates from ``n_nodes`` cells drawn
    with ``seed``), "cells" (those cells) or an (R, d) array of centres.  ``sigma``: None for the mean of the squared
    distances to the nearest initial centre, or a positive number.  ``lam``: the tree's stiffness in units of N / R.
    ``n_iter``: at most this many centre steps; ``tol``: stop when an iteration lowers E by at most tol |E|.

    Raises what ``assign`` raises, and ValueError for ``n_nodes`` outside 2 .. min(cells, 4096), a ``sigma`` that is not
    positive, a negative ``lam`` or ``tol``, a bad ``n_iter`` or ``init``, before any device use."""
    n_iter = _count(n_iter, "n_iter", 0, 1 << 20)
    lam = _positive(lam, "lam", zero_ok=True)
    tol = _positive(tol, "tol", zero_ok=True)
    if sigma is not None:
        sigma = _positive(sigma, "sigma")
    if isinstance(init, str) and init not in ("kmeans", "cells"):
        raise ValueError("init must be 'kmeans', 'cells' or an array of centres (got %r)" % (init,))
    _count(n_nodes, "n_nodes", 2, MAX_NODES)
    P, N, R, centres = _prepare(Y, n_nodes, "n_nodes", (None if isinstance(init, str) else init, seed))
    if isinstance(init, str) and init == "kmeans":
        centres = lloyd(P, centres, lambda C: assign(P, C, 0.0), KMEANS_ITER).centres
    if sigma is None:
        sigma = float(np.mean(assign(P, centres, 0.0).sq_distance.astype(np.float64)))
        if not sigma > 0:
            raise ValueError("every cell lies on a centre: give sigma")
    C, edges, energies, a, steps, converged = fit_tree(N, centres, lambda c: assign(P, c, sigma), lam * N / R, n_iter, tol)
    return PrincipalTree(P, C, edges, energies, sigma, lam, steps, converged, a.best)
