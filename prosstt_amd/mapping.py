"""
Mapping of cells onto the lineage tree, computed where the count matrix lies: on the device.  Given a tree that has genes and
any count matrix with size factors, every cell gets a score at every node of the tree; the best node gives its branch and
pseudotime, the scores give the posterior of that node and of every branch -- what the reference's
``examples/reproduce_axolotl.ipynb`` takes from MERLoT's ``Cells2TreeNodes`` and what ``probabilistic_branching.ipynb`` asks in
its soft form, by the tree's own likelihood.

    m = mapping.map_cells(X, sc, t)                                 # m.node, m.branches, m.pseudotime, m.branch_posterior
    tr = trends.expression_trends(X, sc, t, m.pseudotime, m.branches)
    f = fit.count_model(X, sc, m.node, tr.means)

The one pass over cells x nodes x genes runs in libprosstt_amd_mapping.so (include/prosstt_amd_mapping.h): the int32 matrix
times a node-by-gene float32 panel on the matrix cores, with the argmax and the log-sum-exps behind it.  The panel, the priors
and the posteriors are host numpy in binary64.  There is no CPU fallback for the pass.

Definitions.

Nodes.  As in ``trends``: the integer time steps of every branch in the row order of ``Tree.row_offsets()`` /
``simulation.cell_rows``; node (b, j) has the absolute pseudotime ``branch_times()[b][0] + j``.  ``node_table`` lists them.

The score of cell i at node r is the Poisson log-likelihood of its raw counts under mu_ig = s_i mean_rg, up to a constant of
the cell:  sum_g x_ig log mean_rg - s_i sum_g mean_rg (+ a log-prior of the node).  The negative binomial of the count model
does not factor into a product with a panel, and is out of scope.

``poisson_panel(means, gene_weights, floor)``, binary64 on the host, with w = gene_weights (ones by default) and
mm = max(means, floor):
    L[r][g] = w_g * (log mm[r][g] - mean over the nodes r' of log mm[r'][g]), rounded once to float32; a magnitude below
              2^-100 becomes 0 (no denormal reaches the matrix instruction)
    exposure[r] = sum_g w_g mm[r][g] - the mean over the nodes of that sum
The centring subtracts a constant of the cell from every score, so it changes no argmax and no posterior; it keeps
sum_g |x L| small, and with it the rounding error of the binary32 sums.  ``gene_weights = 1 / beta`` gives the quasi-Poisson
score of a count model whose variance is beta mu.

``node_scores``: for the int32 matrix X (N x G), size factors s (binary64), a panel P (R x G float32), an exposure m and
constants c (R, binary64) and ``genes_per_chain`` C (a multiple of 32 in 32 .. 4096):
    D[i][r]  the genes are cut into consecutive chains of C genes from gene 0; within a chain sum_g float(x_ig) P[r][g] is
             accumulated in binary32 by the matrix instruction's fused multiply-adds from 0 (a count of 2^24 or more is rounded
             once); the chain sums are converted to binary64 and added in ascending chain order
    S[i][r] = (D[i][r] - s_i m_r) + c_r in binary64, every operation rounded on its own
    best     the node of the largest S; ties go to the lower node; a NaN never wins
    lse      log sum_r exp(S[i][r] - best_score) + best_score, summed in a fixed order
    branch_lse  the same over the nodes of every branch, around the branch's own largest score
The results are a function of the row and the panel alone: they do not depend on the other rows, the stream, the tiling or
the layout of the matrix.  A matrix in chunks of cells is therefore just one call per chunk, with the same bits as the call
on the whole matrix.

With u = 2^-24 and A_ir = sum_g |x_ig| |P_rg|, S is within (min(C, G) + 2) u A + (ceil(G / C) + 3) 2^-53 (A + |s m| + |c|) of
the exact value: a shorter chain is a tighter bound.

Out of scope: the negative-binomial score; a float32 panel split into three bf16 parts (exact for counts up to 256 at 3/16
of the cost: the obvious next step); a split of the genes over blocks for matrices of few cells; inferring the topology;
alternating ``map_cells`` and ``expression_trends`` as an elastic-tree fit; several devices.
"""
from typing import Any, NamedTuple, Optional

import numpy as np

from . import _native
from . import device as _device
from .device import _ptr, _torch

GENES_PER_CHAIN = 256
MAX_CHAIN = 4096                        # PROSSTT_AMD_MAPPING_MAX_CHAIN
MAX_NODES = 65535 * 32                  # PROSSTT_AMD_MAPPING_MAX_NODES
TINY = 2.0 ** -100                      # panel entries below this magnitude are stored as 0
NEGATIVE, BRANCH_RANGE = 1, 2           # the bits of the pass's status word
STATUS_MESSAGES = (
    (NEGATIVE, "NEGATIVE", _device.NEGATIVE_ENTRY),
    (BRANCH_RANGE, "BRANCH_RANGE", "branch_offsets do not ascend from 0 to the number of nodes"),
)
PRIORS = ("uniform", "density")


class NodeScores(NamedTuple):
    """Per cell, in plan order: ``best`` (N,) int32 the node of the largest score, ``best_score`` and ``lse`` (N,) float64,
    ``branch_lse`` (N, B) float64, ``scores`` (N, R) float64 or None -- numpy arrays, or device tensors for ``out="torch"``."""
    best: Any
    best_score: Any
    lse: Any
    branch_lse: Any
    scores: Any = None


class NodeTable(NamedTuple):
    """The nodes of a tree: ``names`` the branches in ``tree.branches`` order, ``offsets`` (B + 1,) int64 the first node of
    every branch and R, ``branch_code`` (R,) int32 and ``pseudotime`` (R,) int64 of every node."""
    names: list
    offsets: np.ndarray
    branch_code: np.ndarray
    pseudotime: np.ndarray


class CellMapping(NamedTuple):
    """What ``map_cells`` returns, per cell in plan order: ``node`` (N,) int32, the row of ``simulation.cell_rows``;
    ``branches`` (N,) the node's branch name and ``branch_codes`` (N,) int32 its index in ``tree.branches``; ``pseudotime``
    (N,) int64 the node's absolute time step, what ``sample_density`` returns; ``loglik`` (N,) the best score; ``posterior``
    (N,) = exp(best score - lse), the posterior of the best node; ``branch_posterior`` (N, B), rows summing to 1; ``scores``
    (N, R) or None; ``branch_names`` the columns of ``branch_posterior``."""
    node: np.ndarray
    branches: np.ndarray
    branch_codes: np.ndarray
    pseudotime: np.ndarray
    loglik: np.ndarray
    posterior: np.ndarray
    branch_posterior: np.ndarray
    scores: Optional[Any]
    branch_names: list


def check_status(bits):
    """ValueError naming every bit of the pass's status word that is set."""
    said = ["status bit %s (%d): %s" % (name, bit, text) for bit, name, text in STATUS_MESSAGES if bits & bit]
    if said:
        raise ValueError("; ".join(said))
    if bits:
        raise RuntimeError("the pass set an unknown status bit (status %d)" % bits)


# ------------------------------------------------------------------------------------------------------- the panel

def poisson_panel(means, gene_weights=None, floor=1e-7):
    """(panel (R, G) float32, exposure (R,) float64) of node means (R, G) by the module docstring's definition; host numpy.

    Raises ValueError for means that are not a 2-D array of finite numbers >= 0, weights that are not G finite numbers
    >= 0, and a floor that is not positive and finite."""
    m = np.asarray(means)
    if m.ndim != 2 or m.dtype.kind not in "iuf" or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("means must be a (nodes, genes) array of numbers")
    m = m.astype(np.float64)
    if not np.all(np.isfinite(m)) or np.any(m < 0):
        raise ValueError("means must be finite and not negative")
    floor = float(floor)
    if not (np.isfinite(floor) and floor > 0):
        raise ValueError("floor must be positive and finite (got %r)" % (floor,))
    if gene_weights is None:
        w = np.ones(m.shape[1], dtype=np.float64)
    else:
        w = np.asarray(gene_weights)
        if w.shape != (m.shape[1],) or w.dtype.kind not in "iuf":
            raise ValueError("need one weight per gene: shape (%d,), not %s" % (m.shape[1], w.shape))
        w = w.astype(np.float64)
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError("gene weights must be finite and not negative")
    mm = np.maximum(m, floor)
    logs = np.log(mm)
    panel = (w[None, :] * (logs - logs.mean(axis=0)[None, :])).astype(np.float32, order="C")
    panel[np.abs(panel) < TINY] = 0.0
    total = (mm * w[None, :]).sum(axis=1)
    return panel, total - total.mean()


def node_table(tree):
    """``NodeTable`` of a tree; only ``topology``, ``time``, ``branches`` and ``root`` are read.  ValueError for a tree
    that is sharded over processes or has a branch without time steps."""
    from .trends import _Nodes
    nodes = _Nodes(tree)
    offsets = np.concatenate([nodes.offset, [nodes.R]]).astype(np.int64)
    code = np.repeat(np.arange(len(nodes.names), dtype=np.int32), nodes.length)
    return NodeTable(list(nodes.names), offsets, code, nodes.node_time.astype(np.int64))


# ------------------------------------------------------------------------------------------------------- the scores

def _genes_per_chain(v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 32 <= v <= MAX_CHAIN or v % 32:
        raise ValueError("genes_per_chain must be a multiple of 32 in 32 .. %d (got %r)" % (MAX_CHAIN, v))
    return int(v)


def _size_factors(sc, n_cells):
    if sc is None:
        return np.ones(n_cells, dtype=np.float64)
    torch = _torch()
    if isinstance(sc, torch.Tensor):
        sc = sc.detach().cpu().numpy()
    s = np.asarray(sc)
    if s.shape != (n_cells,) or s.dtype.kind not in "iuf":
        raise ValueError("need one size factor per cell: shape (%d,), not %s" % (n_cells, s.shape))
    s = s.astype(np.float64)
    if not np.all(np.isfinite(s)) or np.any(s < 0):
        raise ValueError("size factors must be finite and not negative")
    return s


def _per_node(values, R, name):
    v = np.asarray(values)
    if v.shape != (R,) or v.dtype.kind not in "iuf":
        raise ValueError("%s must hold one number per node: shape (%d,), not %s" % (name, R, v.shape))
    v = v.astype(np.float64)
    if not np.all(np.isfinite(v)):
        raise ValueError("%s must be finite" % name)
    return v


def _offsets(branch_offsets, R):
    if branch_offsets is None:
        return np.array([0, R], dtype=np.int64)
    o = np.asarray(branch_offsets)
    if o.ndim != 1 or o.shape[0] < 2 or o.dtype.kind not in "iu":
        raise ValueError("branch_offsets must be a 1-D integer array of at least two entries")
    o = o.astype(np.int64)
    if o[0] != 0 or o[-1] != R or np.any(np.diff(o) < 0):
        raise ValueError("branch_offsets must ascend from 0 to the number of nodes (%d)" % R)
    return o


def _panel(panel):
    """(the panel as given, R, G, on_device) after the checks that need no device."""
    torch = _torch()
    if isinstance(panel, torch.Tensor):
        if panel.dtype != torch.float32 or panel.dim() != 2:
            raise ValueError("the panel must be a (nodes, genes) float32 array")
        if panel.device.type == "cpu":
            panel = panel.detach().numpy()
        elif panel.shape[1] > 1 and panel.stride(1) != 1:
            raise ValueError("a device panel needs unit column stride")
    if isinstance(panel, np.ndarray):
        if panel.dtype != np.float32 or panel.ndim != 2:
            raise ValueError("the panel must be a (nodes, genes) float32 array")
    elif not isinstance(panel, torch.Tensor):
        raise ValueError("the panel must be a (nodes, genes) float32 array")
    R, G = (int(v) for v in panel.shape)
    if R < 1 or R > MAX_NODES:
        raise ValueError("mapping takes 1 .. %d nodes (got %d)" % (MAX_NODES, R))
    return panel, R, G, isinstance(panel, torch.Tensor)


def node_scores(X, sc, panel, exposure, constants=None, branch_offsets=None, *, genes_per_chain=GENES_PER_CHAIN,
                scores=False, out="numpy", node_tile=0):
    """``NodeScores`` of an int32 device count matrix against a panel (the module docstring's definition).

    ``X``: anything ``device.CountMatrix`` accepts (a device tensor with unit column stride, or a
    ``device.PresentedCounts``), read in place; the per-cell results of a presented matrix are scattered to plan order.
    ``sc``: one size factor per cell in plan order (host array or tensor, used as binary64), or None for all ones.
    ``panel``: (R, G) float32, a host array or a device tensor (kept by the caller between the chunks of a matrix);
    ``exposure``: (R,); ``constants``: (R,) or None for zeros; ``branch_offsets``: (B + 1,) integers ascending from 0 to R,
    None for one branch of all nodes.  ``scores=True`` also returns the N x R scores.  ``out``: "numpy", or "torch" for
    device tensors.  ``node_tile``: 32-node tiles per block of the pass, 1 .. 4, or 0 for the library's rule; the results do
    not depend on it.  Runs on the current stream.

    Rows are independent: a matrix in chunks of cells is one call per chunk, with the same bits as one call on the whole.

    Raises TypeError for a host matrix or another dtype; ValueError for a CPU tensor, a panel, exposure, constants or size
    factors of the wrong type, shape or with non-finite values, ``branch_offsets`` that do not ascend from 0 to R, a bad
    ``genes_per_chain``, ``node_tile`` or ``out``, and for each bit of the pass's status word, with the bit named (a
    negative count: ``device.NEGATIVE_ENTRY``).  The argument checks come before any device use."""
    result, bits = _node_scores(X, sc, panel, exposure, constants, branch_offsets, genes_per_chain, scores, out, node_tile)
    check_status(bits)
    return result


def _node_scores(X, sc, panel, exposure, constants=None, branch_offsets=None, genes_per_chain=GENES_PER_CHAIN, scores=False,
                 out="numpy", node_tile=0):
    """``node_scores`` up to the verdict: (NodeScores, the pass's status word)."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    genes_per_chain = _genes_per_chain(genes_per_chain)
    if isinstance(node_tile, (bool, np.bool_)) or not isinstance(node_tile, (int, np.integer)) or not 0 <= node_tile <= 4:
        raise ValueError("node_tile must be an integer 0 .. 4 (got %r)" % (node_tile,))
    m = _device.CountMatrix(X, "mapping.node_scores")
    if m.N < 1 or m.G < 1:
        raise ValueError("mapping.node_scores needs at least one cell and one gene (got %d x %d)" % (m.N, m.G))
    if m.N >= 1 << 31:
        raise ValueError("mapping.node_scores takes fewer than 2^31 cells")
    panel, R, Gp, panel_on_device = _panel(panel)
    if Gp != m.G:
        raise ValueError("the panel has %d genes, the matrix %d" % (Gp, m.G))
    s = _size_factors(sc, m.N)
    expo = _per_node(exposure, R, "exposure")
    cons = np.zeros(R, dtype=np.float64) if constants is None else _per_node(constants, R, "constants")
    offsets = _offsets(branch_offsets, R)
    B = offsets.shape[0] - 1
    m = m.on_device()
    if panel_on_device and panel.device != m.device:
        raise ValueError("the panel lies on another device than the matrix")
    L = _device.need_device("mapping")
    torch = _torch()
    dev = m.device
    if m.cell_of_row is not None:
        s = s[m.cell_of_row]                         # the size factor of every ROW
    with torch.cuda.device(dev):
        if not panel_on_device:
            panel = torch.as_tensor(np.array(panel, order="C")).to(dev)       # (a copy: the caller's may be read-only)
        ldp = panel.stride(0) if R > 1 else m.G
        if ldp < m.G:
            raise ValueError("the panel's rows overlap (row stride %d < %d genes)" % (ldp, m.G))
        s_d, m_d, c_d, o_d = (torch.as_tensor(np.ascontiguousarray(a)).to(dev) for a in (s, expo, cons, offsets))
        ws = _device.workspace("mapping", "prosstt_amd_mapping_workspace_bytes", dev, m.N, m.G, R, B)
        best = torch.empty(m.N, dtype=torch.int32, device=dev)
        best_score = torch.empty(m.N, dtype=torch.float64, device=dev)
        lse = torch.empty(m.N, dtype=torch.float64, device=dev)
        branch_lse = torch.empty((m.N, B), dtype=torch.float64, device=dev)
        S = torch.empty((m.N, R), dtype=torch.float64, device=dev) if scores else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _native.check(L.prosstt_amd_mapping_node_scores_tiled(
            m.stream(), _ptr(m.X), m.N, m.G, m.ld, _ptr(s_d), _ptr(panel), ldp, R, _ptr(m_d), _ptr(c_d), _ptr(o_d), B,
            genes_per_chain, int(node_tile), _ptr(ws), ws.numel(), _ptr(best), _ptr(best_score), _ptr(lse), _ptr(branch_lse),
            _ptr(S), _ptr(status)), "mapping")
        bits = int(status.item())
        per_row = (best, best_score, lse, branch_lse) + ((S,) if scores else ())
        if out == "numpy":
            per_cell = _device.to_plan_order(m.cell_of_row, *(a.cpu().numpy() for a in per_row))
        elif m.cell_of_row is None:
            per_cell = per_row
        else:
            row_of_cell = torch.as_tensor(_device.inverse_permutation(m.cell_of_row)).to(dev)
            per_cell = tuple(a.index_select(0, row_of_cell) for a in per_row)
    return NodeScores(*per_cell), bits


# ------------------------------------------------------------------------------------------------------- the mapping

def _tree_parts(tree):
    """(the tree, its density per node, a function that returns its (R, G) node means) of a ``Tree`` with genes or a
    ``trends.Trends``.  The means of a ``Tree`` are read from the device, so they come last."""
    from .trends import Trends
    if isinstance(tree, Trends):
        return tree.tree, np.asarray(tree.density, dtype=np.float64), lambda: np.asarray(tree.means, dtype=np.float64)
    from .fit import simulation_means
    density = np.concatenate([np.asarray(tree.density[b], dtype=np.float64) for b in tree.branches])
    return tree, density, lambda: simulation_means(tree)


def _prior(prior, density, R):
    if isinstance(prior, str):
        if prior not in PRIORS:
            raise ValueError("prior must be 'uniform', 'density' or an array of one log-prior per node (got %r)" % (prior,))
        if prior == "uniform":
            return np.zeros(R, dtype=np.float64)
        if density.shape != (R,) or not np.all(np.isfinite(density)) or np.any(density <= 0):
            raise ValueError("prior='density' needs a positive density at every node: %d of %d nodes have none"
                             % (int(np.count_nonzero(~(density > 0))), R))
        return np.log(density)
    return _per_node(prior, R, "prior")


def map_cells(X, sc, tree, *, gene_weights=None, prior="uniform", floor=1e-7, genes_per_chain=GENES_PER_CHAIN,
              scores=False, out="numpy"):
    """``CellMapping`` of an int32 device count matrix onto ``tree``.

    ``X``, ``sc``, ``genes_per_chain``: as for ``node_scores``.  ``tree``: a ``Tree`` with genes (the means are
    ``fit.simulation_means(tree)``) or a ``trends.Trends`` (its ``means``); only the tree's ``topology``, ``time``,
    ``branches``, ``root`` and means are read.  ``gene_weights``, ``floor``: as for ``poisson_panel``.  ``prior``:
    "uniform", "density" (the log of ``tree.density``, or of the trends' density) or an array of one log-prior per node; it
    is the constant of ``node_scores``.  ``scores=True`` keeps the N x R scores; ``out`` says where (the other fields are
    host arrays either way).

    ``m.pseudotime`` and ``m.branches`` are valid inputs of ``trends.expression_trends`` and ``simulation.cell_rows``, and
    ``m.node`` is the row label ``fit.count_model`` takes.  Rows are independent: a matrix in chunks of cells is one call
    per chunk with the same bits.

    Raises what ``node_scores`` and ``poisson_panel`` raise, and ValueError for a tree that is sharded over processes, that
    has no genes, whose means do not fit its nodes, and for a prior that is not one of the above (a density with zeros
    under "density"); every argument refusal comes before any device use of the pass."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    genes_per_chain = _genes_per_chain(genes_per_chain)
    cm = _device.CountMatrix(X, "mapping.map_cells")
    base, density, read_means = _tree_parts(tree)
    table = node_table(base)
    R = int(table.offsets[-1])
    constants = _prior(prior, density, R)
    means = read_means()
    if means.ndim != 2 or means.shape[0] != R:
        raise ValueError("the tree has %d nodes, its means %s" % (R, means.shape))
    if means.shape[1] != cm.G:
        raise ValueError("the tree has %d genes, the matrix %d" % (means.shape[1], cm.G))
    panel, exposure = poisson_panel(means, gene_weights, floor)
    got = node_scores(X, sc, panel, exposure, constants, table.offsets, genes_per_chain=genes_per_chain, scores=scores,
                      out=out)
    host = [a.detach().cpu().numpy() if out == "torch" else a for a in got[:4]]
    node, loglik, lse, branch_lse = host
    top = branch_lse.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        weights = np.exp(branch_lse - top)
        branch_posterior = weights / weights.sum(axis=1, keepdims=True)
        posterior = np.exp(loglik - lse)
    codes = table.branch_code[node]
    names = np.asarray(table.names)[codes]
    return CellMapping(node, names, codes, table.pseudotime[node], loglik, posterior, branch_posterior, got.scores,
                       table.names)
