"""
Spatial autocorrelation of genes on the cell graph, computed where the count matrix and the graph lie: on the device.
Which genes follow the structure of the graph, without choosing a clustering or a branching first (scanpy's
``metrics.morans_i`` and ``metrics.gearys_c`` on ``obsp["connectivities"]``), and the graph-smoothed expression W.A that one
colours a layout with.

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    nb = neighbors.knn(embed.pca(X, sc).scores, 14, out="torch")
    ac = autocorr.autocorrelation(X, sc, nb)              # ac.morans_i, ac.z_i, ac.pvals_adj, ac.order[:20]
    autocorr.smooth(X, sc, nb)                            # (cells, genes) float32: each cell's weighted neighbour mean

The one pass that couples the graph with the cells x genes matrix runs in libprosstt_amd_autocorr.so
(include/prosstt_amd_autocorr.h): per gene four binary64 sums over cells and edges of a = the float32 entry log1p(x / s) of
``embed.LogNormalized``, bit for bit, centred inside the kernel.  The gene means come from ``LogNormalized.gene_moments()``
(one more read of the matrix); the graph's constants and the statistics are host numpy and scipy in binary64.  There is no
CPU fallback for the pass.

scanpy is not installed here and was not run: the definitions are Moran's and Geary's as scanpy states them, from memory,
and the moments under permutation are Cliff and Ord's (1981), checked in tests/test_autocorr_model.py against the full
enumeration of all permutations of seven cells.

Definitions.  W: any CSR matrix of cells x cells with binary64 weights; it need not be symmetric.  N cells, W0 = sum w,
mu_g = S1_g / N, z = a - mu, everything in binary64:

    I_g = (N / W0) * (cross_g / m2_g),             cross = sum_i z_i sum_j w_ij z_j,  m2 = sum_i z_i^2
    C_g = ((N - 1) / (2 W0)) * (sqdiff_g / m2_g),  sqdiff = sum_i sum_j w_ij (a_i - a_j)^2

    S1 = 1/2 sum_ij (w_ij + w_ji)^2,  S2 = sum_i (sum_j w_ij + sum_j w_ji)^2,  b2 = N m4 / m2^2,  m4 = sum_i z_i^4
    E(I) = -1 / (N - 1),  E(C) = 1, and the exact variances under random permutation of the cells:
    Var(I) = [N ((N^2 - 3N + 3) S1 - N S2 + 3 W0^2) - b2 ((N^2 - N) S1 - 2N S2 + 6 W0^2)] / ((N - 1)(N - 2)(N - 3) W0^2) - E(I)^2
    Var(C) = [(N - 1) S1 (N^2 - 3N + 3 - (N - 1) b2) - 1/4 (N - 1) S2 (N^2 + 3N - 6 - (N^2 - N + 2) b2)
              + W0^2 (N^2 - 3 - (N - 1)^2 b2)] / (N (N - 2)(N - 3) W0^2)
    z_i = (I - E(I)) / sqrt(Var(I)),  z_c = (C - 1) / sqrt(Var(C)),  pvals = the normal upper tail of z_i

A gene with m2 = 0 gets NaN for every statistic; N < 4 gives NaN variances; W0 = 0 gives NaN.

A matrix in chunks of cells (``sample_density_chunks``) is out of scope: the graph couples the cells, so the whole matrix
must lie on one device.  Column slices of a wider tensor work; for a subset of genes use ``hvg.select_genes`` first, the
kernels take no gene list.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, embed
from . import device as _device
from . import graph as _graph
from .device import _ptr, _torch
from .markers import _host, _rows_per_block, benjamini_hochberg

NEGATIVE, INDEX_RANGE = 1, 2                    # the bits of the kernels' status word
GENE_TILES = (0, 64, 256)                       # genes per wave; 0: the library's rule


class GraphSums(NamedTuple):
    """What one pass over graph and matrix leaves, per gene (G,) float64: ``mean`` (the mu the kernel centred with),
    ``cross``, ``sqdiff``, ``m2``, ``m4`` of the module docstring (numpy arrays, or device tensors for ``out="torch"``; ``mean``
    is always a host array); and of the graph: ``n_cells``, ``w_total`` = W0, ``s1``, ``s2`` (host floats)."""
    n_cells: int
    w_total: float
    mean: np.ndarray
    cross: Any
    sqdiff: Any
    m2: Any
    m4: Any
    s1: float
    s2: float


class AutoCorrelation(NamedTuple):
    """(G,) float64 host arrays: ``morans_i``, ``gearys_c``, ``z_i``, ``z_c``, ``pvals`` (upper tail of z_i), ``pvals_adj``
    (Benjamini-Hochberg over the genes with a p-value); ``expected_i`` = -1 / (N - 1); ``order``: int64 gene indices by z_i
    descending, ties to the lower index, NaN last (the first ``n_genes`` of them)."""
    morans_i: np.ndarray
    gearys_c: np.ndarray
    expected_i: float
    z_i: np.ndarray
    z_c: np.ndarray
    pvals: np.ndarray
    pvals_adj: np.ndarray
    order: np.ndarray


# ------------------------------------------------------------------------------------------------------ the graph

def _graph_arrays(graph, n_cells, dev):
    """(indptr, indices, data) of an accepted graph as it came (host arrays or device tensors), or None for a ``Neighbors``
    (whose connectivities the device computes); the dtypes, the shapes, N and the device are checked.  Touches no device."""
    torch = _torch()
    if not isinstance(graph, (_graph.Connectivities, _graph.Transitions)):
        idx, d2, N, _ = _graph._check_neighbors(graph)
        arrays = (idx, d2)
        out = None
    else:
        names = (("indptr", np.int64, torch.int64), ("indices", np.int32, torch.int32), ("data", np.float64, torch.float64))
        arrays = []
        for name, np_dtype, t_dtype in names:
            arr = getattr(graph, name)
            if isinstance(arr, torch.Tensor) and arr.device.type == "cpu":
                arr = arr.detach().numpy()
            want = t_dtype if isinstance(arr, torch.Tensor) else np.dtype(np_dtype)
            if not isinstance(arr, (torch.Tensor, np.ndarray)) or arr.dtype != want or len(arr.shape) != 1:
                raise ValueError("%s must be a 1-D %s array" % (name, np.dtype(np_dtype).name))
            arrays.append(arr)
        N = int(arrays[0].shape[0]) - 1
        if N < 1:
            raise ValueError("indptr needs at least two entries")
        if int(arrays[1].shape[0]) != int(arrays[2].shape[0]):
            raise ValueError("indices and data differ in length")
        out = tuple(arrays)
    if N != n_cells:
        raise ValueError("the graph has %d cells, the matrix %d" % (N, n_cells))
    for arr in arrays:
        if isinstance(arr, torch.Tensor) and arr.device != dev:
            raise ValueError("the graph lies on %s, the matrix on %s" % (arr.device, dev))
    return out


def _device_graph(graph, arrays, dev):
    """(indptr, indices, data) as checked device tensors on ``dev``: ``graph._as_connectivities`` checks a caller's CSR
    arrays, since the kernels trust them, and computes a ``Neighbors``' connectivities as ``cluster.louvain`` does."""
    torch = _torch()
    L = _device.need_device("graph")
    with torch.cuda.device(dev):
        if arrays is None:
            g = _graph._as_connectivities(L, graph)
        else:
            g = _graph._as_connectivities(L, _graph.Connectivities(*arrays, None, None))
    return g.indptr, g.indices, g.data


def graph_constants(indptr, indices, data):
    """(W0, S1, S2) of a CSR matrix (host arrays or device tensors) by the module docstring's definitions: scipy on the
    host, binary64.  W0 = ``numpy.sum(data)``."""
    import scipy.sparse as sparse
    indptr, indices, data = (_host(a) for a in (indptr, indices, data))
    n = indptr.shape[0] - 1
    W = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    both = (W + W.T).tocsr()
    s1 = 0.5 * float(np.sum(both.data * both.data))
    margins = np.asarray(W.sum(axis=1)).ravel() + np.asarray(W.sum(axis=0)).ravel()
    return float(np.sum(data)), s1, float(np.sum(margins * margins))


# ----------------------------------------------------------------------------------------------------------- sums

def _gene_tile(v):
    if isinstance(v, bool) or v not in GENE_TILES:
        raise ValueError("gene_tile must be 0, 64 or 256 (got %r)" % (v,))
    return int(v)


def _host_checks(counts, size_factors, graph):
    """(CountMatrix, graph arrays or None) after every refusal that needs no device."""
    m = embed._counts(counts)
    embed._inverse_sizes(size_factors, m.N)
    arrays = _graph_arrays(graph, m.N, m.X.device)
    return m, arrays


def _raise_status(status):
    bits = int(status.item())
    if bits & NEGATIVE:
        raise ValueError(_device.NEGATIVE_ENTRY)
    if bits:
        raise RuntimeError("the pass refused the graph's arrays (status %d)" % bits)


def _operands(counts, size_factors, graph, arrays, m):
    """The operator, the device CSR arrays (indptr, indices, data) as the graph has them, the columns as the kernels take
    them (the matrix row of every neighbour: one gather per call for a presented matrix, so that the kernels reach a
    neighbour's counts in one hop) and the int32 cell_of_row tensor (None for a matrix in plan order)."""
    torch = _torch()
    op = embed.LogNormalized(counts, size_factors)
    csr = _device_graph(graph, arrays, op.device)
    rows, cell_of_row = csr[1], None
    if m.cell_of_row is not None:
        with torch.cuda.device(op.device):
            row_of_cell = torch.as_tensor(_device.inverse_permutation(m.cell_of_row).astype(np.int32)).to(op.device)
            rows = row_of_cell[csr[1].to(torch.int64)]
            cell_of_row = torch.as_tensor(np.asarray(m.cell_of_row).astype(np.int32)).to(op.device)
    return op, csr, rows, cell_of_row


def graph_sums(counts, size_factors, graph, *, rows_per_block=0, gene_tile=0, mean=None, out="numpy"):
    """``GraphSums`` of an int32 device count matrix and a graph of its cells.

    ``counts`` and ``size_factors``: as for ``embed.LogNormalized`` (a device tensor with unit column stride or a
    ``device.PresentedCounts``, which is read in place and summed in the order of its rows; positive host size factors per cell
    in plan order).  ``graph``: a
    ``graph.Connectivities`` or ``graph.Transitions`` (host arrays, or device tensors on the matrix's device; node i is cell i
    in plan order), or a ``neighbors.Neighbors``, whose connectivities are computed first.  ``rows_per_block``: cells per
    block of the pass, 0 for the library's rule max(16, ceil(cells / 512)); the sums are equal to the bit for equal values and
    equal row orders of the matrix.
    ``gene_tile``: 64 or 256 genes per wave, 0 for the library's rule; the sums do not depend on it.  ``mean``: the (G,)
    binary64 mu to centre with (None: S1 / N of ``gene_moments()``).  Given mu, a gene's sums depend on N, ``rows_per_block``
    and the matrix's row order alone, so a column slice gives the bits of the full call; ``gene_moments`` itself adds in an
    order that depends on ceil(G / 1024), so pass ``mean`` to slice a matrix of more than 1024 genes to the bit.
    ``out``: "numpy", or "torch" for device tensors.  Runs on the current stream.

    Raises TypeError for a host array or another dtype; ValueError for a CPU tensor, bad size factors, a graph of another
    number of cells or on another device, arrays that are not a CSR matrix, a bad ``rows_per_block``, ``gene_tile``, ``mean``
    or ``out``, or a negative count.  The argument checks come before any device use."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    rows_per_block = _rows_per_block(rows_per_block)
    gene_tile = _gene_tile(gene_tile)
    m, arrays = _host_checks(counts, size_factors, graph)
    if mean is not None:
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        if mean.shape != (m.G,) or not np.all(np.isfinite(mean)):
            raise ValueError("mean must hold one finite value per gene: shape (%d,)" % m.G)
    op, (indptr, indices, data), rows, cell_of_row = _operands(counts, size_factors, graph, arrays, m)
    L = _device.need_device("autocorr")
    torch = _torch()
    N, G = op.shape
    dev = op.device
    with torch.cuda.device(dev):
        if mean is None:
            mean = op.gene_moments()[0] / N
        mu = torch.as_tensor(mean).to(dev)
        ws = _device.workspace("autocorr", "prosstt_amd_autocorr_workspace_bytes", dev, N, G, rows_per_block)
        sums = torch.empty((4, G), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nnz = indices.numel()
        _native.check(L.prosstt_amd_autocorr_gene_sums(
            _device.current_stream(dev), _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(cell_of_row), _ptr(indptr),
            _ptr(rows) if nnz else None, _ptr(data) if nnz else None, nnz, _ptr(mu), rows_per_block, gene_tile, _ptr(ws),
            ws.numel(), _ptr(sums[0]), _ptr(sums[1]), _ptr(sums[2]), _ptr(sums[3]), _ptr(status)), "autocorr")
        _raise_status(status)
        w0, s1, s2 = graph_constants(indptr, indices, data)
        if out == "numpy":
            sums = sums.cpu().numpy()
    return GraphSums(N, w0, mean, sums[0], sums[1], sums[2], sums[3], s1, s2)


def smooth(counts, size_factors, graph, *, normalize=True, gene_tile=0, out="torch"):
    """The graph-smoothed expression: (cells, genes) float32, cells in plan order, row i = sum_j w_ij a_j over the entries of
    the graph's row i in their order (binary64, every operation rounded on its own), times 1 / d_i with d_i = sum_j w_ij for
    ``normalize=True`` (the weighted mean of the neighbours), rounded once to float32.  A cell whose weights add up to 0 (one
    without entries) gives zeros.  A diagonal entry counts like any other: add one for a MAGIC-style average that keeps the
    cell itself.  Arguments and refusals as for ``graph_sums``; ``out``: "torch" (a device tensor) or "numpy"."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError("normalize must be True or False (got %r)" % (normalize,))
    gene_tile = _gene_tile(gene_tile)
    m, arrays = _host_checks(counts, size_factors, graph)
    op, (indptr, indices, data), rows, cell_of_row = _operands(counts, size_factors, graph, arrays, m)
    L = _device.need_device("autocorr")
    torch = _torch()
    N, G = op.shape
    dev = op.device
    with torch.cuda.device(dev):
        panel = torch.empty((N, G), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        nnz = indices.numel()
        _native.check(L.prosstt_amd_autocorr_smooth(
            _device.current_stream(dev), _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(cell_of_row), _ptr(indptr),
            _ptr(rows) if nnz else None, _ptr(data) if nnz else None, nnz, int(bool(normalize)), gene_tile, _ptr(panel), G,
            _ptr(status)), "autocorr")
        _raise_status(status)
        return panel if out == "torch" else panel.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ statistics

def permutation_moments(n_cells, w_total, s1, s2, b2):
    """(E(I), Var(I), Var(C)) under random permutation of the cells, by the module docstring's formulas: ``b2`` the (G,)
    kurtosis N m4 / m2^2 of every gene, the rest the graph's constants.  Fewer than four cells or W0 = 0 give NaN variances."""
    N, W0, S1, S2 = float(n_cells), float(w_total), float(s1), float(s2)
    b2 = np.asarray(b2, dtype=np.float64)
    EI = -1.0 / (N - 1) if N > 1 else np.nan
    if N < 4 or W0 == 0:
        return EI, np.full(b2.shape, np.nan), np.full(b2.shape, np.nan)
    W2 = W0 * W0
    var_i = (N * ((N * N - 3 * N + 3) * S1 - N * S2 + 3 * W2) - b2 * ((N * N - N) * S1 - 2 * N * S2 + 6 * W2)) \
        / ((N - 1) * (N - 2) * (N - 3) * W2) - EI * EI
    var_c = ((N - 1) * S1 * (N * N - 3 * N + 3 - (N - 1) * b2)
             - 0.25 * (N - 1) * S2 * (N * N + 3 * N - 6 - (N * N - N + 2) * b2)
             + W2 * (N * N - 3 - (N - 1) ** 2 * b2)) / (N * (N - 2) * (N - 3) * W2)
    return EI, var_i, var_c


def statistics(gs, n_genes=None):
    """``AutoCorrelation`` of a ``GraphSums`` by the module docstring's formulas, host numpy in binary64."""
    import scipy.stats
    if not isinstance(gs, GraphSums):
        raise TypeError("statistics takes a GraphSums, not %s" % type(gs).__name__)
    cross, sqdiff, m2, m4 = (np.asarray(_host(a), dtype=np.float64) for a in (gs.cross, gs.sqdiff, gs.m2, gs.m4))
    G = m2.shape[0]
    if n_genes is None:
        n_genes = G
    elif isinstance(n_genes, bool) or int(n_genes) != n_genes or not 1 <= n_genes <= G:
        raise ValueError("need an integer 1 <= n_genes <= genes = %d (got %r)" % (G, n_genes))
    N, W0 = float(gs.n_cells), float(gs.w_total)
    nan = np.full(G, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        flat = ~(m2 > 0)
        I = np.where(flat, np.nan, (N / W0 if W0 != 0 else np.nan) * (cross / m2))
        C = np.where(flat, np.nan, ((N - 1) / (2 * W0) if W0 != 0 else np.nan) * (sqdiff / m2))
        EI, var_i, var_c = permutation_moments(gs.n_cells, W0, gs.s1, gs.s2, N * m4 / (m2 * m2))
        z_i = np.where(flat, np.nan, (I - EI) / np.sqrt(var_i))
        z_c = np.where(flat, np.nan, (C - 1.0) / np.sqrt(var_c))
    p = scipy.stats.norm.sf(z_i)
    have = ~np.isnan(p)
    adj = nan.copy()
    if have.any():
        adj[have] = benjamini_hochberg(p[have])
    key = np.where(np.isnan(z_i), -np.inf, z_i)
    order = np.lexsort((np.arange(G), -key, np.isnan(z_i)))[:int(n_genes)].astype(np.int64)
    return AutoCorrelation(I, C, EI, z_i, z_c, p, adj, order)


def autocorrelation(counts, size_factors, graph, n_genes=None, *, rows_per_block=0):
    """The whole call: ``statistics(graph_sums(counts, size_factors, graph), n_genes)``.  ``n_genes``: how many of ``order`` to
    keep, 1 .. genes (None: all)."""
    G = embed._counts(counts).G
    if n_genes is not None and (isinstance(n_genes, bool) or int(n_genes) != n_genes or not 1 <= n_genes <= G):
        raise ValueError("need an integer 1 <= n_genes <= genes = %d (got %r)" % (G, n_genes))
    return statistics(graph_sums(counts, size_factors, graph, rows_per_block=rows_per_block), n_genes)


def morans_i(counts, size_factors, graph):
    """Moran's I of every gene, (G,) float64 (scanpy's ``metrics.morans_i``)."""
    return statistics(graph_sums(counts, size_factors, graph)).morans_i


def gearys_c(counts, size_factors, graph):
    """Geary's C of every gene, (G,) float64 (scanpy's ``metrics.gearys_c``)."""
    return statistics(graph_sums(counts, size_factors, graph)).gearys_c
