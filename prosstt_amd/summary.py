"""
Summary statistics of a count matrix, computed where the matrix lies: on the device.

The reference matches a simulation to real data through five summaries of a count matrix X (every compare_*.ipynb
notebook, and the inputs of sim_utils.learn_data_summary, sim_utils.py:670-719):

    np.mean(X, axis=0)   np.var(X, axis=0)   np.sum(X == 0, axis=0)   np.sum(X == 0, axis=1)   np.sum(X, axis=1)

``count_summary`` forms the exact integer sums behind all five in one read of an int32 device matrix
(libprosstt_amd_stats.so, include/prosstt_amd_stats.h), and only O(cells + genes) numbers cross PCIe;
``sample_density_summary`` samples ``simulation.sample_density``'s matrix chunk by chunk and summarises it without the
matrix ever leaving the device.  Means and variances are formed from the exact integers on the host.

    s = summary.count_summary(sim.draw_counts(..., out="torch"))
    sut.learn_data_summary(s.cell_stats(), s.gene_stats(), relative_means)

There is no CPU fallback: host arrays are refused.
"""

import numpy as np
import pandas as pd

from . import _native
from . import device as _device
from .device import _torch

_U64 = 1 << 64


class CountSummary:
    """The exact sums of an (n_cells x n_genes) count matrix, and what the reference computes from them.

    Exact integer arrays: ``gene_sum`` (sum over cells, int64), ``gene_sumsq`` (sum of squares: an object array of Python
    ints -- it can exceed 64 bits), ``gene_zeros``, ``cell_total`` (library sizes), ``cell_zeros`` (int64).
    Derived binary64 values: ``gene_means`` (correctly rounded sum / n_cells) and ``gene_var`` (ddof 0, correctly rounded
    (n_cells * sumsq - sum^2) / n_cells^2).  Cells are in plan order."""

    def __init__(self, gene_sum, gene_sumsq, gene_zeros, cell_total, cell_zeros):
        self.gene_sum = np.asarray(gene_sum, dtype=np.int64)
        self.gene_sumsq = np.array([int(v) for v in gene_sumsq], dtype=object)
        self.gene_zeros = np.asarray(gene_zeros, dtype=np.int64)
        self.cell_total = np.asarray(cell_total, dtype=np.int64)
        self.cell_zeros = np.asarray(cell_zeros, dtype=np.int64)
        self.n_cells = int(self.cell_total.shape[0])
        self.n_genes = int(self.gene_sum.shape[0])
        if self.cell_zeros.shape != (self.n_cells,):
            raise ValueError("cell_total and cell_zeros must have one entry per cell")
        if self.gene_sumsq.shape != (self.n_genes,) or self.gene_zeros.shape != (self.n_genes,):
            raise ValueError("gene_sum, gene_sumsq and gene_zeros must have one entry per gene")
        self._means = self._var = None

    @classmethod
    def from_parts(cls, gene_sum, gene_sumsq, gene_zeros, cell_total, cell_zeros):
        """A summary from its integer parts (``gene_sumsq``: Python ints, or anything ``int()`` takes exactly)."""
        return cls(gene_sum, gene_sumsq, gene_zeros, cell_total, cell_zeros)

    @classmethod
    def concat(cls, parts):
        """The summary of the matrices of ``parts`` stacked over cells: cells appended in order, gene sums added."""
        parts = list(parts)
        if not parts:
            raise ValueError("concat needs at least one summary")
        if len({p.n_genes for p in parts}) != 1:
            raise ValueError("the summaries cover different numbers of genes")
        gene_sum = sum((p.gene_sum.astype(object) for p in parts[1:]), parts[0].gene_sum.astype(object))
        if len(gene_sum) and max(gene_sum) >= 1 << 63:
            raise OverflowError("a gene's sum exceeds int64")
        return cls(np.array(gene_sum, dtype=np.int64) if len(gene_sum) else gene_sum.astype(np.int64),
                   sum((p.gene_sumsq for p in parts[1:]), parts[0].gene_sumsq),
                   sum((p.gene_zeros for p in parts[1:]), parts[0].gene_zeros),
                   np.concatenate([p.cell_total for p in parts]), np.concatenate([p.cell_zeros for p in parts]))

    @property
    def gene_means(self):
        if self._means is None:
            n = self.n_cells
            means = self.gene_sum.astype(np.float64) / n             # exact operands below 2^53: one rounding
            big = np.flatnonzero(self.gene_sum >= 1 << 53)
            for g in big:
                means[g] = int(self.gene_sum[g]) / n                 # (int / int is correctly rounded)
            self._means = means
        return self._means

    @property
    def gene_var(self):
        if self._var is None:
            n = self.n_cells
            nn = n * n
            self._var = np.array([(n * s2 - s1 * s1) / nn for s1, s2 in zip(self.gene_sum.tolist(), self.gene_sumsq)],
                                 dtype=np.float64).reshape(self.n_genes)
        return self._var

    def cell_stats(self):
        """DataFrame, index ["total", "zeros"], one column per cell (plan order): learn_data_summary's ``cell_stats``."""
        return pd.DataFrame(np.vstack([self.cell_total, self.cell_zeros]), index=["total", "zeros"])

    def gene_stats(self):
        """DataFrame, index ["means", "var", "zeros"], one column per gene: learn_data_summary's ``gene_stats``."""
        return pd.DataFrame(np.vstack([self.gene_means, self.gene_var, self.gene_zeros.astype(np.float64)]),
                            index=["means", "var", "zeros"])

    def __repr__(self):
        return "CountSummary(n_cells=%d, n_genes=%d)" % (self.n_cells, self.n_genes)


def _matrix(counts):
    """The checked device view (device.CountMatrix) of an accepted input, or raise."""
    m = _device.CountMatrix(counts, "count_summary")
    if m.N == 0:
        raise ValueError("count_summary needs at least one cell")
    return m.on_device()


class _Outputs:
    """Device outputs of one summary: gene sums accumulate over calls, cell outputs are written per call."""

    def __init__(self, n_cells, n_genes, device):
        torch = _torch()
        z = dict(dtype=torch.int64, device=device)
        self.gene_sum = torch.zeros(n_genes, **z)
        self.gene_sumsq = torch.zeros(n_genes, 2, **z)           # (low, high) 64-bit words
        self.gene_zeros = torch.zeros(n_genes, **z)
        self.cell_total = torch.empty(n_cells, **z)
        self.cell_zeros = torch.empty(n_cells, **z)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def enqueue(self, m, lo, accumulate):
        """Summarise the device matrix of view m into the gene outputs and cells [lo, lo + N) (on the current stream)."""
        L = _native.load("stats")
        N = m.N
        ws = m.workspace("stats", "prosstt_amd_stats_workspace_bytes")
        p = _device._ptr
        _native.check(L.prosstt_amd_stats_count_summary(
            m.stream(), p(m.X), N, m.G, m.ld, p(ws), ws.numel(),
            p(self.gene_sum), p(self.gene_sumsq), p(self.gene_zeros), p(self.cell_total[lo:lo + N]),
            p(self.cell_zeros[lo:lo + N]), p(self.status), _native.STATS_ACCUMULATE if accumulate else 0), "stats")

    def fetch(self):
        """Host copies (one synchronising copy of O(cells + genes) numbers); ValueError for a negative entry."""
        torch = _torch()
        flat = torch.cat([self.status.to(torch.int64), self.gene_sum, self.gene_sumsq.reshape(-1), self.gene_zeros,
                          self.cell_total, self.cell_zeros]).cpu().numpy()
        G, N = self.gene_sum.numel(), self.cell_total.numel()
        if flat[0]:
            raise ValueError(_device.NEGATIVE_ENTRY)
        at = 1
        parts = []
        for n in (G, 2 * G, G, N, N):
            parts.append(flat[at:at + n])
            at += n
        gene_sum, sq, gene_zeros, cell_total, cell_zeros = parts
        sq = sq.view(np.uint64).reshape(G, 2)
        sumsq = [(int(hi) << 64) | int(lo) for lo, hi in sq.tolist()]
        return gene_sum, sumsq, gene_zeros, cell_total, cell_zeros


def count_summary(counts):
    """``CountSummary`` of an int32 device count matrix: a (cells, genes) torch tensor with unit column stride (any row
    stride; column slices of a wider tensor are fine), or a ``device.PresentedCounts`` (``draw_counts(out="torch")``),
    whose per-cell arrays then come back in plan order.  Runs on the current stream (the sampler's), so it needs no
    synchronisation after sampling; returns after one copy of O(cells + genes) numbers to the host.

    Raises TypeError for a host array or another dtype, ValueError for a CPU tensor, a non-unit column stride, no cells or
    a negative entry."""
    torch = _torch()
    m = _matrix(counts)
    with torch.cuda.device(m.device):
        out = _Outputs(m.N, m.G, m.device)
        out.enqueue(m, 0, accumulate=False)
        gene_sum, sumsq, gene_zeros, cell_total, cell_zeros = out.fetch()
    return CountSummary(gene_sum, sumsq, gene_zeros, *_device.to_plan_order(m.cell_of_row, cell_total, cell_zeros))


def default_chunk_cells(no_cells, G):
    """Cells per chunk of ``sample_density_summary`` when none is given: about 2 GiB of int32 counts per chunk."""
    return int(max(1, min(no_cells, (2 << 30) // (4 * max(int(G), 1)))))


def sample_density_summary(tree, no_cells, alpha=0.3, beta=2, scale=True, scale_v=0.7, scale_mean=0., *,
                           chunk_cells=None, seed=None, strict=True):
    """``sample_density`` (simulation.py:416-471) summarised on the device: ``(CountSummary, pseudotime, branches,
    scalings)``.  The numpy stream is drawn in ``sample_density``'s order (plan, scalings, seed), so at equal
    ``np.random`` state the plan arrays are ``sample_density``'s and the summary is that of its matrix, for every
    ``chunk_cells``.  The cells are sampled ``chunk_cells`` at a time (default: about 2 GiB of counts per chunk) by
    ``simulation.sample_density_chunks(out="torch")`` and each chunk is summarised as it comes; the matrix never crosses
    PCIe and device memory holds at most two chunks, so 1 M x 30 000 cells fit one GPU."""
    from . import simulation as sim
    torch = _torch()
    if no_cells <= 0:
        raise ValueError("sample_density_summary needs at least one cell")
    if chunk_cells is None:
        chunk_cells = default_chunk_cells(no_cells, tree.G)
    _device.require_gpu()
    dev = torch.cuda.current_device()
    out = _Outputs(no_cells, tree.G, torch.device("cuda", dev))
    perms, pts, brs, scs = [], [], [], []
    lo = 0
    for part, pt, br, sc in sim.sample_density_chunks(tree, no_cells, chunk_cells, alpha, beta, scale, scale_v, scale_mean,
                                                      seed=seed, out="torch", strict=strict):
        m = _matrix(part)
        out.enqueue(m, lo, accumulate=True)
        perms.append(lo + m.cell_of_row)
        pts.append(pt)
        brs.append(br)
        scs.append(sc)
        lo += m.N
    gene_sum, sumsq, gene_zeros, cell_total, cell_zeros = out.fetch()
    total, zeros = _device.to_plan_order(np.concatenate(perms), cell_total, cell_zeros)
    return (CountSummary(gene_sum, sumsq, gene_zeros, total, zeros), np.concatenate(pts), np.concatenate(brs),
            np.concatenate(scs))
