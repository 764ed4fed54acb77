"""
Exact k nearest neighbours of cells, computed on the device: the step between ``embed.pca`` and diffusion maps / UMAP.

Every example notebook of the reference ends with ``pp.neighbors(data, use_rep="X")`` (15, 100, 200 or 700 neighbours) on
the log-normalised matrix.  ``knn`` is that search on a panel of coordinates per cell -- ``PCA.scores`` usually -- in
libprosstt_amd_knn.so (include/prosstt_amd_knn.h): exact, with no seed, and defined to the bit.

    p = embed.pca(X, sc); nb = neighbors.knn(p.scores, 14)       # scanpy's n_neighbors=15 counts the cell itself
    nb.indices, nb.sq_distances, nb.distances, nb.to_csr()

The definition.  P is an N x d panel of binary32 coordinates.  For the pair (i, j)

    d2(i, j) = acc_d,  acc_0 = 0,  acc_{c+1} = fl32(acc_c + fl32(t_c * t_c)),  t_c = fl32(P[i][c] - P[j][c]),  c = 0 .. d-1

a separate binary32 subtract, multiply and add per coordinate in ascending c; nothing is fused, subnormals are kept.
Hence d2(i, j) and d2(j, i) are the same bits.  The neighbours of cell i are the k cells j != i with the smallest key
(bits(d2(i, j)), j), listed in ascending key; ``bits`` is the value's 32-bit pattern read as unsigned (numeric order
for the non-negative finite values in play): ties go to the lower index.  All keys of a row are distinct, so the result
is unique and does not depend on the grid, the chunking or the stream.  The Gram form |a|^2 + |b|^2 - 2 a.b is NOT the
definition: it cancels for exactly the pairs that matter.

There is no CPU fallback: the search runs on the current device, on the current stream.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, device
from .device import _ptr, _torch

MAX_DIM = 128                   # d: the widest panel the kernels take
MAX_NEIGHBORS = 1024            # k
MAX_MAGNITUDE = 2.0 ** 59       # |p| below this: d <= 128 terms below 2^120 each, so no d2 overflows binary32
OUT_CHOICES = "out must be 'numpy' or 'torch'"


class Neighbors(NamedTuple):
    """``indices`` (N, k) int32: the neighbours of every cell in ascending key; ``sq_distances`` (N, k) float32: their
    d2, the bits of the module docstring's definition.  numpy arrays, or device tensors for ``out="torch"``."""
    indices: Any
    sq_distances: Any

    @property
    def distances(self):
        """sqrt(sq_distances), in binary64 (numpy arrays and device tensors alike)."""
        if isinstance(self.sq_distances, np.ndarray):
            return np.sqrt(self.sq_distances.astype(np.float64))
        return self.sq_distances.double().sqrt()

    def to_csr(self):
        """The N x N ``scipy.sparse.csr_matrix`` of distances (binary64): k entries per row, columns ascending within a
        row -- the layout of scikit-learn's ``kneighbors_graph(mode="distance")``.  (A zero distance is a stored
        entry.)"""
        import scipy.sparse as sparse
        idx, dist = self.indices, self.distances
        if not isinstance(idx, np.ndarray):
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        n, k = idx.shape
        order = np.argsort(idx, axis=1, kind="stable")
        out = sparse.csr_matrix((np.take_along_axis(dist, order, axis=1).ravel(),
                                 np.take_along_axis(idx, order, axis=1).ravel(),
                                 np.arange(0, n * k + 1, k, dtype=np.int64)), shape=(n, n))
        out.has_sorted_indices = True
        return out


def _check_sizes(shape, n_neighbors, out, chunk_rows):
    """(N, d, k, chunk_rows for the ABI) of an accepted call, or ValueError; touches no device."""
    if len(shape) != 2:
        raise ValueError("knn needs a (cells, coordinates) panel, not %d dimensions" % len(shape))
    N, d = (int(v) for v in shape)
    if N < 2 or N >= 1 << 31:
        raise ValueError("knn needs 2 <= cells < 2^31 (got %d)" % N)
    if not 1 <= d <= MAX_DIM:
        raise ValueError("knn needs 1 <= coordinates <= %d (got %d)" % (MAX_DIM, d))
    kmax = min(N - 1, MAX_NEIGHBORS)
    k = int(n_neighbors)
    if k != n_neighbors or not 1 <= k <= kmax:
        raise ValueError("need 1 <= n_neighbors <= min(cells - 1, %d) = %d (got %r)" % (MAX_NEIGHBORS, kmax, n_neighbors))
    if out not in ("numpy", "torch"):
        raise ValueError(OUT_CHOICES)
    chunk = 0
    if chunk_rows is not None:
        chunk = int(chunk_rows)
        if chunk != chunk_rows or not 1 <= chunk <= N:
            raise ValueError("need 1 <= chunk_rows <= cells (got %r)" % (chunk_rows,))
    return N, d, k, chunk


NOT_FINITE = "knn needs finite coordinates below 2^59 in magnitude"


def _panel(points, n_neighbors, out, chunk_rows):
    """(f32 device tensor with unit column stride, N, d, ld, k, chunk) of an accepted input.  Everything that can be
    refused without a device is refused before one is used."""
    torch = _torch()
    if isinstance(points, torch.Tensor) and points.device.type != "cpu":
        if points.dtype not in (torch.float32, torch.float64):
            raise TypeError("knn needs float32 or float64 coordinates, not %s" % points.dtype)
        N, d, k, chunk = _check_sizes(tuple(points.shape), n_neighbors, out, chunk_rows)
        P = points.detach()
        if P.dtype != torch.float32:
            P = P.to(torch.float32)                               # rounded once, to nearest
        if (d > 1 and P.stride(1) != 1) or P.stride(0) < d:
            P = P.contiguous()
        with torch.cuda.device(P.device):
            if not bool((P.abs() < MAX_MAGNITUDE).all()):         # (false for a NaN too)
                raise ValueError(NOT_FINITE)
        return P, N, d, P.stride(0), k, chunk
    if isinstance(points, torch.Tensor):
        if not points.dtype.is_floating_point:
            raise TypeError("knn needs floating-point coordinates, not %s" % points.dtype)
        points = points.detach().to(torch.float64 if points.dtype != torch.float32 else torch.float32).numpy()
    host = np.asarray(points)
    if not np.issubdtype(host.dtype, np.floating):
        raise TypeError("knn needs floating-point coordinates, not %s" % host.dtype)
    N, d, k, chunk = _check_sizes(host.shape, n_neighbors, out, chunk_rows)
    if not np.all(np.abs(host) < MAX_MAGNITUDE):
        raise ValueError(NOT_FINITE)
    host = np.ascontiguousarray(host, dtype=np.float32)           # rounded once, to nearest
    device.need_device("knn")
    ld = -(-d // 4) * 4                                           # rows on 16 bytes: the kernels' 16-byte load path
    wide = torch.empty((N, ld), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
    P = wide[:, :d]
    P.copy_(torch.from_numpy(host))
    return P, N, d, ld, k, chunk


def knn(points, n_neighbors=15, *, out="numpy", chunk_rows=None):
    """The ``n_neighbors`` nearest other cells of every cell (the module docstring's definition): ``Neighbors(indices,
    sq_distances)``, (N, k) int32 and float32.

    ``points``: (cells, coordinates), 1 <= coordinates <= 128.  A host array -- ``PCA.scores`` usually -- is rounded to
    binary32 (to nearest) and copied to the current device; a float32 device tensor is read where it lies (any row
    stride and base alignment: column views of a wider tensor are fine); a float64 device tensor is rounded to binary32
    once, to nearest, before the search: distances are those of the ROUNDED coordinates.
    ``n_neighbors`` (k) counts OTHER cells: 1 <= k <= min(cells - 1, 1024).  scanpy's ``n_neighbors`` includes the cell
    itself, so scanpy's default 15 is ``knn(scores, 14)``.
    ``out``: "numpy" (host arrays) or "torch" (device tensors, no host copy).  ``chunk_rows``: query cells per pass
    (None: the library's choice, which keeps a pass's distances in the last-level cache); the result does not depend
    on it.  Runs on the current stream; the workspace is a torch allocation.

    Raises TypeError for a dtype that is not floating; ValueError, before any device use, for a shape that is not 2-D,
    fewer than two cells, coordinates outside 1 .. 128, k out of range or a bad ``out``; ValueError for a non-finite
    coordinate or one with |p| >= 2^59 (below that no squared distance overflows)."""
    torch = _torch()
    P, N, d, ld, k, chunk = _panel(points, n_neighbors, out, chunk_rows)
    L = _native.load("knn")
    with torch.cuda.device(P.device):
        ws = device.workspace("knn", "prosstt_amd_knn_workspace_bytes", P.device, N, d, k, chunk)
        index = torch.empty((N, k), dtype=torch.int32, device=P.device)
        sqdist = torch.empty((N, k), dtype=torch.float32, device=P.device)
        _native.check(L.prosstt_amd_knn_search(device.current_stream(P.device), _ptr(P), N, d, ld, k, chunk, _ptr(index),
                                               _ptr(sqdist), _ptr(ws), ws.numel()), "knn")
        if out == "torch":
            return Neighbors(index, sqdist)
        return Neighbors(index.cpu().numpy(), sqdist.cpu().numpy())
