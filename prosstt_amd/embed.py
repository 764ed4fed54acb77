"""
PCA of the log-normalised count matrix, computed where the matrix lies: on the device.

Every example notebook of the reference embeds the sampled cells the same way after sampling:

    X = (X.transpose() / scalings).transpose()        # each cell divided by its library-size scaling
    data = ad.AnnData(np.log(X + 1))
    pp.neighbors(data, use_rep="X"); diffmap / umap / tsne(data)

At the sizes this package is for, that neighbour search goes through the leading principal components of log1p(X / s)
first (scanpy's default above 50 genes).  ``pca`` computes them without copying the matrix to the host and without
forming log1p(X / s): randomized subspace iteration (Halko, Martinsson and Tropp 2011, Alg. 4.4) whose passes over the
int32 counts run in libprosstt_amd_embed.so (include/prosstt_amd_embed.h); the centring, QR and SVD are binary64
torch, with only l x l factors on the host.

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch"); p = embed.pca(X, sc)
    p.scores                                          # (cells, k) in plan order: the input of neighbours / UMAP

The definition.  A[i, j] = log1p(X[i, j] / s[i]) (natural log), formed on the device in float32 with a relative error
of at most 2^-20 for size factors 2^-94 <= s <= 2^126 (inv_size = fl32(1 / s) in [2^-126, 2^94]; others are refused:
past 2^94 a large count's x * inv_size overflows, or its hardware reciprocal is flushed).  Genes are centred, Ac = A - 1 mu^T with mu = S1 / N, but Ac is never formed: Ac.W = A.W - 1 (mu^T W)
and Ac^T.Q = A^T.Q - mu (1^T Q) are rank-1 corrections in binary64.  With l = min(k + 10, N, G) and
Omega = np.random.default_rng(seed).standard_normal((G, l)):

    Q = qr(Ac.Omega);  n_iter times: P = qr(Ac^T.Q), Q = qr(Ac.P)
    B^T = Ac^T.Q = V S U^T;  components = V^T[:k], singular_values = S[:k], scores = Q.U[:, :k].diag(S[:k])

The products with A take f32 panels (rounded on the way in) and their results are widened to binary64.  Each component
is flipped so that its loading of largest magnitude is positive (the lowest gene on ties), with its scores;
explained_variance = S^2 / (N - 1) and explained_variance_ratio divides it by the total variance
sum_j (S2_j - N mu_j^2) / (N - 1) of the per-gene sums S1, S2 of A and A^2 (binary64), as in scikit-learn and scanpy.

There is no CPU fallback: host arrays are refused.
"""
from typing import NamedTuple

import numpy as np

from . import _native
from . import device as _device
from .device import _torch

MAX_PANEL = 128                 # l: the widest panel the kernels take
OVERSAMPLE = 10                 # l = min(k + OVERSAMPLE, N, G)
MAX_COMPONENTS = MAX_PANEL - OVERSAMPLE
MIN_INV_SIZE = 2.0 ** -126      # inv_size = fl32(1 / s): the smallest normal float32
MAX_INV_SIZE = 2.0 ** 94        # x * inv_size < 2^125 for every int32 count x: v_rcp_f32 of it stays a normal float32


class PCA(NamedTuple):
    """Binary64 numpy arrays, cells in plan order: ``scores`` (N, k), ``components`` (k, G), ``singular_values`` (k,),
    ``explained_variance`` (k,), ``explained_variance_ratio`` (k,), ``gene_mean`` (G,: the mean of log1p(X / s))."""
    scores: np.ndarray
    components: np.ndarray
    singular_values: np.ndarray
    explained_variance: np.ndarray
    explained_variance_ratio: np.ndarray
    gene_mean: np.ndarray


def _counts(counts):
    """The view (device.CountMatrix) of an accepted count input, checked up to (not including) its device."""
    m = _device.CountMatrix(counts, "embed")
    if m.N < 1 or m.G < 1:
        raise ValueError("embed needs at least one cell and one gene (got %d x %d)" % (m.N, m.G))
    if m.N >= 1 << 31:
        raise ValueError("embed takes fewer than 2^31 cells")
    return m


def _inverse_sizes(size_factors, n_cells):
    """fl32(1 / s) of positive, finite host size factors (binary64 division), or raise ValueError.  The kernels' domain
    of inv_size is [2^-126, 2^94] (include/prosstt_amd_embed.h), that is 2^-94 <= s <= 2^126: past 2^94 a large count's
    x * inv overflows to a NaN entry, or the reciprocal in log1p's formula is a denormal that the hardware flushes."""
    torch = _torch()
    if isinstance(size_factors, torch.Tensor):
        size_factors = size_factors.detach().cpu().numpy()
    s = np.asarray(size_factors, dtype=np.float64)
    if s.shape != (n_cells,):
        raise ValueError("need one size factor per cell: shape (%d,), not %s" % (n_cells, s.shape))
    if not np.all(np.isfinite(s)) or not np.all(s > 0):
        raise ValueError("size factors must be positive and finite")
    with np.errstate(over="ignore"):
        inv = (1.0 / s).astype(np.float32)
    if not np.all(np.isfinite(inv)) or not np.all(inv >= MIN_INV_SIZE):
        raise ValueError("size factors must have a normal float32 reciprocal")
    if not np.all(inv <= MAX_INV_SIZE):
        raise ValueError("size factors must be at least 2^-94 (the float32 reciprocal of a size factor may not exceed "
                         "2^94)")
    return inv


class LogNormalized:
    """The operator A = log1p(X / s) over an int32 device count matrix, never formed.

    ``counts``: a (cells, genes) int32 device tensor with unit column stride (any row stride: column slices of a wider
    tensor are fine), or a ``device.PresentedCounts``; ``size_factors``: positive, finite host values, one per cell in
    plan order (the sampler's scalings, or e.g. cell_total / median) with 2^-94 <= s <= 2^126, so that inv_size =
    fl32(1 / s) lies in [2^-126, 2^94].  A ``PresentedCounts`` is read in its row order:
    the operator permutes the size factors and the N x l panels (``index_select``), never the matrix.

    ``.shape``; ``.gene_moments()`` -> (S1, S2) binary64 numpy sums of A and A^2 per gene; ``.matmul(W)``: f32 device
    (G, l) -> f32 device A.W (N, l), cells in plan order; ``.rmatmul(Q)``: f32 device (N, l), cells in plan order -> f32
    device A^T.Q (G, l).  1 <= l <= 128.  Each runs on the current stream; ValueError after a call that met a negative
    count."""

    def __init__(self, counts, size_factors):
        torch = _torch()
        m = _counts(counts)
        N, cell_of_row = m.N, m.cell_of_row
        inv = _inverse_sizes(size_factors, N)
        self.matrix = m.on_device()
        _native.load("embed")
        X = m.X
        self.counts, self.ld, self.device, self.dtype = X, m.ld, X.device, torch.float32
        self._row_of_cell = self._cell_of_row = None
        if cell_of_row is not None:
            inv = inv[cell_of_row]                                    # row i of X is cell cell_of_row[i]
            self._cell_of_row = torch.as_tensor(cell_of_row).to(X.device)
            self._row_of_cell = torch.as_tensor(_device.inverse_permutation(cell_of_row)).to(X.device)
        self.inv_size = torch.as_tensor(inv).to(X.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=X.device)

    @property
    def shape(self):
        return tuple(self.counts.shape)

    def _workspace(self, l):
        return self.matrix.workspace("embed", "prosstt_amd_embed_workspace_bytes", l)

    def _check_status(self):
        if int(self.status.item()):
            raise ValueError(_device.NEGATIVE_ENTRY)

    def _panel(self, P, rows, name):
        torch = _torch()
        if not isinstance(P, torch.Tensor):
            raise TypeError("%s takes a float32 device tensor, not %s" % (name, type(P).__name__))
        if P.dtype != torch.float32:
            raise TypeError("%s needs a float32 panel, not %s" % (name, P.dtype))
        if P.device != self.device:
            raise ValueError("%s needs a panel on %s, not on %s" % (name, self.device, P.device))
        if P.dim() != 2 or P.shape[0] != rows:
            raise ValueError("%s needs a (%d, l) panel, not %s" % (name, rows, tuple(P.shape)))
        l = P.shape[1]
        if not 1 <= l <= MAX_PANEL:
            raise ValueError("%s needs 1 <= l <= %d columns (got %d)" % (name, MAX_PANEL, l))
        return P.contiguous(), l

    def gene_moments(self):
        """(S1, S2): per gene the binary64 sums over cells of A and of A^2."""
        torch = _torch()
        N, G = self.shape
        p = _device._ptr
        with torch.cuda.device(self.device):
            ws = self._workspace(1)
            S = torch.empty(2, G, dtype=torch.float64, device=self.device)
            _native.check(_native.load("embed").prosstt_amd_embed_gene_moments(
                self.matrix.stream(), p(self.counts), N, G, self.ld, p(self.inv_size), p(ws), ws.numel(), p(S[0]),
                p(S[1]), p(self.status)), "embed")
            self._check_status()
            S = S.cpu().numpy()
        return S[0].copy(), S[1].copy()

    def matmul(self, W):
        """A.W: f32 device (G, l) -> f32 device (N, l), cells in plan order."""
        torch = _torch()
        N, G = self.shape
        W, l = self._panel(W, G, "matmul")
        p = _device._ptr
        with torch.cuda.device(self.device):
            ws = self._workspace(l)
            Y = torch.empty(N, l, dtype=torch.float32, device=self.device)
            _native.check(_native.load("embed").prosstt_amd_embed_matmul(
                self.matrix.stream(), p(self.counts), N, G, self.ld, p(self.inv_size), p(W), l, p(Y), p(ws),
                ws.numel(), p(self.status)), "embed")
            self._check_status()
            if self._row_of_cell is not None:
                Y = Y.index_select(0, self._row_of_cell)
        return Y

    def rmatmul(self, Q):
        """A^T.Q: f32 device (N, l), cells in plan order -> f32 device (G, l)."""
        torch = _torch()
        N, G = self.shape
        Q, l = self._panel(Q, N, "rmatmul")
        p = _device._ptr
        with torch.cuda.device(self.device):
            if self._cell_of_row is not None:
                Q = Q.index_select(0, self._cell_of_row)
            ws = self._workspace(l)
            Z = torch.empty(G, l, dtype=torch.float32, device=self.device)
            _native.check(_native.load("embed").prosstt_amd_embed_rmatmul(
                self.matrix.stream(), p(self.counts), N, G, self.ld, p(self.inv_size), p(Q), l, p(Z), p(ws),
                ws.numel(), p(self.status)), "embed")
            self._check_status()
        return Z


def _check_components(N, G, n_components, n_iter):
    k = int(n_components)
    if k != n_components or not 1 <= k <= min(N, G, MAX_COMPONENTS):
        raise ValueError("need 1 <= n_components <= min(cells, genes, %d) = %d (got %r)"
                         % (MAX_COMPONENTS, min(N, G, MAX_COMPONENTS), n_components))
    if int(n_iter) != n_iter or n_iter < 0:
        raise ValueError("n_iter must be a non-negative integer (got %r)" % (n_iter,))
    if N < 2:
        raise ValueError("a PCA needs at least two cells")
    return k, int(n_iter)


def _gram(Y):
    """Y^T Y of a tall (n, l) binary64 tensor, as a sum of row-block products (one wide batched product rather than one
    long reduction, which the BLAS runs on a handful of tiles)."""
    torch = _torch()
    n, l = Y.shape
    c = max(1, min(256, n // 256))
    b = -(-n // c)
    if c * b != n:
        Y = torch.cat([Y, Y.new_zeros(c * b - n, l)])
    Yb = Y.reshape(c, b, l)
    return torch.bmm(Yb.transpose(1, 2), Yb).sum(dim=0)


def _qr(Y):
    """(Q, R) of a tall binary64 tensor by shifted CholeskyQR3 (Fukaya, Kannan, Nakatsukasa, Yamamoto and Yanagisawa
    2020): three rounds of Y <- Y R^-1 with R the Cholesky factor of the Gram matrix, the first shifted so that it
    succeeds for any condition number.  The products stay on Y's device; only l x l matrices visit the host.  A zero or
    non-finite Y goes to torch.linalg.qr (Householder)."""
    torch = _torch()
    n, l = Y.shape
    R = np.eye(l)
    try:
        for shifted in (True, False, False):
            G = _gram(Y).cpu().numpy()
            G = (G + G.T) / 2
            if shifted:
                norm2 = float(np.trace(G))
                if not norm2 > 0 or not np.isfinite(norm2):
                    raise np.linalg.LinAlgError("zero or non-finite panel")
                G[np.diag_indices(l)] += 11 * (n * l + l * (l + 1)) * np.finfo(np.float64).eps * norm2
            Ri = np.linalg.cholesky(G).T                          # upper triangular, G = Ri^T Ri
            Y = Y @ torch.as_tensor(np.linalg.inv(Ri), dtype=Y.dtype, device=Y.device)
            R = Ri @ R
    except np.linalg.LinAlgError:
        Q, Rt = torch.linalg.qr(Y)
        return Q, Rt.cpu().numpy() @ R
    return Y, R


def _randomized_pca(op, S1, S2, n_components, n_iter, seed):
    """The driver of the module docstring's definition after the moments, over any operator with ``shape``, ``dtype``
    and ``device`` (its panels' torch dtype and device), ``matmul`` and ``rmatmul``; ``S1``, ``S2``: its per-gene sums of
    A and A^2 (binary64 numpy)."""
    torch = _torch()
    f64 = torch.float64
    N, G = op.shape
    k = n_components
    l = min(k + OVERSAMPLE, N, G)
    S1 = np.asarray(S1, dtype=np.float64)
    S2 = np.asarray(S2, dtype=np.float64)
    mean = S1 / N
    mu = torch.as_tensor(mean, dtype=f64, device=op.device)

    def centred(P):                       # Ac.P = A.P - 1 (mu^T P), P (G, l) binary64 -> (N, l)
        Pr = P.to(op.dtype)
        Pw = Pr.to(f64)
        return op.matmul(Pr).to(f64) - (Pw * mu[:, None]).sum(dim=0)[None, :]   # (mu @ Pw: a one-tile GEMM, 2 ms)

    def centred_t(Q):                     # Ac^T.Q = A^T.Q - mu (1^T Q), Q (N, l) binary64 -> (G, l)
        Qr = Q.to(op.dtype)
        Qw = Qr.to(f64)
        return op.rmatmul(Qr).to(f64) - mu[:, None] * Qw.sum(dim=0)[None, :]

    omega = np.random.default_rng(seed).standard_normal((G, l))
    Q = _qr(centred(torch.as_tensor(omega, dtype=f64, device=op.device)))[0]
    for _ in range(n_iter):
        P = _qr(centred_t(Q))[0]
        Q = _qr(centred(P))[0]
    Bt = centred_t(Q)                     # (G, l) = V S U^T
    Q2, R = _qr(Bt)                       # Bt = Q2 R; R (l x l) = Ur S Vh on the host: V = Q2 Ur, U = Vh^T
    Ur, S, Vh = np.linalg.svd(R)
    components = (Q2 @ torch.as_tensor(Ur[:, :k], dtype=f64, device=op.device)).T.cpu().numpy()
    scores = (Q @ torch.as_tensor(Vh[:k].T * S[:k], dtype=f64, device=op.device)).cpu().numpy()
    top = np.argmax(np.abs(components), axis=1)                # the first gene on ties
    signs = np.where(components[np.arange(k), top] < 0, -1.0, 1.0)
    components *= signs[:, None]
    scores *= signs[None, :]
    sv = S[:k].copy()
    explained = sv * sv / (N - 1)
    total = np.sum(S2 - N * mean * mean) / (N - 1)
    return PCA(np.ascontiguousarray(scores), np.ascontiguousarray(components), sv, explained, explained / total, mean)


def pca(counts, size_factors, n_components=50, *, n_iter=7, seed=0):
    """Principal components of log1p(X / s), genes centred (the module docstring's definition): a ``PCA`` of binary64
    numpy arrays, cells in plan order.

    ``counts``: an int32 device tensor (cells, genes) with unit column stride, or a ``device.PresentedCounts``
    (``sample_density(out="torch")``); ``size_factors``: one positive, finite value per cell in plan order (the sampler's
    scalings).  ``n_components`` (k, scanpy's n_comps): 1 <= k <= min(cells, genes, 118); ``n_iter``: subspace
    iterations (scikit-learn's 'auto' for k < 0.1 min(cells, genes)); ``seed``: of the Gaussian test matrix.  The
    matrix is read 2 n_iter + 3 times and never leaves the device; runs on the current stream.

    Raises TypeError for a host array or another dtype, ValueError for a CPU tensor, bad size factors, k or n_iter out of
    range, fewer than two cells, or a negative count."""
    torch = _torch()
    m = _counts(counts)
    k, n_iter = _check_components(m.N, m.G, n_components, n_iter)
    op = LogNormalized(counts, size_factors)
    with torch.cuda.device(op.device):
        S1, S2 = op.gene_moments()
        return _randomized_pca(op, S1, S2, k, n_iter, seed)
