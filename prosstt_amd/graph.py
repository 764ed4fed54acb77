"""
Fuzzy connectivities of the kNN graph of cells and its diffusion map, computed on the device: the step after
``neighbors.knn`` (scanpy's ``pp.neighbors`` connectivities and ``tl.diffmap``, where the reference's notebooks end).

    p = embed.pca(X, sc); nb = neighbors.knn(p.scores, 14, out="torch")
    dm = graph.diffmap(nb)                       # dm.eigenvalues (15,), dm.eigenvectors (N, 15): obsm["X_diffmap"]
    g = graph.connectivities(nb); g.to_csr()     # obsp["connectivities"]

Everything runs in libprosstt_amd_graph.so (include/prosstt_amd_graph.h) and in torch's device plumbing (a sort, prefix
sums, the dense products of the Lanczos basis); there is no CPU fallback.

The definition (all binary64).  The input is ``Neighbors(indices, sq_distances)``: N rows of k other cells,
d_ij = sqrt(float64(sq_distances)); 3 <= N < 2^31, 2 <= k <= min(N - 1, 1024); every index in [0, N) and not its row,
every d^2 finite and >= 0.

  Memberships (directed, N x k).  For row i: rho_i = min{d_ij : d_ij > 0} (0 if there is none), g_ij = max(d_ij - rho_i,
  0), f(s) = sum_j exp(-g_ij / s), target = log2(k + 1), and sigma_i from exactly this bisection, 64 steps, no early exit:

      lo = 0; hi = inf; mid = 1
      repeat 64 times:
          if f(mid) > target:  hi = mid;  mid = (lo + hi) / 2
          else:                lo = mid;  mid = (hi == inf) ? 2 mid : (lo + hi) / 2
      sigma_i = max(mid, 1e-3 * mean_j d_ij)

  a_ij = 1 where g_ij = 0, exp(-g_ij / sigma_i) otherwise.  This is umap-learn's ``smooth_knn_dist`` as scanpy calls it
  (local_connectivity 1, the self column skipped, k + 1 = scanpy's n_neighbors) with two deliberate differences: the root
  is found to full precision instead of umap's 1e-5 early exit, so sigma is a continuous function of the row; and the
  floor uses the row's own mean also when rho = 0.  (The correspondence is from reading umap-learn, not from a run.)

  Connectivities.  W = A + A^T - A o A^T, A the N x N matrix of the a_ij, computed as (a + b) - a b: symmetric to the
  bit.  CSR with int64 indptr, int32 indices ascending within a row, binary64 data; every stored pair once per direction,
  no diagonal, no explicit zeros beyond what a itself yields.  Rows have between k and N - 1 entries.

  Operator (scanpy's ``_compute_transitions`` with density_normalize=True).  q = W 1, K_ij = W_ij / (q_i q_j),
  z_i = sqrt((K 1)_i), T_ij = K_ij / (z_i z_j): symmetric, the sparsity of W; on a connected graph T z = z, so the first
  eigenvalue is 1 with eigenvector z / |z|.

  Diffusion map.  The n_comps eigenvalues of T of largest magnitude, listed by descending value, with unit eigenvectors
  (N x n_comps); each eigenvector's entry of largest magnitude (the lowest index among equals) is positive.  Like scanpy,
  component 0, the trivial one, is kept.

The solver is plain Lanczos with full reorthogonalisation (two passes of classical Gram-Schmidt against the whole basis)
and no restart, in binary64 on the device; w = T v is the library's kernel.  Every 16 steps the tridiagonal matrix goes to
the host, and the run stops when the residual estimate |beta_m s_mi| of each of the n_comps Ritz pairs of largest
magnitude is below ``tol``.  A disconnected graph has a repeated eigenvalue 1; a single-vector Lanczos run, like scanpy's
ARPACK call, may not return every copy.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, device
from .device import _ptr, _torch
from .neighbors import MAX_NEIGHBORS

CHECK_EVERY = 16                # Lanczos steps between two looks at the Ritz values
MAX_STEPS = 2048
LANES = (0, 4, 16, 64)          # lanes per row of the product kernel; 0: the library's choice
BAD_INDEX, BAD_SELF, BAD_DISTANCE, BAD_DEGREE = 1, 2, 4, 8          # bits of the status word (prosstt_amd_graph.h)


class NotConverged(RuntimeError):
    """The Lanczos run ended (``max_steps``, or a breakdown) before every residual estimate was below ``tol``.
    ``residuals``: the estimates of the n_comps Ritz pairs at the end (empty if there were fewer than n_comps steps);
    ``steps``: the steps taken."""

    def __init__(self, message, residuals, steps):
        super().__init__(message)
        self.residuals = residuals
        self.steps = steps


def _csr(indptr, indices, data):
    import scipy.sparse as sparse
    if not isinstance(indptr, np.ndarray):
        indptr, indices, data = (t.cpu().numpy() for t in (indptr, indices, data))
    n = indptr.shape[0] - 1
    out = sparse.csr_matrix((data, indices, indptr), shape=(n, n))
    out.has_sorted_indices = True
    return out


class Connectivities(NamedTuple):
    """W in CSR (``indptr`` int64 (N + 1,), ``indices`` int32, ``data`` float64) and the ``rho`` and ``sigma`` (N,) of
    the memberships.  numpy arrays, or device tensors for ``out="torch"``."""
    indptr: Any
    indices: Any
    data: Any
    rho: Any
    sigma: Any

    def to_csr(self):
        """W as an N x N ``scipy.sparse.csr_matrix`` (copied to the host if it lies on the device)."""
        return _csr(self.indptr, self.indices, self.data)


class Transitions(NamedTuple):
    """T in CSR (the ``indptr`` and ``indices`` of W, ``data`` float64) and the ``q`` and ``z`` (N,) of the operator's
    definition, as device tensors."""
    indptr: Any
    indices: Any
    data: Any
    q: Any
    z: Any

    def to_csr(self):
        return _csr(self.indptr, self.indices, self.data)


class DiffusionMap(NamedTuple):
    """``eigenvalues`` (n_comps,) descending, ``eigenvectors`` (N, n_comps), ``steps`` (Lanczos steps taken),
    ``residuals`` (n_comps,) the estimates |beta_m s_mi| the run stopped on (a host array), ``transitions``: T as a
    scipy CSR matrix (``out="numpy"``) or a ``Transitions`` of device tensors (``out="torch"``)."""
    eigenvalues: Any
    eigenvectors: Any
    steps: int
    residuals: Any
    transitions: Any


# ------------------------------------------------------------------------------------------------- argument checks

def _check_neighbors(nb):
    """(indices, sq_distances, N, k) of an accepted ``Neighbors``: host arrays or device tensors as they came, the
    shapes and dtypes checked; ValueError otherwise.  Touches no device."""
    torch = _torch()
    try:
        idx, d2 = nb
    except (TypeError, ValueError):
        raise ValueError("need a Neighbors(indices, sq_distances) pair") from None
    pair = []
    for name, arr, np_dtype, t_dtype in (("indices", idx, np.int32, torch.int32), ("sq_distances", d2, np.float32, torch.float32)):
        if isinstance(arr, torch.Tensor):
            if arr.dtype != t_dtype:
                raise ValueError("%s must be %s, not %s" % (name, np.dtype(np_dtype).name, arr.dtype))
            if arr.device.type == "cpu":
                arr = arr.detach().numpy()
        else:
            arr = np.asarray(arr)
            if arr.dtype != np_dtype:
                raise ValueError("%s must be %s, not %s" % (name, np.dtype(np_dtype).name, arr.dtype))
        if len(arr.shape) != 2:
            raise ValueError("%s must be (cells, neighbours), not %d dimensions" % (name, len(arr.shape)))
        pair.append(arr)
    idx, d2 = pair
    if tuple(idx.shape) != tuple(d2.shape):
        raise ValueError("indices %s and sq_distances %s differ in shape" % (tuple(idx.shape), tuple(d2.shape)))
    if isinstance(idx, np.ndarray) != isinstance(d2, np.ndarray) or (not isinstance(idx, np.ndarray) and idx.device != d2.device):
        raise ValueError("indices and sq_distances must lie in the same place")
    N, k = (int(v) for v in idx.shape)
    if N < 3 or N >= 1 << 31:
        raise ValueError("need 3 <= cells < 2^31 (got %d)" % N)
    kmax = min(N - 1, MAX_NEIGHBORS)
    if not 2 <= k <= kmax:
        raise ValueError("need 2 <= neighbours <= min(cells - 1, %d) = %d (got %d)" % (MAX_NEIGHBORS, kmax, k))
    return idx, d2, N, k


def _check_csr_shapes(g):
    """N of a ``Connectivities`` whose arrays have the dtypes and shapes of one; ValueError otherwise.  No device."""
    torch = _torch()
    names = (("indptr", np.int64, torch.int64), ("indices", np.int32, torch.int32), ("data", np.float64, torch.float64))
    for name, np_dtype, t_dtype in names:
        arr = getattr(g, name)
        want = t_dtype if isinstance(arr, torch.Tensor) else np.dtype(np_dtype)
        if not isinstance(arr, (torch.Tensor, np.ndarray)) or arr.dtype != want or len(arr.shape) != 1:
            raise ValueError("%s must be a 1-D %s array" % (name, np.dtype(np_dtype).name))
    N = int(g.indptr.shape[0]) - 1
    if N < 3 or N >= 1 << 31:
        raise ValueError("need 3 <= cells < 2^31 (got %d)" % N)
    if int(g.indices.shape[0]) != int(g.data.shape[0]):
        raise ValueError("indices and data differ in length")
    return N


def _check_diffmap(N, n_comps, tol, seed, max_steps, out):
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    if int(n_comps) != n_comps or not 1 <= n_comps < N:
        raise ValueError("need 1 <= n_comps < cells = %d (got %r)" % (N, n_comps))
    if not (isinstance(tol, (int, float)) and 0 < tol < float("inf")):
        raise ValueError("tol must be a positive finite number (got %r)" % (tol,))
    if int(seed) != seed or seed < 0:
        raise ValueError("seed must be a non-negative integer (got %r)" % (seed,))
    limit = min(N, MAX_STEPS)
    if max_steps is not None:
        if int(max_steps) != max_steps or max_steps < n_comps:
            raise ValueError("need max_steps >= n_comps (got %r)" % (max_steps,))
        limit = min(limit, int(max_steps))
    return int(n_comps), limit


def _on_device(arr, dev=None):
    torch = _torch()
    if isinstance(arr, np.ndarray):
        host = np.ascontiguousarray(arr)
        if not host.flags.writeable:                  # torch wants an owned buffer
            host = host.copy()
        return torch.from_numpy(host).to(dev or torch.device("cuda", torch.cuda.current_device()))
    return arr.detach().contiguous()


BAD_VALUES = ((BAD_INDEX, "a neighbour index lies outside [0, cells)"), (BAD_SELF, "a cell is listed as its own neighbour"),
              (BAD_DISTANCE, "a squared distance is negative, infinite or NaN"),
              (BAD_DEGREE, "a row of the connectivities does not sum to a positive finite number"))


def _raise_status(status):
    bits = int(status.item())
    if bits:
        raise ValueError("; ".join(text for bit, text in BAD_VALUES if bits & bit))


# ------------------------------------------------------------------------------------------------------ connectivities

def _sorted_runs(keys):
    """(sorted_keys, perm, pos, nnz) of the int64 device vector ``keys``, what a fold entry point reads: torch's stable
    sort, ``pos`` the prefix sum of the heads of the runs of equal keys and ``nnz`` the number of runs (one host read)."""
    sorted_keys, perm = _torch().sort(keys, stable=True)
    head = _torch().ones_like(sorted_keys)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]                      # 1 where a run of equal keys begins
    pos = _torch().cumsum(head, 0)
    return sorted_keys, perm, pos, int(pos[-1].item())


def _symmetrize(L, idx, a, N, k, fold, fold_library):
    """(indptr, indices, data) of the symmetrisation of the directed values ``a`` (N, k) float64 on the entries ``idx``:
    the graph library's keyed emit, torch's sort and prefix sum, and ``fold``, an entry of library ``fold_library`` with
    the arguments of prosstt_amd_graph_symmetrize_fold, which says how the two directions of a pair combine."""
    torch = _torch()
    dev = idx.device
    st = device.current_stream(dev)
    ws = device.workspace("graph", "prosstt_amd_graph_workspace_bytes", dev, N, k)
    _native.check(L.prosstt_amd_graph_symmetrize_emit(st, _ptr(idx), _ptr(a), N, k, _ptr(ws), ws.numel()), "graph")
    sorted_keys, perm, pos, nnz = _sorted_runs(ws[:8 * 2 * N * k].view(torch.int64))
    indptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    indices = torch.empty(nnz, dtype=torch.int32, device=dev)
    data = torch.empty(nnz, dtype=torch.float64, device=dev)
    _native.check(fold(st, _ptr(sorted_keys), _ptr(perm), _ptr(pos), N, k, nnz, _ptr(ws), ws.numel(), _ptr(indptr),
                       _ptr(indices), _ptr(data)), fold_library)
    return indptr, indices, data


def _connectivities(L, idx, d2, N, k):
    """Connectivities of device tensors from contiguous device ``idx`` (N, k) int32 and ``d2`` float32."""
    torch = _torch()
    dev = idx.device
    st = device.current_stream(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = torch.empty((N, k), dtype=torch.float64, device=dev)
    rho = torch.empty(N, dtype=torch.float64, device=dev)
    sigma = torch.empty(N, dtype=torch.float64, device=dev)
    _native.check(L.prosstt_amd_graph_memberships(st, _ptr(idx), _ptr(d2), N, k, _ptr(a), _ptr(rho), _ptr(sigma),
                                                  _ptr(status)), "graph")
    _raise_status(status)
    indptr, indices, data = _symmetrize(L, idx, a, N, k, L.prosstt_amd_graph_symmetrize_fold, "graph")
    return Connectivities(indptr, indices, data, rho, sigma)


def connectivities(nb, *, out="scipy"):
    """The fuzzy connectivities W of the kNN graph ``nb`` (the module docstring's definition):
    ``Connectivities(indptr, indices, data, rho, sigma)``; ``.to_csr()`` is the scipy matrix.

    ``nb``: a ``neighbors.Neighbors`` (or any pair) of int32 indices and float32 squared distances, (cells, k) each, as
    numpy arrays (copied to the current device) or as device tensors (used where they lie, on the current stream).
    ``out``: "scipy" (host arrays) or "torch" (device tensors, no host copy).

    Raises ValueError, before any device use, for wrong dtypes or shapes, fewer than 3 cells, k outside 2 .. min(cells
    - 1, 1024) or a bad ``out``; ValueError, from the device's check, for an index outside [0, cells) or equal to its
    row and for a squared distance that is negative or not finite."""
    if out not in ("scipy", "torch"):
        raise ValueError("out must be 'scipy' or 'torch'")
    idx, d2, N, k = _check_neighbors(nb)
    L = device.need_device("graph")
    torch = _torch()
    idx = _on_device(idx)
    d2 = _on_device(d2, idx.device)
    with torch.cuda.device(idx.device):
        g = _connectivities(L, idx, d2, N, k)
        if out == "torch":
            return g
        return Connectivities(*(t.cpu().numpy() for t in g))


def _as_connectivities(L, graph):
    """A ``Connectivities`` of device tensors from what ``transitions`` and ``diffmap`` accept (already checked on the
    host); a caller's CSR arrays are checked here, since the kernels that read them trust them."""
    torch = _torch()
    if not isinstance(graph, Connectivities):
        idx, d2, N, k = _check_neighbors(graph)
        idx = _on_device(idx)
        d2 = _on_device(d2, idx.device)
        with torch.cuda.device(idx.device):
            return _connectivities(L, idx, d2, N, k)
    indptr = _on_device(graph.indptr)
    indices, data = _on_device(graph.indices, indptr.device), _on_device(graph.data, indptr.device)
    with torch.cuda.device(indptr.device):
        nnz = indices.numel()
        ok = (indptr[0] == 0) & (indptr[-1] == nnz) & (indptr[1:] >= indptr[:-1]).all()
        if nnz:
            ok = ok & (indices >= 0).all() & (indices < indptr.numel() - 1).all()
        if not bool(ok):
            raise ValueError("indptr and indices are not those of a CSR matrix of cells x cells")
    return Connectivities(indptr, indices, data, graph.rho, graph.sigma)


def _host_checks(graph):
    """N of a ``Neighbors`` or ``Connectivities``, refused on the host where it can be."""
    if isinstance(graph, Connectivities):
        return _check_csr_shapes(graph)
    return _check_neighbors(graph)[2]


def _transitions(L, g):
    torch = _torch()
    dev = g.indptr.device
    N, nnz = g.indptr.numel() - 1, g.indices.numel()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    T = torch.empty(nnz, dtype=torch.float64, device=dev)
    q = torch.empty(N, dtype=torch.float64, device=dev)
    z = torch.empty(N, dtype=torch.float64, device=dev)
    _native.check(L.prosstt_amd_graph_normalize(device.current_stream(dev), _ptr(g.indptr), _ptr(g.indices), _ptr(g.data), N,
                                                nnz, _ptr(T), _ptr(q), _ptr(z), _ptr(status)), "graph")
    _raise_status(status)
    return Transitions(g.indptr, g.indices, T, q, z)


def transitions(graph):
    """The density-normalised transition matrix T of a ``Neighbors`` or a ``Connectivities`` (the module docstring's
    operator), as a ``Transitions`` of device tensors."""
    _host_checks(graph)
    L = device.need_device("graph")
    g = _as_connectivities(L, graph)
    with _torch().cuda.device(g.indptr.device):
        return _transitions(L, g)


def spmv(T, x, lanes_per_row=0):
    """y = T x on the device: ``T`` a ``Transitions`` (or any CSR triple of device tensors that ``transitions`` or
    ``connectivities`` returned), ``x`` a float64 device vector.  ``lanes_per_row``: 4, 16 or 64 lanes own a row; 0 lets
    the library choose from the mean row length.  Equal inputs give equal bits for a given ``lanes_per_row``."""
    torch = _torch()
    if lanes_per_row not in LANES:
        raise ValueError("lanes_per_row must be 0, 4, 16 or 64 (got %r)" % (lanes_per_row,))
    L = device.need_device("graph")
    N = T.indptr.numel() - 1
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or tuple(x.shape) != (N,) or x.device != T.data.device:
        raise ValueError("x must be a float64 vector of %d entries on %s" % (N, T.data.device))
    x = x.contiguous()
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _native.check(L.prosstt_amd_graph_spmv(device.current_stream(x.device), _ptr(T.indptr), _ptr(T.indices), _ptr(T.data),
                                               N, T.indices.numel(), _ptr(x), _ptr(y), lanes_per_row), "graph")
    return y


# -------------------------------------------------------------------------------------------------------- diffusion map

def _ritz(alpha, beta, m, n_comps):
    """(values descending, S (m, n_comps), residual estimates) of the n_comps Ritz pairs of largest magnitude of the
    m-step tridiagonal matrix."""
    tri = np.diag(alpha[:m]) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
    theta, S = np.linalg.eigh(tri)
    pick = np.argsort(-np.abs(theta), kind="stable")[:n_comps]
    pick = pick[np.argsort(-theta[pick], kind="stable")]
    return theta[pick], S[:, pick], np.abs(beta[m - 1] * S[m - 1, pick])


def _lanczos(L, T, n_comps, tol, seed, limit):
    """(eigenvalues (host), eigenvectors (device, N x n_comps), steps, residual estimates (host)) of T."""
    torch = _torch()
    dev = T.data.device
    N, nnz = T.indptr.numel() - 1, T.indices.numel()
    st = device.current_stream(dev)
    start = np.random.default_rng(seed).standard_normal(N)
    start /= np.linalg.norm(start)
    rows = min(limit, 4 * CHECK_EVERY) + 1
    V = torch.empty((rows, N), dtype=torch.float64, device=dev)          # the basis, a vector per row
    V[0].copy_(torch.from_numpy(start))
    alpha = torch.zeros(limit, dtype=torch.float64, device=dev)
    beta = torch.zeros(limit, dtype=torch.float64, device=dev)
    w = torch.empty(N, dtype=torch.float64, device=dev)
    breakdown = N * 2.0 ** -52
    residuals = np.empty(0)
    for j in range(limit):
        if j + 1 >= V.shape[0]:
            V = torch.cat([V, torch.empty((min(V.shape[0], limit + 1 - V.shape[0]), N), dtype=torch.float64, device=dev)])
        _native.check(L.prosstt_amd_graph_spmv(st, _ptr(T.indptr), _ptr(T.indices), _ptr(T.data), N, nnz, _ptr(V[j]),
                                               _ptr(w), 0), "graph")
        alpha[j].copy_(torch.dot(w, V[j]))
        basis = V[:j + 1]
        for _ in range(2):
            w.addmv_(basis.t(), torch.mv(basis, w), alpha=-1.0)
        beta[j].copy_(torch.linalg.vector_norm(w))
        torch.div(w, beta[j], out=V[j + 1])
        m = j + 1
        if not ((m % CHECK_EVERY == 0 and m >= n_comps) or m == limit):
            continue
        a, b = alpha[:m].cpu().numpy(), beta[:m].cpu().numpy()
        small = np.flatnonzero(~(b >= breakdown))                        # (a NaN counts)
        broke = small.size > 0
        if broke:
            m = int(small[0]) + 1                                        # the Krylov space ended here
        if m >= n_comps:
            theta, S, residuals = _ritz(a, b, m, n_comps)
            if np.all(residuals < tol):
                vectors = torch.mm(V[:m].t(), torch.from_numpy(np.ascontiguousarray(S)).to(dev))
                return theta, vectors, m, residuals
        if broke:
            raise NotConverged("the Lanczos run broke down at step %d (beta below cells * 2^-52) before %d components "
                               "converged" % (m, n_comps), residuals, m)
    raise NotConverged("no convergence to tol = %g in %d Lanczos steps (largest residual estimate %.3g)"
                       % (tol, limit, residuals.max() if residuals.size else float("nan")), residuals, limit)


def _fix_signs(vectors):
    """Unit columns whose entry of largest magnitude (the lowest index among equals) is positive."""
    torch = _torch()
    vectors = vectors / torch.linalg.vector_norm(vectors, dim=0, keepdim=True)
    mag = vectors.abs()
    rows = torch.arange(vectors.shape[0], device=vectors.device)[:, None]
    first = torch.where(mag == mag.amax(dim=0, keepdim=True), rows, vectors.shape[0]).amin(dim=0)
    sign = torch.where(vectors.gather(0, first[None, :]) < 0, -1.0, 1.0)
    return vectors * sign


def diffmap(graph, n_comps=15, *, tol=1e-10, seed=0, max_steps=None, out="numpy"):
    """The diffusion map of a kNN graph (the module docstring's definition): ``DiffusionMap(eigenvalues, eigenvectors,
    steps, residuals, transitions)``.

    ``graph``: a ``neighbors.Neighbors`` (numpy arrays or device tensors, as ``connectivities`` takes them) or a
    ``Connectivities``.  ``n_comps``: 1 <= n_comps < cells.  ``tol``: the bound on every residual estimate.  ``seed``:
    of the start vector ``numpy.random.default_rng(seed).standard_normal(cells)``; equal calls give equal bits.
    ``max_steps``: Lanczos steps allowed (None: min(cells, 2048), the most there are).  ``out``: "numpy" (host arrays,
    ``transitions`` a scipy CSR matrix) or "torch" (device tensors, ``transitions`` a ``Transitions``).

    Raises ValueError for what ``connectivities`` refuses and for a bad n_comps, tol, seed, max_steps or out (before any
    device use where the input allows); ``NotConverged`` when ``max_steps`` are taken, or the run breaks down, before
    every estimate is below ``tol``."""
    N = _host_checks(graph)
    n_comps, limit = _check_diffmap(N, n_comps, tol, seed, max_steps, out)
    L = device.need_device("graph")
    torch = _torch()
    g = _as_connectivities(L, graph)
    with torch.cuda.device(g.indptr.device):
        T = _transitions(L, g)
        values, vectors, steps, residuals = _lanczos(L, T, n_comps, float(tol), int(seed), limit)
        vectors = _fix_signs(vectors)
        if out == "torch":
            return DiffusionMap(torch.from_numpy(values).to(vectors.device), vectors, steps, residuals, T)
        return DiffusionMap(values, vectors.cpu().numpy(), steps, residuals, T.to_csr())
