"""
Exact t-SNE layouts of the cells, computed on the device: the picture the reference's notebooks draw their branch
assignments on (scanpy's ``tl.tsne``, ``obsm["X_tsne"]``).

    p = embed.pca(X, sc)
    res = tsne.tsne(p.scores)                    # res.embedding (N, 2) float32: obsm["X_tsne"]; res.kl_divergence
    aff = tsne.affinities(neighbors.knn(p.scores, 90, out="torch"), 30.0, out="torch"); aff.to_csr()
    res = tsne.tsne(aff, 3, init="random", seed=7)

Everything runs in libprosstt_amd_tsne.so (include/prosstt_amd_tsne.h), with libprosstt_amd_graph.so's keyed emit and torch's
sort for the transpose; torch is the device plumbing.  There is no CPU fallback.  The repulsion is evaluated over all N^2
pairs in a fixed order, not approximated (Barnes-Hut) as the CPU libraries do: equal calls give equal bits.

The definition.  Affinities are binary64.  Positions, gradient, update and gains are binary32.  The normaliser Z and the
sums across tiles and slabs are binary64.

  Conditional affinities (N x k).  The input is ``Neighbors(indices, sq_distances)``, d2 = float64(sq_distances); 3 <= N <
  2^31, 2 <= k <= min(N - 1, 1024), 1 < perplexity < k; every index in [0, N) and not its row, every d2 finite and >= 0.
  For row i: g_j = d2_j - min_j d2_j, target = log(perplexity); for a given beta, p_j = exp(-beta g_j), S = sum p_j, H(beta)
  = log S + beta (sum g_j p_j) / S; beta_i from exactly this bisection, 64 steps, no early exit:

      lo = 0; hi = inf; beta = 1
      repeat 64 times:
          if H(beta) > target:  lo = beta;  beta = (hi == inf) ? 2 beta : (lo + hi) / 2
          else:                 hi = beta;  beta = (lo + hi) / 2

  and p_{j|i} = p_j / S.  This is scikit-learn's ``_binary_search_perplexity`` with the root found to full precision
  instead of its 1e-5 early exit, and with the shift by the row minimum (which cancels in p_j / S).  A row whose distances
  are all equal ends with beta = 2^64 and p = 1 / k exactly.

  Joint affinities.  P = (A + A^T) / (2 N), A the N x N matrix of the p_{j|i}, in CSR as ``graph.Connectivities`` holds W
  (int64 indptr, int32 indices ascending within a row, binary64 data, no diagonal).  Each value is (a + b) / (2 N), one IEEE
  addition and one IEEE division: P is symmetric to the bit.

  Gradient at positions Y (N x c, c = 2 or 3) and exaggeration x (binary32).  For a pair: delta = y_i - y_j, d2 = delta_0
  delta_0 then fmaf(delta_c, delta_c, d2), w = 1 + d2, q = the hardware reciprocal of w (within 1 ulp).
    - Repulsion over ALL pairs, j = i included (the self term adds exactly 1 and 0): z_i = sum_j q, R_i = sum_j (q q) delta.
      Columns are cut into tiles of ``TILE``; within a tile the sums are binary32 chains in ascending column order, across
      tiles binary64; the tiles are dealt to ``slabs`` runs of whole tiles whose binary64 partial sums are added in
      ascending order.  Z = sum_i z_i - N, a fixed-order binary64 reduction.  No atomic: equal inputs and equal ``slabs``
      give equal bits on every run and stream; ``slabs=0`` lets the library choose (at least four blocks per CU).
    - Attraction, per entry e = (i, j) of P: term = (float32(P_e) q_e) delta, added per row in a fixed order: att_i.
    - grad_i = 4 (x att_i - float32(R_i / Z)), binary32, each operation rounded.

  Iteration n (scikit-learn's ``_gradient_descent`` without its early stops; synchronous: Y^n is read, Y^(n+1) written),
  per coordinate in binary32, every operation rounded on its own:

      gain = (update grad < 0) ? gain + 0.2 : gain 0.8;  gain = max(gain, 0.01)
      update = mu update - (eta gain) grad;  y += update

  Iterations n < ``exploration`` use x = ``early_exaggeration`` and mu = 0.5, later ones x = 1 and mu = 0.8.

  Objective.  KL = sum_e P_e (log P_e + log1p(d2_e)) + (sum P) log Z, binary64; entries with P_e = 0 add nothing.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, device, graph, neighbors
from .device import _ptr, _torch
from .layout import _check_components, _check_positions, _number

TILE = 256                      # columns of a tile of the repulsion (PROSSTT_AMD_TSNE_TILE)
MAX_SLABS = 1024
MAX_ITERATIONS = 1 << 30
BAD_INDEX, BAD_SELF, BAD_DISTANCE = 1, 1 << 8, 1 << 16               # bits of the status word (prosstt_amd_tsne.h)
BAD_VALUES = ((BAD_INDEX, "a neighbour index lies outside [0, cells)"), (BAD_SELF, "a cell is listed as its own neighbour"),
              (BAD_DISTANCE, "a squared distance is negative, infinite or NaN"))


class Affinities(NamedTuple):
    """P in CSR (``indptr`` int64 (N + 1,), ``indices`` int32, ``data`` float64) and the ``beta`` (N,) of the conditional
    affinities.  numpy arrays, or device tensors for ``out="torch"``."""
    indptr: Any
    indices: Any
    data: Any
    beta: Any

    def to_csr(self):
        """P as an N x N ``scipy.sparse.csr_matrix`` (copied to the host if it lies on the device)."""
        return graph._csr(self.indptr, self.indices, self.data)


class TSNE(NamedTuple):
    """``embedding`` (N, c) float32: the positions after the last iteration; ``init`` (N, c) float32: the positions the run
    started from; ``kl_divergence``: the objective at ``embedding``; ``n_iter``: the iterations run; ``learning_rate``:
    as given or chosen.  numpy arrays, or device tensors for ``out="torch"``."""
    embedding: Any
    init: Any
    kl_divergence: float
    n_iter: int
    learning_rate: float


# ------------------------------------------------------------------------------------------------- argument checks

def _positive(name, v):
    if not (_number(v) and 0 < v < float("inf")):
        raise ValueError("%s must be a positive finite number (got %r)" % (name, v))
    return float(v)


def _integer(name, v, lo, hi):
    if not _number(v) or int(v) != v or not lo <= v <= hi:
        raise ValueError("need an integer %d <= %s <= %d (got %r)" % (lo, name, hi, v))
    return int(v)


def _check_perplexity(perplexity, k):
    if not (_number(perplexity) and 1 < perplexity < k):
        raise ValueError("need 1 < perplexity < neighbours = %d (got %r)" % (k, perplexity))
    return float(perplexity)


def _check_affinities(aff):
    """N of an ``Affinities`` whose arrays have the dtypes and shapes of one; ValueError otherwise.  No device."""
    if not isinstance(aff, Affinities):
        raise ValueError("need a tsne.Affinities")
    return graph._check_csr_shapes(aff)


def _check_descent(N, Y, slabs):
    """(the positions as ``_check_positions`` returns them, c)."""
    shape = tuple(getattr(Y, "shape", ()))
    if len(shape) != 2 or shape[1] not in (2, 3):
        raise ValueError("Y must be (%d, 2) or (%d, 3), not %s" % (N, N, shape))
    _integer("slabs", slabs, 0, MAX_SLABS)
    return _check_positions(Y, N, shape[1], "Y"), shape[1]


def _device_affinities(aff):
    """The ``Affinities`` as device tensors; a caller's CSR arrays and values are checked here, since the kernels trust
    them."""
    torch = _torch()
    g = graph._as_connectivities(device.need_device("graph"), graph.Connectivities(aff.indptr, aff.indices, aff.data, None, None))
    with torch.cuda.device(g.indptr.device):
        if not bool(torch.isfinite(g.data).all() & (g.data >= 0).all()):
            raise ValueError("the affinities must be finite and >= 0")
    return Affinities(g.indptr, g.indices, g.data, aff.beta)


# -------------------------------------------------------------------------------------------------------- affinities

def _affinities(L, idx, d2, N, k, perplexity):
    """(conditional affinities (N, k), beta (N,)) as device tensors from contiguous device ``idx`` and ``d2``."""
    torch = _torch()
    dev = idx.device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    cond = torch.empty((N, k), dtype=torch.float64, device=dev)
    beta = torch.empty(N, dtype=torch.float64, device=dev)
    _native.check(L.prosstt_amd_tsne_affinities(device.current_stream(dev), _ptr(idx), _ptr(d2), N, k, perplexity, _ptr(cond),
                                                _ptr(beta), _ptr(status)), "tsne")
    bits = int(status.item())
    if bits:
        raise ValueError("; ".join(text for bit, text in BAD_VALUES if bits & bit))
    return cond, beta


def _joint(L, idx, cond, N, k):
    return graph._symmetrize(device.need_device("graph"), idx, cond, N, k, L.prosstt_amd_tsne_symmetrize_fold, "tsne")


def _affinities_of(L, nb, perplexity):
    """The device ``Affinities`` of a checked ``Neighbors``."""
    torch = _torch()
    idx, d2, N, k = nb
    idx = graph._on_device(idx)
    d2 = graph._on_device(d2, idx.device)
    with torch.cuda.device(idx.device):
        cond, beta = _affinities(L, idx, d2, N, k, perplexity)
        return Affinities(*_joint(L, idx, cond, N, k), beta)


def affinities(nb, perplexity=30.0, *, out="scipy"):
    """The joint affinities P of the kNN graph ``nb`` (the module docstring's definition): ``Affinities(indptr, indices,
    data, beta)``; ``.to_csr()`` is the scipy matrix.

    ``nb``: a ``neighbors.Neighbors`` (or any pair) of int32 indices and float32 squared distances, (cells, k) each, as
    numpy arrays (copied to the current device) or as device tensors (used where they lie, on the current stream); scikit-
    learn takes k = 3 perplexity.  ``out``: "scipy" (host arrays) or "torch" (device tensors, no host copy).

    Raises ValueError, before any device use, for wrong dtypes or shapes, fewer than 3 cells, k outside 2 .. min(cells - 1,
    1024), a perplexity outside (1, k) or a bad ``out``; ValueError, from the device's check, for an index outside [0,
    cells) or equal to its row and for a squared distance that is negative or not finite."""
    if out not in ("scipy", "torch"):
        raise ValueError("out must be 'scipy' or 'torch'")
    checked = graph._check_neighbors(nb)
    perplexity = _check_perplexity(perplexity, checked[3])
    L = device.need_device("tsne")
    aff = _affinities_of(L, checked, perplexity)
    if out == "torch":
        return aff
    return Affinities(*(t.cpu().numpy() for t in aff))


# ---------------------------------------------------------------------------------------------------------- descent

def _workspace(dev, N, c, slabs):
    return device.workspace("tsne", "prosstt_amd_tsne_workspace_bytes", dev, N, c, slabs)


def _gradient(L, aff, y, exaggeration, slabs, ws, with_sums=False):
    """(grad (N, c) float32, Z as a one-element float64 tensor, sums of |q q delta| (N, c) float64 or None) on the device."""
    torch = _torch()
    N, c = y.shape
    dev = y.device
    grad = torch.empty_like(y)
    z = torch.empty(1, dtype=torch.float64, device=dev)
    sums = torch.empty((N, c), dtype=torch.float64, device=dev) if with_sums else None
    _native.check(L.prosstt_amd_tsne_gradient(device.current_stream(dev), _ptr(aff.indptr), _ptr(aff.indices), _ptr(aff.data),
                                              N, aff.indices.numel(), c, _ptr(y), float(exaggeration), int(slabs), _ptr(ws),
                                              ws.numel(), _ptr(grad), _ptr(z), _ptr(sums)), "tsne")
    return grad, z, sums


def gradient(aff, Y, *, exaggeration=1.0, slabs=0, _sums=False):
    """(grad, Z) of the module docstring's definition at the positions ``Y``: an (N, c) float32 device tensor and a float.

    ``aff``: an ``Affinities`` (host arrays or device tensors).  ``Y``: (N, c) finite numbers, c = 2 or 3, a numpy array or
    a device tensor.  ``slabs``: 1 .. 1024 runs of column tiles, or 0 for the library's choice; the bits depend on it."""
    N = _check_affinities(aff)
    Y, c = _check_descent(N, Y, slabs)
    _positive("exaggeration", exaggeration)
    L = device.need_device("tsne")
    torch = _torch()
    aff = _device_affinities(aff)
    dev = aff.indptr.device
    with torch.cuda.device(dev):
        y = graph._on_device(Y, dev).to(dev)
        grad, z, sums = _gradient(L, aff, y, exaggeration, slabs, _workspace(dev, N, c, slabs), _sums)
        return (grad, float(z.item()), sums) if _sums else (grad, float(z.item()))


def _iterations(L, aff, y0, y1, update, gains, it_begin, it_end, exploration, early_exaggeration, learning_rate, slabs, ws):
    """Enqueue the iterations on the current stream; the tensor of (y0, y1) that holds the result."""
    N, c = y0.shape
    _native.check(L.prosstt_amd_tsne_iterations(
        device.current_stream(y0.device), _ptr(aff.indptr), _ptr(aff.indices), _ptr(aff.data), N, aff.indices.numel(), c,
        _ptr(y0), _ptr(y1), _ptr(update), _ptr(gains), int(it_begin), int(it_end), int(exploration), float(early_exaggeration),
        float(learning_rate), int(slabs), _ptr(ws), ws.numel()), "tsne")
    return y1 if (it_end - it_begin) & 1 else y0


def _check_schedule(exploration, early_exaggeration, learning_rate):
    _integer("exploration", exploration, 0, MAX_ITERATIONS)
    _positive("early_exaggeration", early_exaggeration)
    _positive("learning_rate", learning_rate)


def optimize(aff, Y, it_begin, it_end, *, update=None, gains=None, exploration=250, early_exaggeration=12.0, learning_rate,
             slabs=0):
    """Iterations ``it_begin`` .. ``it_end - 1`` of the module docstring's definition from the positions ``Y``: new (N, c)
    float32 device tensors ``(Y, update, gains)``; the inputs are left as they are.  For tests and for resuming a run.

    ``update``, ``gains``: the state of the descent, (N, c) like ``Y``; None: zeros and ones, the state before iteration
    0."""
    N = _check_affinities(aff)
    Y, c = _check_descent(N, Y, slabs)
    _integer("it_begin", it_begin, 0, MAX_ITERATIONS)
    _integer("it_end", it_end, it_begin, MAX_ITERATIONS)
    _check_schedule(exploration, early_exaggeration, learning_rate)
    state = [None if t is None else _check_positions(t, N, c, name) for t, name in ((update, "update"), (gains, "gains"))]
    L = device.need_device("tsne")
    torch = _torch()
    aff = _device_affinities(aff)
    dev = aff.indptr.device
    with torch.cuda.device(dev):
        y0 = graph._on_device(Y, dev).to(dev).clone()
        y1 = torch.empty_like(y0)
        update = torch.zeros_like(y0) if state[0] is None else graph._on_device(state[0], dev).to(dev).clone()
        gains = torch.ones_like(y0) if state[1] is None else graph._on_device(state[1], dev).to(dev).clone()
        y = _iterations(L, aff, y0, y1, update, gains, it_begin, it_end, exploration, early_exaggeration, learning_rate, slabs,
                        _workspace(dev, N, c, slabs))
        return y, update, gains


def _objective(L, aff, y, slabs, ws):
    """KL of the definition at the device positions ``y``, a float."""
    torch = _torch()
    N, c = y.shape
    rows = torch.empty(N, dtype=torch.float64, device=y.device)
    _native.check(L.prosstt_amd_tsne_objective(device.current_stream(y.device), _ptr(aff.indptr), _ptr(aff.indices),
                                               _ptr(aff.data), N, aff.indices.numel(), c, _ptr(y), _ptr(rows)), "tsne")
    _, z, _ = _gradient(L, aff, y, 1.0, slabs, ws)
    return float((rows.sum() + aff.data.sum() * torch.log(z[0])).item())


# -------------------------------------------------------------------------------------------------------------- tsne

def _is_neighbors(X):
    return isinstance(X, tuple) and not isinstance(X, Affinities) and len(X) == 2


def _pca_start(panel, c):
    """The first c columns of the panel, scaled so that column 0 has standard deviation 1e-4, as float32 on the host."""
    first = panel[:, :c]
    first = first.detach().cpu().numpy() if not isinstance(first, np.ndarray) else first
    first = np.asarray(first, dtype=np.float64)
    spread = first[:, 0].std()
    if not (spread > 0 and np.isfinite(spread)):
        raise ValueError("init='pca' needs a first column that is finite and not constant")
    return (first / spread * 1e-4).astype(np.float32)


def tsne(X, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", n_iter=1000, exploration=250,
         init="pca", seed=0, slabs=0, out="numpy"):
    """The exact t-SNE layout of the cells (the module docstring's definition): ``TSNE(embedding, init, kl_divergence,
    n_iter, learning_rate)``.

    ``X``: an (N, d) score panel (a numpy array or a device tensor, ``embed.pca``'s scores usually: the function calls
    ``neighbors.knn(X, min(N - 1, 1024, int(3 perplexity)))`` itself), a ``neighbors.Neighbors`` with 2 <= k <= 1024 and
    perplexity < k, or an ``Affinities``.  ``n_components``: 2 or 3.  ``learning_rate``: "auto" is max(N /
    early_exaggeration / 4, 50), as in scikit-learn (scanpy passes 1000).  ``n_iter``: the iterations, of which the first
    ``exploration`` run with ``early_exaggeration`` and momentum 0.5.  ``init``: "pca" (needs a panel: its first
    n_components columns, scaled so that column 0 has standard deviation 1e-4), "random" (1e-4
    ``default_rng(seed).standard_normal``) or (N, n_components) positions.  ``slabs``: as in ``gradient``.  ``out``: "numpy"
    or "torch" (device tensors).  Equal calls give equal bits.

    Raises ValueError for a bad argument, before any device use where the input allows, and for what ``neighbors.knn`` and
    ``affinities`` refuse."""
    torch = _torch()
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    c = _check_components(n_components)
    _integer("n_iter", n_iter, 0, MAX_ITERATIONS)
    _integer("slabs", slabs, 0, MAX_SLABS)
    _integer("seed", seed, 0, (1 << 64) - 1)
    if learning_rate != "auto":
        _positive("learning_rate", learning_rate)
    _check_schedule(exploration, early_exaggeration, 1.0)
    if not (_number(perplexity) and perplexity > 1):
        raise ValueError("perplexity must be a number above 1 (got %r)" % (perplexity,))
    panel = nb = None
    if isinstance(X, Affinities):
        N = _check_affinities(X)
    elif _is_neighbors(X):
        nb = graph._check_neighbors(X)
        N = nb[2]
        _check_perplexity(perplexity, nb[3])
    else:
        panel = X if isinstance(X, torch.Tensor) else np.asarray(X)
        if len(panel.shape) != 2:
            raise ValueError("X must be an (N, d) panel, a Neighbors or an Affinities")
        N = int(panel.shape[0])
        if N < 3 or N >= 1 << 31:
            raise ValueError("need 3 <= cells < 2^31 (got %d)" % N)
        k = min(N - 1, neighbors.MAX_NEIGHBORS, int(3 * perplexity))
        if k < 2:
            raise ValueError("need at least 2 neighbours (got %d from %d cells and perplexity %r)" % (k, N, perplexity))
        _check_perplexity(perplexity, k)
    start = None
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError("init must be 'pca', 'random' or positions (got %r)" % (init,))
        if init == "pca" and (panel is None or panel.shape[1] < c):
            raise ValueError("init='pca' needs a score panel of at least n_components columns")
    else:
        start = _check_positions(init, N, c, "init")
    eta = max(N / float(early_exaggeration) / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)

    L = device.need_device("tsne")
    if panel is not None:
        found = neighbors.knn(panel, k, out="torch")
        aff = _affinities_of(L, graph._check_neighbors(found), float(perplexity))
    elif nb is not None:
        aff = _affinities_of(L, nb, float(perplexity))
    else:
        aff = _device_affinities(X)
    dev = aff.indptr.device
    with torch.cuda.device(dev):
        if start is None:
            start = (_pca_start(panel, c) if init == "pca" else
                     (1e-4 * np.random.default_rng(seed).standard_normal((N, c))).astype(np.float32))
        first = graph._on_device(start, dev).to(dev)
        y0 = first.clone()
        y1 = torch.empty_like(y0)
        update, gains = torch.zeros_like(y0), torch.ones_like(y0)
        ws = _workspace(dev, N, c, slabs)
        y = _iterations(L, aff, y0, y1, update, gains, 0, n_iter, exploration, early_exaggeration, eta, slabs, ws)
        kl = _objective(L, aff, y, slabs, ws)
        if out == "torch":
            return TSNE(y, first, kl, int(n_iter), eta)
        return TSNE(y.cpu().numpy(), first.cpu().numpy(), kl, int(n_iter), eta)
