"""
UMAP layouts of the connectivity graph of cells, computed on the device: the picture the reference's notebooks draw after
``pp.neighbors`` (scanpy's ``tl.umap``, ``obsm["X_umap"]``).

    p = embed.pca(X, sc); nb = neighbors.knn(p.scores, 14, out="torch")
    lay = layout.umap(nb)                        # lay.embedding (N, 2) float32: obsm["X_umap"]
    lay = layout.umap(graph.connectivities(nb, out="torch"), 3, init="random", seed=7)

The epochs run in libprosstt_amd_layout.so (include/prosstt_amd_layout.h); the spectral start uses graph.py's Lanczos
solver with libprosstt_amd_graph.so's product kernel; torch is the device plumbing.  There is no CPU fallback.

The definition.  Coordinates are binary32, schedules binary64.  (The correspondences with umap-learn are from reading it,
not from a run.)  umap-learn's optimiser is an in-place SGD whose threads race; this is its SYNCHRONOUS form: every epoch
reads the positions of the previous one and writes new ones, so equal inputs give equal bits.

  Input.  W in CSR as ``graph.Connectivities`` holds it (N rows, symmetric, int64 indptr, int32 indices, binary64 data, 3 <=
  N < 2^31; finite, >= 0, max > 0); p_e = W_e / max(W) for CSR position e, one IEEE division.  Positions Y are N x c,
  row-major binary32, c = 2 or 3.

  Parameters.  E = n_epochs, 1 <= E <= 4096; binary64 a, b, gamma, alpha0, of which the kernel rounds a, b and gamma to
  binary32 once; negative_sample_rate r, 0 <= r <= 31; seed, a uint64.

  Epoch n (0-based), for every row i independently, all reads from Y^n:
    - Entry e = (i, j) is active iff floor((n + 1) p_e) > floor(n p_e) (a binary64 product and floor).  Stateless; an edge
      is sampled floor(E p_e) times in all, so edges with p < 1 / E never are: umap-learn's ``epochs_per_sample`` schedule
      and its pruning of weak edges.
    - Attraction, per active entry: delta = y_i - y_j, d2 = sum delta^2, coef = -2 a b d2^(b - 1) / (a d2^b + 1) if d2 > 0,
      else 0; term = 2 clip(coef delta, -4, 4) per coordinate.  (The 2: W stores the pair in both directions with equal p,
      and umap-learn moves both ends on each sample.)
    - Repulsion, per active entry and s = 0 .. r - 1: k = ((h >> 32) N) >> 32, h = mix(base_n ^ (32 e + s)), base_n =
      mix(seed + 0x9E3779B97F4A7C15 (n + 1)), e the CSR position as uint64, all modulo 2^64;
          mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31.
      If k = i there is no term.  Otherwise delta = y_i - y_k, coef = 2 gamma b / ((0.001 + d2) (a d2^b + 1)) if d2 > 0,
      else 0; term = clip(coef delta, -4, 4).
    - alpha_n = alpha0 (1 - n / E), computed in binary64 and rounded to binary32.
    - y_i^(n+1) = y_i^n + alpha_n sum(terms): a lane's own partial sum in ascending order, then a fixed shuffle tree (the
      header says how items are dealt to lanes).  Equal inputs and an equal ``lanes_per_row`` give equal bits on every run
      and stream; there is no floating-point atomic.

  a and b.  ``find_ab_params(spread, min_dist)`` fits 1 / (1 + a x^(2 b)) to (x < min_dist ? 1 : exp(-(x - min_dist) /
  spread)) on linspace(0, 3 spread, 300) with scipy's ``curve_fit``, on the host: (1.0, 0.5) gives a = 0.5830300, b =
  1.3341670.

  Start.  ``init="spectral"``: columns 1 .. c of the leading eigenvectors of S = D^(-1/2) W D^(-1/2), S_ij = W_ij /
  sqrt(q_i q_j) with q = W 1 (symmetric to the bit), component 0 dropped; unit columns with graph.py's sign rule; then
  v (10 / max|v|) + 1e-4 default_rng(seed).standard_normal((N, c)), rescaled per coordinate to [0, 10] as 10 (x - min) /
  (max - min), cast to binary32.  ``graph.NotConverged`` propagates; a disconnected graph is the caller's case for one of
  the other two.  ``init="random"``: default_rng(seed).uniform(-10, 10, (N, c)), cast to binary32.  Or an (N, c) array or
  device tensor of finite numbers.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, device, graph
from .device import _ptr, _torch

LANES = graph.LANES
MAX_EPOCHS = 4096
MAX_RATE = 31
SPECTRAL_TOL = 1e-10            # the bound on the Lanczos residual estimates of the spectral start


class Layout(NamedTuple):
    """``embedding`` (N, c) float32: the positions after the last epoch; ``init`` (N, c) float32: the positions the run
    started from; ``a``, ``b``: the curve's parameters as given or fitted; ``n_epochs``: the epochs run.  numpy arrays, or
    device tensors for ``out="torch"``."""
    embedding: Any
    init: Any
    a: float
    b: float
    n_epochs: int


def find_ab_params(spread=1.0, min_dist=0.5):
    """(a, b) of the module docstring's fit, on the host."""
    from scipy.optimize import curve_fit
    if not (_number(spread) and 0 < spread < float("inf")):
        raise ValueError("spread must be a positive finite number (got %r)" % (spread,))
    if not (_number(min_dist) and 0 <= min_dist < 3 * spread):
        raise ValueError("need 0 <= min_dist < 3 spread (got %r)" % (min_dist,))
    x = np.linspace(0, 3 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), x, y)
    return float(a), float(b)


# ------------------------------------------------------------------------------------------------- argument checks

def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _check_components(c):
    if not _number(c) or int(c) != c or c not in (2, 3):
        raise ValueError("n_components must be 2 or 3 (got %r)" % (c,))
    return int(c)


def _check_epoch_args(n_epochs, a, b, gamma, alpha, rate, seed, lanes_per_row):
    if not _number(n_epochs) or int(n_epochs) != n_epochs or not 1 <= n_epochs <= MAX_EPOCHS:
        raise ValueError("need an integer 1 <= n_epochs <= %d (got %r)" % (MAX_EPOCHS, n_epochs))
    for name, v in (("a", a), ("b", b), ("alpha", alpha)):
        if not (_number(v) and 0 < v < float("inf")):
            raise ValueError("%s must be a positive finite number (got %r)" % (name, v))
    if not (_number(gamma) and 0 <= gamma < float("inf")):
        raise ValueError("gamma must be a finite number >= 0 (got %r)" % (gamma,))
    if not _number(rate) or int(rate) != rate or not 0 <= rate <= MAX_RATE:
        raise ValueError("need an integer 0 <= negative_sample_rate <= %d (got %r)" % (MAX_RATE, rate))
    if not _number(seed) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64) (got %r)" % (seed,))
    if lanes_per_row not in LANES:
        raise ValueError("lanes_per_row must be 0, 4, 16 or 64 (got %r)" % (lanes_per_row,))


def _check_positions(Y, N, c, what):
    """A float32 (N, c) host array or device tensor as it came, finite; ValueError otherwise."""
    torch = _torch()
    if not isinstance(Y, torch.Tensor):
        Y = np.asarray(Y)
        if Y.dtype.kind not in "fiu":
            raise ValueError("%s must be an array of numbers, not %s" % (what, Y.dtype))
    if tuple(Y.shape) != (N, c):
        raise ValueError("%s must be (%d, %d), not %s" % (what, N, c, tuple(Y.shape)))
    if isinstance(Y, np.ndarray):
        Y = np.ascontiguousarray(Y, dtype=np.float32)
        finite = bool(torch.isfinite(torch.from_numpy(Y)).all())
    else:
        if not Y.dtype.is_floating_point:
            raise ValueError("%s must be a floating-point tensor, not %s" % (what, Y.dtype))
        Y = Y.detach().to(torch.float32)
        finite = bool(torch.isfinite(Y).all())
    if not finite:
        raise ValueError("%s must be finite" % what)
    return Y


# ------------------------------------------------------------------------------------------------------------ epochs

def _weights(g):
    """p of the definition from a ``Connectivities`` of device tensors; W is checked here."""
    torch = _torch()
    if g.data.numel() == 0:
        raise ValueError("the connectivities hold no entry")
    top = g.data.max()
    if not bool(torch.isfinite(g.data).all() & (g.data >= 0).all() & (top > 0)):
        raise ValueError("the connectivities must be finite and >= 0, with a largest entry > 0")
    return g.data / top


def _epochs(L, g, p, y0, y1, epoch_begin, epoch_end, n_epochs, a, b, gamma, alpha, rate, seed, lanes_per_row):
    """Enqueue the epochs on the current stream; the tensor of (y0, y1) that holds the result."""
    N, c = y0.shape
    _native.check(L.prosstt_amd_layout_epochs(
        device.current_stream(y0.device), _ptr(g.indptr), _ptr(g.indices), _ptr(p), N, g.indices.numel(), c, _ptr(y0), _ptr(y1),
        int(epoch_begin), int(epoch_end), int(n_epochs), float(a), float(b), float(gamma), float(alpha), int(rate), int(seed),
        int(lanes_per_row)), "layout")
    return y1 if (epoch_end - epoch_begin) & 1 else y0


def _negatives(seed, epoch, e_begin, count, rate, N):
    """k of the definition's hash for entries e_begin .. e_begin + count - 1 and s = 0 .. rate - 1: a (count, rate) int32
    device tensor.  The probe the tests compare with the model bit for bit."""
    torch = _torch()
    L = device.need_device("layout")
    out = torch.empty((int(count), int(rate)), dtype=torch.int32, device="cuda")
    if out.numel() == 0:
        return out
    _native.check(L.prosstt_amd_layout_negatives(device.current_stream(out.device), int(seed), int(epoch), int(e_begin),
                                                 int(count), int(rate), int(N), _ptr(out)), "layout")
    return out


def optimize(conn, Y, epoch_begin, epoch_end, *, n_epochs, a, b, gamma=1.0, alpha=1.0, negative_sample_rate=5, seed=0,
             lanes_per_row=0):
    """Epochs ``epoch_begin`` .. ``epoch_end - 1`` of a run of ``n_epochs`` (the module docstring's definition) from the
    positions ``Y``: a new (N, c) float32 device tensor; ``Y`` is left as it is.  For tests and for resuming a run.

    ``conn``: a ``graph.Connectivities`` (host arrays or device tensors).  ``Y``: (N, c) finite numbers, c = 2 or 3, a
    numpy array or a device tensor."""
    if not isinstance(conn, graph.Connectivities):
        raise ValueError("need a graph.Connectivities")
    N = graph._check_csr_shapes(conn)
    shape = tuple(getattr(Y, "shape", ()))
    if len(shape) != 2 or shape[1] not in (2, 3):
        raise ValueError("Y must be (%d, 2) or (%d, 3), not %s" % (N, N, shape))
    _check_epoch_args(n_epochs, a, b, gamma, alpha, negative_sample_rate, seed, lanes_per_row)
    for name, v in (("epoch_begin", epoch_begin), ("epoch_end", epoch_end)):
        if not _number(v) or int(v) != v:
            raise ValueError("%s must be an integer (got %r)" % (name, v))
    if not 0 <= epoch_begin <= epoch_end <= n_epochs:
        raise ValueError("need 0 <= epoch_begin <= epoch_end <= n_epochs (got %r, %r, %r)" % (epoch_begin, epoch_end, n_epochs))
    Y = _check_positions(Y, N, shape[1], "Y")
    L = device.need_device("layout")
    torch = _torch()
    g = graph._as_connectivities(device.need_device("graph"), conn)
    with torch.cuda.device(g.indptr.device):
        p = _weights(g)
        y0 = graph._on_device(Y, g.indptr.device).to(g.indptr.device).clone()
        y1 = torch.empty_like(y0)
        return _epochs(L, g, p, y0, y1, epoch_begin, epoch_end, n_epochs, a, b, gamma, alpha, negative_sample_rate, seed,
                       lanes_per_row)


# ------------------------------------------------------------------------------------------------------------- start

def _spectral(Lg, g, c, seed):
    """(eigenvalues (host, c), unit eigenvectors (device, N x c)) of components 1 .. c of S."""
    torch = _torch()
    N = g.indptr.numel() - 1
    if c + 1 >= N:
        raise ValueError("need n_components + 1 < cells = %d" % N)
    q = graph._transitions(Lg, g).q
    rows = torch.repeat_interleave(torch.arange(N, device=q.device), g.indptr[1:] - g.indptr[:-1])
    S = g.data / torch.sqrt(q[rows] * q[g.indices.long()])
    values, vectors, _, _ = graph._lanczos(Lg, graph.Transitions(g.indptr, g.indices, S, q, None), c + 1, SPECTRAL_TOL,
                                           int(seed), min(N, graph.MAX_STEPS))
    return values[1:], graph._fix_signs(vectors)[:, 1:]


def _scale_start(vectors, seed):
    """The spectral start from unit eigenvectors (N, c), a host array: the module docstring's formula."""
    v = np.asarray(vectors, dtype=np.float64)
    x = v * (10.0 / np.abs(v).max()) + 1e-4 * np.random.default_rng(seed).standard_normal(v.shape)
    lo, hi = x.min(axis=0), x.max(axis=0)
    return (10.0 * (x - lo) / (hi - lo)).astype(np.float32)


def spectral_vectors(graph_, n_components=2, *, seed=0, out="numpy"):
    """(eigenvalues (c,), unit eigenvectors (N, c)) of components 1 .. c of S = D^(-1/2) W D^(-1/2): what the spectral
    start is scaled from.  ``graph_``: a ``Neighbors`` or a ``Connectivities``; ``seed``: of the Lanczos start vector."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    c = _check_components(n_components)
    N = graph._host_checks(graph_)
    if not _number(seed) or int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64) (got %r)" % (seed,))
    if c + 1 >= N:
        raise ValueError("need n_components + 1 < cells = %d" % N)
    Lg = device.need_device("graph")
    torch = _torch()
    g = graph._as_connectivities(Lg, graph_)
    with torch.cuda.device(g.indptr.device):
        _weights(g)
        values, vectors = _spectral(Lg, g, c, seed)
        if out == "torch":
            return torch.from_numpy(np.ascontiguousarray(values)).to(vectors.device), vectors
        return values, vectors.cpu().numpy()


# -------------------------------------------------------------------------------------------------------------- umap

def umap(graph_, n_components=2, *, min_dist=0.5, spread=1.0, n_epochs=None, alpha=1.0, gamma=1.0, negative_sample_rate=5,
         init="spectral", seed=0, a=None, b=None, lanes_per_row=0, out="numpy"):
    """The UMAP layout of a kNN graph (the module docstring's definition): ``Layout(embedding, init, a, b, n_epochs)``.

    ``graph_``: a ``neighbors.Neighbors`` (numpy arrays or device tensors) or a ``graph.Connectivities``, as
    ``graph.diffmap`` takes them.  ``n_components``: 2 or 3.  ``a``, ``b``: the curve's parameters; None (both): fitted
    from ``spread`` and ``min_dist`` by ``find_ab_params``.  ``n_epochs``: None means 500 for at most 10 000 cells and 200
    beyond, as in umap-learn.  ``alpha``: the first learning rate; ``gamma``: the weight of the repulsion.  ``init``:
    "spectral", "random" or (N, n_components) positions.  ``seed``: of the negative samples, of the start's random numbers
    and of the Lanczos start vector; equal calls give equal bits.  ``lanes_per_row``: 4, 16 or 64 lanes own a row; 0 lets
    the library choose.  ``out``: "numpy" or "torch" (device tensors).

    Raises ValueError for what ``graph.diffmap`` refuses of a graph, for a bad argument (before any device use where the
    input allows) and for connectivities that are not finite, negative or all zero; ``graph.NotConverged`` from the
    spectral start."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    c = _check_components(n_components)
    N = graph._host_checks(graph_)
    if (a is None) != (b is None):
        raise ValueError("give both a and b, or neither")
    if n_epochs is None:
        n_epochs = 500 if N <= 10000 else 200
    _check_epoch_args(n_epochs, 1.0 if a is None else a, 1.0 if b is None else b, gamma, alpha, negative_sample_rate, seed,
                      lanes_per_row)
    start = None
    if isinstance(init, str):
        if init not in ("spectral", "random"):
            raise ValueError("init must be 'spectral', 'random' or positions (got %r)" % (init,))
        if init == "spectral" and c + 1 >= N:
            raise ValueError("need n_components + 1 < cells = %d for the spectral start" % N)
    else:
        start = _check_positions(init, N, c, "init")
    if a is None:
        a, b = find_ab_params(spread, min_dist)
    L = device.need_device("layout")
    Lg = device.need_device("graph")
    torch = _torch()
    g = graph._as_connectivities(Lg, graph_)
    dev = g.indptr.device
    with torch.cuda.device(dev):
        p = _weights(g)
        if isinstance(init, str) and init == "spectral":
            _, vectors = _spectral(Lg, g, c, seed)
            start = _scale_start(vectors.cpu().numpy(), seed)
        elif start is None:
            start = np.random.default_rng(seed).uniform(-10, 10, (N, c)).astype(np.float32)
        first = graph._on_device(start, dev).to(dev)
        y0 = first.clone()
        y1 = torch.empty_like(y0)
        y = _epochs(L, g, p, y0, y1, 0, n_epochs, n_epochs, a, b, gamma, alpha, negative_sample_rate, seed, lanes_per_row)
        if out == "torch":
            return Layout(y, first, float(a), float(b), int(n_epochs))
        return Layout(y.cpu().numpy(), first.cpu().numpy(), float(a), float(b), int(n_epochs))
