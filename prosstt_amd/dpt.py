"""
Diffusion pseudotime of the cells and its first branching, computed on the device: the step that ``graph.diffmap`` exists
for (Haghverdi et al. 2016; scanpy's ``tl.dpt``).  It gives back what the simulation knows, a pseudotime and a branch per
cell, to compare with ``pt`` and ``br`` (``evaluate.trajectory`` does).

    dm = graph.diffmap(neighbors.knn(p.scores, 14, out="torch"), out="torch")
    res = dpt.dpt(dm, root, n_branchings=1)      # res.pseudotime (N,) float64, res.groups (N,) int8, res.tips, res.splits
    d = dpt.distances(dm, [root, 7])             # (2, N) float64 rows of the DPT distance

The distance rows and the concordance sums over all N^2 pairs run in libprosstt_amd_dpt.so (include/prosstt_amd_dpt.h);
sorts, ``unique``, prefix sums, gathers and the argmax are torch's device plumbing on the input's stream.  There is no CPU
fallback.

The rule for the distance weights is from memory of scanpy's ``_get_dpt_row``, not from a run of it.  The branching is
defined here in full: it follows the 2016 paper and the outline of scanpy's ``haghverdi16`` flavour and is a copy of neither.

The definition.

  Input: a ``graph.DiffusionMap`` with eigenvalues lambda (n_comps,) and eigenvectors Psi (N, n_comps), binary64, as numpy
  arrays or device tensors; ``root``, a cell index; 1 <= n_dcs <= n_comps (default min(10, n_comps)).  The weights are
  computed on the host in binary64: w_l = lambda_l / (1 - lambda_l) where lambda_l < 0.9994 and w_l = 1 otherwise (the
  division is not evaluated where it is not selected: lambda_0 is 1).

  Distance row of a source cell s: acc = 0; for l ascending: t = w_l (psi_sl - psi_jl), acc = acc + t t, every operation a
  binary64 operation rounded on its own; d(s, j) = sqrt(acc).

  Pseudotime: d(root, .) / max_j d(root, j).  Connected components get no special treatment (scanpy sets infinity for the
  cells the root does not reach): a disconnected graph is the caller's problem, as in ``graph.diffmap``.

  Branching (``n_branchings`` = 1; every argmax takes the lowest index among equals).
    Tips: t0 = argmax d(root, .), t1 = argmax d(t0, .), t2 = argmax (d(t0, .) + d(t1, .)).
    For each rotation (a, b, c) of (t0, t1, t2), that is (t0, t1, t2), (t1, t2, t0), (t2, t0, t1): ``order`` is the stable
    ascending sort of d(a, .); ru and rv are the dense int32 ranks of d(b, .)[order] and d(c, .)[order] (equal values get
    equal ranks: ``unique(return_inverse=True)``).  For positions p, q: s_pq = sgn(ru_p - ru_q) sgn(rv_p - rv_q), and the
    kernel's output, int64 each: lower_r = sum_{p < r} s_pr, upper_r = sum_{q > r} s_rq.
    Split scan (int64, exact): H(n) = sum_{r < n} lower_r, the sum over the pairs inside the first n positions, and T(n) =
    sum_{r >= n} upper_r, the sum over the pairs inside the rest.  In binary64 (each integer rounded once):
    diff(n) = H(n) / (n (n - 1) / 2) - T(n) / ((N - n)(N - n - 1) / 2); n* = argmax diff(n) over m <= n <= N - m, m =
    ``min_group_size``, 2 <= m and 2 m <= N.  Near tip a the distances to b and c move together (tau near +1), past the
    branching against each other (tau near -1): the head ``order[:n*]`` is tip a's arm.
    Groups: a cell in exactly one of the three heads gets 1, 2 or 3 (for t0, t1, t2); a cell in none or in several gets 0,
    the branching region.
  tau is Kendall's tau-a: ties count 0 in the sum.  (scanpy takes scipy's tau-b once and approximate updates after it.)
"""
from typing import Any, NamedTuple

import numpy as np

from . import _native, device, graph
from .device import _ptr, _torch
from .layout import _number

MAX_SLABS = 1024                # PROSSTT_AMD_DPT_MAX_SLABS
MAX_BATCH = 1024
MAX_SOURCES = 65535
THRESHOLD = 0.9994              # eigenvalues from here on get the weight 1


class DPT(NamedTuple):
    """``pseudotime`` (N,) float64; ``groups`` (N,) int8: 1, 2, 3 for the arms of the three tips, 0 for the branching
    region; ``tips``: the cells (t0, t1, t2); ``splits``: the three head lengths n*.  ``groups``, ``tips`` and ``splits``
    are None for ``n_branchings=0``.  numpy arrays, or device tensors for ``out="torch"``; tips and splits are ints."""
    pseudotime: Any
    groups: Any
    tips: Any
    splits: Any


# ------------------------------------------------------------------------------------------------- argument checks

def _integer(name, v, lo, hi):
    if not _number(v) or int(v) != v or not lo <= v <= hi:
        raise ValueError("need an integer %d <= %s <= %d (got %r)" % (lo, name, hi, v))
    return int(v)


def _check_map(dm, n_dcs):
    """(N, n_comps, n_dcs) of an accepted ``graph.DiffusionMap``; ValueError otherwise.  Touches no device."""
    torch = _torch()
    if not isinstance(dm, graph.DiffusionMap):
        raise ValueError("need a graph.DiffusionMap")
    for name, arr, dims in (("eigenvalues", dm.eigenvalues, 1), ("eigenvectors", dm.eigenvectors, 2)):
        want = torch.float64 if isinstance(arr, torch.Tensor) else np.dtype(np.float64)
        if not isinstance(arr, (torch.Tensor, np.ndarray)) or arr.dtype != want or len(arr.shape) != dims:
            raise ValueError("%s must be a %d-D float64 array" % (name, dims))
    N, n_comps = (int(v) for v in dm.eigenvectors.shape)
    if int(dm.eigenvalues.shape[0]) != n_comps:
        raise ValueError("%d eigenvalues for %d eigenvectors" % (int(dm.eigenvalues.shape[0]), n_comps))
    if N < 3 or N >= 1 << 31:
        raise ValueError("need 3 <= cells < 2^31 (got %d)" % N)
    if not 1 <= n_comps < N:
        raise ValueError("need 1 <= n_comps < cells = %d (got %d)" % (N, n_comps))
    if n_dcs is None:
        n_dcs = min(10, n_comps)
    elif not _number(n_dcs) or int(n_dcs) != n_dcs or not 1 <= n_dcs <= n_comps:
        raise ValueError("need an integer 1 <= n_dcs <= n_comps = %d (got %r)" % (n_comps, n_dcs))
    return N, n_comps, int(n_dcs)


def _check_sources(sources, N):
    """The cell indices as an int64 host array; ValueError otherwise."""
    try:
        arr = np.asarray(sources)
    except Exception:
        raise ValueError("sources must be a sequence of cell indices") from None
    if arr.ndim != 1 or arr.dtype.kind not in "iu" or not 1 <= arr.size <= MAX_SOURCES:
        raise ValueError("sources must be 1 to %d integer cell indices" % MAX_SOURCES)
    if arr.min() < 0 or arr.max() >= N:
        raise ValueError("a source lies outside [0, cells = %d)" % N)
    return arr.astype(np.int64)


def _check_ranks(ru, rv):
    """(ru, rv, batch, N) of int32 (batch, N) rank arrays, host arrays or device tensors as they came; ValueError
    otherwise.  Host arrays are checked for values outside [0, N) here."""
    torch = _torch()
    pair = []
    for name, arr in (("ru", ru), ("rv", rv)):
        if isinstance(arr, torch.Tensor):
            if arr.dtype != torch.int32:
                raise ValueError("%s must be int32, not %s" % (name, arr.dtype))
            if arr.device.type == "cpu":
                arr = arr.detach().numpy()
        else:
            arr = np.asarray(arr)
            if arr.dtype != np.int32:
                raise ValueError("%s must be int32, not %s" % (name, arr.dtype))
        if len(arr.shape) != 2:
            raise ValueError("%s must be (batch, cells), not %d dimensions" % (name, len(arr.shape)))
        pair.append(arr)
    ru, rv = pair
    if tuple(ru.shape) != tuple(rv.shape):
        raise ValueError("ru %s and rv %s differ in shape" % (tuple(ru.shape), tuple(rv.shape)))
    if isinstance(ru, np.ndarray) != isinstance(rv, np.ndarray) or (not isinstance(ru, np.ndarray) and ru.device != rv.device):
        raise ValueError("ru and rv must lie in the same place")
    batch, N = (int(v) for v in ru.shape)
    if N < 3 or N >= 1 << 31:
        raise ValueError("need 3 <= cells < 2^31 (got %d)" % N)
    if not 1 <= batch <= MAX_BATCH:
        raise ValueError("need 1 <= batch <= %d (got %d)" % (MAX_BATCH, batch))
    for name, arr in (("ru", ru), ("rv", rv)):
        if isinstance(arr, np.ndarray) and (arr.min() < 0 or arr.max() >= N):
            raise ValueError("a rank of %s lies outside [0, cells = %d)" % (name, N))
    return ru, rv, batch, N


def weights(eigenvalues, n_dcs):
    """The distance weights w_l, l < ``n_dcs``, of the module docstring's definition: a float64 host array."""
    lam = np.array(eigenvalues[:n_dcs], dtype=np.float64)
    w = np.ones_like(lam)
    below = lam < THRESHOLD
    w[below] = lam[below] / (1.0 - lam[below])
    return w


# ------------------------------------------------------------------------------------------------------- device steps

def _device_map(dm, n_dcs):
    """(Psi as a contiguous device tensor, the weights as a device tensor)."""
    psi = graph._on_device(dm.eigenvectors)
    lam = dm.eigenvalues
    lam = lam if isinstance(lam, np.ndarray) else lam.detach().cpu().numpy()
    return psi, graph._on_device(weights(lam, n_dcs), psi.device)


def _rows(L, psi, w, sources):
    """d(sources[i], .) as an (n_sources, N) float64 device tensor; ``sources`` an int64 device tensor."""
    torch = _torch()
    N, n_comps = psi.shape
    out = torch.empty((sources.numel(), N), dtype=torch.float64, device=psi.device)
    _native.check(L.prosstt_amd_dpt_rows(device.current_stream(psi.device), _ptr(psi), n_comps, _ptr(w), N, w.numel(),
                                         _ptr(sources), sources.numel(), _ptr(out)), "dpt")
    return out


def _concordance(L, ru, rv, slabs):
    """(lower, upper) int64 (batch, N) device tensors of contiguous int32 device ranks."""
    torch = _torch()
    batch, N = ru.shape
    dev = ru.device
    ws = device.workspace("dpt", "prosstt_amd_dpt_workspace_bytes", dev, N, batch, int(slabs))
    lower = torch.empty((batch, N), dtype=torch.int64, device=dev)
    upper = torch.empty((batch, N), dtype=torch.int64, device=dev)
    _native.check(L.prosstt_amd_dpt_concordance(device.current_stream(dev), _ptr(ru), _ptr(rv), N, batch, int(slabs), _ptr(ws),
                                                ws.numel(), _ptr(lower), _ptr(upper)), "dpt")
    return lower, upper


def _argmax_lowest(x):
    """The lowest index of the largest entry of the vector ``x``, a 0-d int64 device tensor (the length if x holds a NaN)."""
    torch = _torch()
    n = x.shape[0]
    return torch.where(x == x.max(), torch.arange(n, device=x.device), n).min()


def _ranks(D):
    """(order, ru, rv) of the three rotations of the distance rows ``D`` (3, N) of the tips: int64 and int32 (3, N)."""
    torch = _torch()
    order = torch.sort(D, dim=1, stable=True).indices
    dense = [[torch.unique(D[b][order[a]], sorted=True, return_inverse=True)[1].to(torch.int32) for b in ((a + 1) % 3, (a + 2) % 3)]
             for a in range(3)]
    return order, torch.stack([d[0] for d in dense]), torch.stack([d[1] for d in dense])


def _splits(lower, upper, m):
    """n* of the definition per row of ``lower`` and ``upper`` (batch, N): an int64 (batch,) device tensor."""
    torch = _torch()
    N = lower.shape[1]
    n = torch.arange(m, N - m + 1, device=lower.device)
    head = torch.cumsum(lower, 1)[:, n - 1]                               # H(n): positions below n
    tail = upper.sum(1, keepdim=True) - torch.cumsum(upper, 1)[:, n - 1]  # T(n): positions from n on
    head_pairs, tail_pairs = (n * (n - 1)) // 2, ((N - n) * (N - n - 1)) // 2
    diff = head.double() / head_pairs.double() - tail.double() / tail_pairs.double()
    at = torch.arange(n.numel(), device=lower.device)
    return torch.where(diff == diff.amax(1, keepdim=True), at, n.numel()).amin(1) + m


def _groups(order, splits):
    """The group of every cell from the three orders (3, N) and head lengths (3,): int8 (N,)."""
    torch = _torch()
    N = order.shape[1]
    in_head = torch.zeros((3, N), dtype=torch.bool, device=order.device)
    in_head.scatter_(1, order, torch.arange(N, device=order.device)[None, :] < splits[:, None])
    label = (in_head * torch.tensor([[1], [2], [3]], device=order.device)).sum(0)
    return torch.where(in_head.sum(0) == 1, label, 0).to(torch.int8)


def _branching(L, psi, w, d_root, m, slabs):
    """Every stage of the branching as device tensors: tips (3,), rows (3, N), order, ru, rv, lower, upper (3, N), splits
    (3,), groups (N,)."""
    torch = _torch()
    t0 = _argmax_lowest(d_root)
    d0 = _rows(L, psi, w, t0.reshape(1))[0]
    t1 = _argmax_lowest(d0)
    d1 = _rows(L, psi, w, t1.reshape(1))[0]
    t2 = _argmax_lowest(d0 + d1)
    d2 = _rows(L, psi, w, t2.reshape(1))[0]
    D = torch.stack([d0, d1, d2])
    order, ru, rv = _ranks(D)
    lower, upper = _concordance(L, ru, rv, slabs)
    splits = _splits(lower, upper, m)
    return dict(tips=torch.stack([t0, t1, t2]), rows=D, order=order, ru=ru, rv=rv, lower=lower, upper=upper, splits=splits,
                groups=_groups(order, splits))


# -------------------------------------------------------------------------------------------------------- entry points

def distances(dm, sources, n_dcs=None, *, out="numpy"):
    """The distance rows d(s, .) of the module docstring's definition for the cells ``sources`` (1 to 65535 indices):
    (len(sources), N) float64, a numpy array or, for ``out="torch"``, a device tensor.

    Raises ValueError, before any device use, for anything but a ``graph.DiffusionMap`` of float64 arrays, ``n_dcs``
    outside 1 .. n_comps, a source outside [0, cells) or a bad ``out``."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    N, _, n_dcs = _check_map(dm, n_dcs)
    sources = _check_sources(sources, N)
    L = device.need_device("dpt")
    torch = _torch()
    psi, w = _device_map(dm, n_dcs)
    with torch.cuda.device(psi.device):
        d = _rows(L, psi, w, graph._on_device(sources, psi.device))
        return d if out == "torch" else d.cpu().numpy()


def concordance(ru, rv, slabs=0):
    """(lower, upper) of the module docstring's definition for the sequence pairs (ru[b], rv[b]): int64 (batch, N) each,
    numpy arrays for numpy input and device tensors for device tensors.

    ``ru``, ``rv``: int32 (batch, N) dense ranks in [0, N), 1 <= batch <= 1024.  ``slabs``: 1 .. 1024 runs of column tiles,
    or 0 for the library's choice; the result does not depend on it.

    Raises ValueError for wrong dtypes or shapes and a bad ``slabs``, and for a rank outside [0, N): before any device use
    for host arrays, from a check on the device for device tensors."""
    ru, rv, batch, N = _check_ranks(ru, rv)
    _integer("slabs", slabs, 0, MAX_SLABS)
    L = device.need_device("dpt")
    torch = _torch()
    host = isinstance(ru, np.ndarray)
    ru = graph._on_device(ru)
    rv = graph._on_device(rv, ru.device)
    with torch.cuda.device(ru.device):
        if not host and not bool((ru >= 0).all() & (ru < N).all() & (rv >= 0).all() & (rv < N).all()):
            raise ValueError("a rank lies outside [0, cells = %d)" % N)
        lower, upper = _concordance(L, ru, rv, slabs)
        return (lower.cpu().numpy(), upper.cpu().numpy()) if host else (lower, upper)


def dpt(dm, root, n_dcs=None, *, n_branchings=0, min_group_size=5, slabs=0, out="numpy", _stages=False):
    """Diffusion pseudotime from the cell ``root`` and, for ``n_branchings=1``, the first branching (the module docstring's
    definition): ``DPT(pseudotime, groups, tips, splits)``.

    ``dm``: a ``graph.DiffusionMap`` (numpy arrays, copied to the current device, or device tensors, used where they lie on
    the current stream).  ``n_dcs``: the components used, 1 .. n_comps (None: min(10, n_comps)).  ``n_branchings``: 0 or
    1.  ``min_group_size``: the fewest cells on either side of a split, 2 <= m, 2 m <= cells.  ``slabs``: as in
    ``concordance``.  ``out``: "numpy" or "torch" (device tensors).  Equal calls give equal bits.

    Raises ValueError for a bad argument, before any device use."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    N, _, n_dcs = _check_map(dm, n_dcs)
    root = _integer("root", root, 0, N - 1)
    if not _number(n_branchings) or n_branchings not in (0, 1):
        raise ValueError("n_branchings must be 0 or 1 (got %r)" % (n_branchings,))
    if not _number(min_group_size) or int(min_group_size) != min_group_size or min_group_size < 2 or 2 * min_group_size > N:
        raise ValueError("need an integer min_group_size with 2 <= min_group_size and 2 min_group_size <= cells = %d (got %r)"
                         % (N, min_group_size))
    _integer("slabs", slabs, 0, MAX_SLABS)
    L = device.need_device("dpt")
    torch = _torch()
    psi, w = _device_map(dm, n_dcs)
    with torch.cuda.device(psi.device):
        d_root = _rows(L, psi, w, torch.tensor([root], dtype=torch.int64, device=psi.device))[0]
        pseudotime = d_root / d_root.max()
        stages = _branching(L, psi, w, d_root, int(min_group_size), slabs) if n_branchings else None
        groups = tips = splits = None
        if stages is not None:
            groups = stages["groups"]
            tips = tuple(int(v) for v in stages["tips"].cpu())
            splits = tuple(int(v) for v in stages["splits"].cpu())
        if out == "numpy":
            pseudotime = pseudotime.cpu().numpy()
            groups = None if groups is None else groups.cpu().numpy()
        res = DPT(pseudotime, groups, tips, splits)
        return (res, dict(stages or {}, root_row=d_root)) if _stages else res
