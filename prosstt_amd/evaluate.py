"""
Scores of an inferred trajectory against the simulated truth, computed on the device: how close ``ptree``'s, ``dpt``'s or
``mapping``'s answer (or anyone's) is to the ``pt``, ``br`` and ``Tree`` that the simulation knows.

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    lf = ptree.principal_tree(embed.pca(X, sc, 10).scores).to_tree(root=int(np.argmin(pt)), G=X.shape[1])
    ev = evaluate.trajectory(t, pt, br, lf)
    ev.labels.accuracy, ev.labels.ari                 # the branches, as a clustering
    ev.ordering.comparable.gamma, ev.ordering.spearman    # the order of the cells on a common lineage
    ev.distances.pearson()                            # the geodesic distances on the two trees, over all pairs

The sums over all N (N - 1) / 2 pairs of cells run in libprosstt_amd_evaluate.so (include/prosstt_amd_evaluate.h has the
definition): exact integers, binned by the pair of true branches.  The stable sort by branch, ``unique`` for the dense ranks,
``bincount`` and the gathers are torch's device plumbing; the ratios are taken on the host from Python integers.  There is
no CPU fallback.

The definitions.

  Pair sets.  The cells are sorted by their true class (stable).  For classes p <= q the pair set is every (i, j) with i in
  p and j in q (p < q), or every i < j in p (p = q): each unordered pair of cells lies in one set.

  Pair counts of two integer sequences a and b: sa = sgn(a_i - a_j), sb = sgn(b_i - b_j); per class pair S = sum sa sb, P =
  sum (sa sb)^2, A2 = sum sa^2, B2 = sum sb^2.  Concordant C = (P + S) / 2, discordant D = (P - S) / 2.  Over the class pairs
  a mask selects (all of them by default), with the sums added first: Goodman-Kruskal's gamma = S / P = (C - D) / (C + D),
  Kendall's tau-a = S / pairs and tau-b = S / sqrt(A2 B2).  A ratio whose denominator is 0 is NaN.

  Pair moments of two trees.  A cell's depth on a tree is h = rint((t - t0) ticks) for its absolute pseudotime t, the tree's
  first time t0 and ``ticks`` steps per unit of pseudotime (0 <= h <= 65 535).  The junction table J[p][q] is rint((e - t0)
  ticks) for ``trends._Nodes.junction``'s e, and 65 535 where that is None (one branch is the other or its ancestor).  d(i, j)
  = h_i + h_j - 2 min(h_i, h_j, J[c_i][c_j]): ``trends``' tree distance in ticks.  With d on the true tree and d2 on the
  second: per true class pair sum d, sum d2, sum d^2, sum d2^2, sum d d2, exact.  Pearson's r over n pairs is
  (n Sdd2 - Sd Sd2) / sqrt((n Sdd - Sd^2) (n Sd2d2 - Sd2^2)), the numerator and the product as integers.

  Labels.  The contingency table n_uv of the true and the found labels over the cells labelled on both sides (a negative
  integer label means none).  The adjusted Rand index (Hubert and Arabie) from the integers; the normalised mutual information
  with the arithmetic mean of the entropies; per true class the best Jaccard index n_uv / (n_u + n_v - n_uv) and the best F1 =
  2 n_uv / (n_u + n_v) over the found classes; ``accuracy``: the share of cells on their true class under the one-to-one
  matching of found to true labels that maximises it (``scipy.optimize.linear_sum_assignment``).

Out of scope: more than 64 branches, waypoint sampling, trees given as arbitrary graphs, edge-flip and topology scores,
several devices, a matrix in chunks of cells (the pairs couple the cells).
"""
import math
from typing import Any, NamedTuple, Optional

import numpy as np

from . import _native, device
from .device import _ptr, _torch
from .trends import _Nodes

MAX_CLASSES = 64                        # PROSSTT_AMD_EVALUATE_MAX_CLASSES
MAX_DEPTH = 65535                       # PROSSTT_AMD_EVALUATE_MAX_DEPTH
MAX_TILES_PER_BLOCK = 4096              # PROSSTT_AMD_EVALUATE_MAX_TILES_PER_BLOCK
MAX_VALUE = 1 << 30                     # |a_i| and |b_i| below this: every difference fits int32
OFFSETS_RANGE, DEPTH_RANGE, BRANCH_RANGE = 1, 2, 4                  # the bits of the passes' status word
STATUS_MESSAGES = (
    (OFFSETS_RANGE, "OFFSETS_RANGE", "the class offsets do not ascend from 0 to the number of cells"),
    (DEPTH_RANGE, "DEPTH_RANGE", "a depth is outside 0 .. %d" % MAX_DEPTH),
    (BRANCH_RANGE, "BRANCH_RANGE", "a branch of the second tree is outside [0, K2)"),
)


def check_status(bits):
    """ValueError naming every bit of the passes' status word that is set."""
    said = ["status bit %s (%d): %s" % (name, bit, text) for bit, name, text in STATUS_MESSAGES if bits & bit]
    if said:
        raise ValueError("; ".join(said))
    if bits:
        raise RuntimeError("the pass set an unknown status bit (status %d)" % bits)


# ---------------------------------------------------------------------------------------------------- host statistics

def _host(x):
    torch = _torch()
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _selection(mask, K):
    """The class pairs p <= q that ``mask`` selects, as a boolean (K, K) upper triangle; a pair is selected if the mask holds
    it in either order.  None: all of them."""
    if mask is None:
        return np.triu(np.ones((K, K), dtype=bool))
    m = np.asarray(mask)
    if m.dtype != np.bool_ or m.shape != (K, K):
        raise ValueError("a mask must be a boolean (%d, %d) array" % (K, K))
    return np.triu(m | m.T)


def _total(table, selection):
    """The entries of an integer or object (K, K) table that ``selection`` holds, added as a Python integer."""
    return sum(int(v) for v in np.asarray(table)[selection].tolist())


def _ratio(num, den):
    return num / den if den else float("nan")


def _over_root(num, square):
    """num / sqrt(square) for Python integers: one square root, one division; the root is exact where the integer is a
    square (equal sequences give exactly 1).  NaN where square <= 0."""
    if square <= 0:
        return float("nan")
    root = math.isqrt(square)
    return num / (root if root * root == square else math.sqrt(square))


def class_pairs(sizes):
    """The number of pairs of every pair set p <= q for the class sizes: int64 (K, K), 0 below the diagonal."""
    n = np.asarray(sizes, dtype=np.int64)
    out = np.triu(np.outer(n, n), 1)
    out[np.diag_indices(len(n))] = n * (n - 1) // 2
    return out


class Scores(NamedTuple):
    """Goodman-Kruskal's ``gamma`` and Kendall's ``tau_a`` and ``tau_b``: floats, or (K, K) arrays per class pair."""
    gamma: Any
    tau_a: Any
    tau_b: Any


class PairCounts(NamedTuple):
    """``s``, ``p``, ``a2``, ``b2`` and ``pairs``: (K, K) int64 per class pair p <= q (0 below the diagonal), by the module
    docstring's definition -- numpy arrays, or device tensors for ``out="torch"`` (``pairs`` is always a numpy array)."""
    s: Any
    p: Any
    a2: Any
    b2: Any
    pairs: np.ndarray

    def concordant(self):
        return (_host(self.p) + _host(self.s)) // 2

    def discordant(self):
        return (_host(self.p) - _host(self.s)) // 2

    def _sums(self, mask):
        sel = _selection(mask, self.pairs.shape[0])
        return tuple(_total(_host(t), sel) for t in (self.s, self.p, self.a2, self.b2, self.pairs))

    def gamma(self, mask=None):
        s, p, _, _, _ = self._sums(mask)
        return _ratio(s, p)

    def tau_a(self, mask=None):
        s, _, _, _, n = self._sums(mask)
        return _ratio(s, n)

    def tau_b(self, mask=None):
        s, _, a2, b2, _ = self._sums(mask)
        return _over_root(s, a2 * b2)

    def scores(self, mask=None):
        return Scores(self.gamma(mask), self.tau_a(mask), self.tau_b(mask))

    def per_pair(self):
        """``Scores`` of (K, K) float64 arrays: every class pair p <= q on its own, NaN below the diagonal and where a
        denominator is 0."""
        K = self.pairs.shape[0]
        out = np.full((3, K, K), np.nan)
        for p in range(K):
            for q in range(p, K):
                one = np.zeros((K, K), dtype=bool)
                one[p, q] = True
                out[:, p, q] = self.scores(one)
        return Scores(out[0], out[1], out[2])


SUMS = ("d", "d2", "dd", "d2d2", "dd2")


class PairMoments(NamedTuple):
    """The five sums of the module docstring per true class pair p <= q as (K, K) object arrays of Python integers (``d``,
    ``d2``, ``dd``, ``d2d2``, ``dd2``; 0 below the diagonal), ``pairs`` (K, K) int64, ``ticks``, and ``words`` (K, K, 5, 2): the
    (low, high) 64-bit words as the library wrote them -- a uint64 numpy array, or for ``out="torch"`` a device tensor of
    int64 bit patterns."""
    d: np.ndarray
    d2: np.ndarray
    dd: np.ndarray
    d2d2: np.ndarray
    dd2: np.ndarray
    pairs: np.ndarray
    ticks: int
    words: Any

    def pearson(self, mask=None):
        """Pearson's correlation of d and d2 over the pairs of the class pairs ``mask`` selects (None: all pairs)."""
        sel = _selection(mask, self.pairs.shape[0])
        n, sx, sy, sxx, syy, sxy = (_total(t, sel) for t in (self.pairs, self.d, self.d2, self.dd, self.d2d2, self.dd2))
        return _over_root(n * sxy - sx * sy, (n * sxx - sx * sx) * (n * syy - sy * sy))

    def mean_distances(self, mask=None):
        """(mean d, mean d2) in pseudotime units over the selected pairs."""
        sel = _selection(mask, self.pairs.shape[0])
        n, sx, sy = (_total(t, sel) for t in (self.pairs, self.d, self.d2))
        return _ratio(sx, n * self.ticks), _ratio(sy, n * self.ticks)


def moments_from_words(words, pairs, ticks):
    """``PairMoments`` of the library's (K, K, 5, 2) words."""
    w = np.ascontiguousarray(_host(words)).view(np.uint64)
    K = w.shape[0]
    tables = []
    for i in range(len(SUMS)):
        flat = [(int(hi) << 64) | int(lo) for lo, hi in w[:, :, i, :].reshape(-1, 2).tolist()]
        t = np.empty(K * K, dtype=object)
        t[:] = flat
        tables.append(t.reshape(K, K))
    return PairMoments(*tables, np.asarray(pairs, dtype=np.int64), int(ticks), words)


class Ordering(NamedTuple):
    """``counts``: the ``PairCounts`` of (true pseudotime, found pseudotime) by true branch; ``comparable_mask`` (K, K) bool:
    the branch pairs on a common root-to-tip path; ``overall``, ``comparable`` and ``within`` (the diagonal): ``Scores`` over
    those pairs; ``per_pair``: ``Scores`` of (K, K) arrays; ``spearman``; ``branch_names``: the order of the classes."""
    counts: PairCounts
    comparable_mask: np.ndarray
    overall: Scores
    comparable: Scores
    within: Scores
    per_pair: Scores
    spearman: float
    branch_names: list


class LabelScores(NamedTuple):
    """``table`` (true classes, found classes) int64 and the label values of its rows and columns; ``n`` the cells labelled
    on both sides; ``ari``, ``nmi``; ``jaccard`` and ``f1`` per true class; ``accuracy`` and ``matching`` (true label -> found
    label) of the best one-to-one matching."""
    table: np.ndarray
    true_labels: np.ndarray
    found_labels: np.ndarray
    n: int
    ari: float
    nmi: float
    jaccard: np.ndarray
    f1: np.ndarray
    accuracy: float
    matching: dict


class Evaluation(NamedTuple):
    """``labels``: ``LabelScores`` or None; ``ordering``: ``Ordering`` or None; ``distances``: ``PairMoments`` or None (without
    a second tree)."""
    labels: Optional[LabelScores]
    ordering: Optional[Ordering]
    distances: Optional[PairMoments]


def label_scores(table, true_labels=None, found_labels=None):
    """``LabelScores`` of an integer contingency table (true classes x found classes): the host half of ``labels``."""
    from scipy.optimize import linear_sum_assignment
    t = np.asarray(table)
    if t.ndim != 2 or t.dtype.kind not in "iu" or t.size == 0 or t.min() < 0 or t.sum() == 0:
        raise ValueError("a contingency table is a 2-D array of counts with at least one cell")
    t = t.astype(np.int64)
    rows, cols = t.sum(axis=1), t.sum(axis=0)
    n = int(t.sum())

    def pairs_of(v):
        return sum(int(x) * (int(x) - 1) // 2 for x in np.asarray(v).ravel().tolist())

    index, a, b, n2 = pairs_of(t), pairs_of(rows), pairs_of(cols), n * (n - 1) // 2
    den = (a + b) * n2 - 2 * a * b
    ari = 2 * (index * n2 - a * b) / den if den else 1.0

    def entropy(v):
        p = v[v > 0].astype(np.float64) / n
        return float(-(p * np.log(p)).sum())

    hu, hv = entropy(rows), entropy(cols)
    nz = t > 0
    pij = t[nz].astype(np.float64) / n
    outer = np.outer(rows, cols)[nz].astype(np.float64) / (float(n) * float(n))
    mi = float((pij * (np.log(pij) - np.log(outer))).sum())
    if (rows > 0).sum() == 1 and (cols > 0).sum() == 1:
        nmi = 1.0
    else:
        nmi = _ratio(max(mi, 0.0), (hu + hv) / 2.0) if hu + hv > 0 else 1.0
    with np.errstate(invalid="ignore", divide="ignore"):
        tf = t.astype(np.float64)
        jaccard = np.nanmax(np.where(t > 0, tf / (rows[:, None] + cols[None, :] - t), 0.0), axis=1)
        f1 = np.nanmax(np.where(t > 0, 2.0 * tf / (rows[:, None] + cols[None, :]), 0.0), axis=1)
    ri, ci = linear_sum_assignment(t, maximize=True)
    tl = np.arange(t.shape[0]) if true_labels is None else np.asarray(true_labels)
    fl = np.arange(t.shape[1]) if found_labels is None else np.asarray(found_labels)
    matching = {tl[r].item(): fl[c].item() for r, c in zip(ri, ci)}
    return LabelScores(t, tl, fl, n, ari, nmi, jaccard, f1, int(t[ri, ci].sum()) / n, matching)


# ------------------------------------------------------------------------------------------------- argument checks

def _integer(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("need an integer %d <= %s <= %d (got %r)" % (lo, name, hi, v))
    return int(v)


def _out(out):
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")


def _vector(name, x, kinds="iu"):
    """``x`` as a 1-D host array or device tensor of an accepted kind ("i", "u", "f"), and whether it lies on a device."""
    torch = _torch()
    if isinstance(x, torch.Tensor):
        if x.device.type == "cpu":
            x = x.detach().numpy()
        else:
            kind = "f" if x.dtype.is_floating_point else ("b" if x.dtype == torch.bool else "i")
            if kind not in kinds or x.dtype.is_complex or x.dim() != 1:
                raise ValueError("%s must be a 1-D array of %s" % (name, "integers" if kinds == "iu" else "numbers"))
            return x.detach(), True
    try:
        arr = np.asarray(x)
    except Exception:
        raise ValueError("%s must be a 1-D array" % name) from None
    if arr.ndim != 1 or arr.dtype.kind not in kinds:
        raise ValueError("%s must be a 1-D array of %s" % (name, "integers" if kinds == "iu" else "numbers"))
    return _signed(name, arr), False


def _signed(name, arr):
    """A host integer vector as int64, the form in which every one of them travels (torch holds the unsigned kinds only in
    part); other kinds as they are.  ValueError for a value of 2^63 or more."""
    if arr.dtype.kind not in "iu":
        return arr
    if arr.dtype.kind == "u" and arr.size and int(arr.max()) >= 1 << 63:
        raise ValueError("%s: a value is 2^63 or more" % name)
    return arr.astype(np.int64)


def _cells(n):
    if n < 2 or n >= 1 << 31:
        raise ValueError("need 2 <= cells < 2^31 (got %d)" % n)
    return n


def _check_range(name, arr, on_device, lo, hi, what):
    """ValueError unless lo <= arr <= hi everywhere (a device tensor is asked on the device)."""
    if on_device:
        ok = bool(((arr >= lo) & (arr <= hi)).all())
    else:
        ok = bool(arr.min() >= lo and arr.max() <= hi)
    if not ok:
        raise ValueError("%s: %s" % (name, what))


def _place(arrays, dev=None):
    """The vectors as contiguous device tensors on one device."""
    torch = _torch()
    out = []
    for arr in arrays:
        if isinstance(arr, np.ndarray):
            t = torch.from_numpy(np.array(arr)).to(dev or torch.device("cuda", torch.cuda.current_device()))
        else:
            t = arr.contiguous()
        dev = dev or t.device
        if t.device != dev:
            raise ValueError("the arguments lie on different devices")
        out.append(t)
    return out


def _first_device(arrays):
    for arr in arrays:
        if not isinstance(arr, np.ndarray):
            return arr.device
    return None


# ------------------------------------------------------------------------------------------------------ device steps

def _sorted_by_class(classes, K):
    """(order, offsets, sizes as a host array) of int64 device class codes: the stable sort by class."""
    torch = _torch()
    order = torch.sort(classes, stable=True).indices
    sizes = torch.bincount(classes, minlength=K)
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=classes.device)
    offsets[1:] = torch.cumsum(sizes, 0)
    return order, offsets, sizes.cpu().numpy()


def _run_counts(L, a, b, offsets, K, tiles_per_block):
    """((K, K, 4) int64 device tensor, status) of sorted contiguous int32 device sequences."""
    torch = _torch()
    N, dev = a.numel(), a.device
    ws = device.workspace("evaluate", "prosstt_amd_evaluate_workspace_bytes", dev, N, K, tiles_per_block)
    counts = torch.empty((K, K, 4), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.check(L.prosstt_amd_evaluate_pair_counts(device.current_stream(dev), _ptr(a), _ptr(b), _ptr(offsets), N, K,
                                                     tiles_per_block, _ptr(ws), ws.numel(), _ptr(counts), _ptr(status)),
                  "evaluate")
    return counts, int(status.item())


def _run_moments(L, h, h2, c2, offsets, J, J2, K, K2, tiles_per_block):
    """((K, K, 5, 2) int64 device tensor of words, status)."""
    torch = _torch()
    N, dev = h.numel(), h.device
    ws = device.workspace("evaluate", "prosstt_amd_evaluate_workspace_bytes", dev, N, K, tiles_per_block)
    words = torch.empty((K, K, 5, 2), dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.check(L.prosstt_amd_evaluate_pair_moments(device.current_stream(dev), _ptr(h), _ptr(h2), _ptr(c2), _ptr(offsets),
                                                      _ptr(J), _ptr(J2), N, K, K2, tiles_per_block, _ptr(ws), ws.numel(),
                                                      _ptr(words), _ptr(status)), "evaluate")
    return words, int(status.item())


def _dense_ranks(t):
    """The dense ranks of a device vector (equal values get equal ranks, the smallest 0): int64."""
    return _torch().unique(t, sorted=True, return_inverse=True)[1]


def _exact_dot(x, y):
    """sum x_i y_i of int64 device vectors with |x_i|, |y_i| < 2^31, as a Python integer: 16-bit halves, so that each of
    the four int64 sums is exact for fewer than 2^31 terms."""
    xh, xl, yh, yl = x >> 16, x & 0xFFFF, y >> 16, y & 0xFFFF
    hh, hl, lh, ll = (int((u * v).sum().item()) for u, v in ((xh, yh), (xh, yl), (xl, yh), (xl, yl)))
    return (hh << 32) + ((hl + lh) << 16) + ll


def _spearman(ra, rb):
    """Spearman's correlation from the dense ranks of two device vectors: the centred doubled midranks 2 mid - (N + 1) are
    integers that sum to 0, so r = Sxy / sqrt(Sxx Syy) with exact integer sums."""
    torch = _torch()
    N = ra.numel()

    def centred(r):
        counts = torch.bincount(r)
        ends = torch.cumsum(counts, 0)
        return (2 * ends - counts + 1 - (N + 1))[r]

    x, y = centred(ra), centred(rb)
    return _over_root(_exact_dot(x, y), _exact_dot(x, x) * _exact_dot(y, y))


# -------------------------------------------------------------------------------------------------------- entry points

def pair_counts(a, b, classes, K=None, *, tiles_per_block=0, out="numpy"):
    """``PairCounts`` of two integer sequences over the cells and the class of every cell (the module docstring's definition).

    ``a``, ``b``: (N,) integers below 2^30 in size, ``classes``: (N,) integers in [0, K) -- host arrays (copied to the current
    device) or device tensors (used where they lie, on the current stream); 2 <= N < 2^31.  ``K``: 1 .. 64 classes (None: the
    largest class + 1).  ``tiles_per_block``: 1 .. 4096 column tiles of 256 cells per block, or 0 for the library's choice; the
    result does not depend on it.  ``out``: "numpy", or "torch" for device tensors.

    Raises ValueError for wrong kinds, shapes and sizes, a value or class out of range and a bad ``K``,
    ``tiles_per_block`` or ``out``: before any device use for host arrays, from a check on the device for device tensors."""
    _out(out)
    tiles_per_block = _integer("tiles_per_block", tiles_per_block, 0, MAX_TILES_PER_BLOCK)
    vectors = [_vector(name, x) for name, x in (("a", a), ("b", b), ("classes", classes))]
    N = _cells(int(vectors[0][0].shape[0]))
    if any(int(v.shape[0]) != N for v, _ in vectors):
        raise ValueError("a, b and classes differ in length")
    if K is not None:
        K = _integer("K", K, 1, MAX_CLASSES)
    for (arr, on_device), (name, lo, hi, what) in zip(vectors, (
            ("a", -MAX_VALUE + 1, MAX_VALUE - 1, "a value is 2^30 or more in size"),
            ("b", -MAX_VALUE + 1, MAX_VALUE - 1, "a value is 2^30 or more in size"),
            ("classes", 0, (MAX_CLASSES if K is None else K) - 1, "a class lies outside [0, K)"))):
        if not on_device:
            _check_range(name, arr, False, lo, hi, what)
    L = device.need_device("evaluate")
    torch = _torch()
    arrays = _place([v for v, _ in vectors], _first_device([v for v, _ in vectors]))
    with torch.cuda.device(arrays[0].device):
        for (_, on_device), t, name in zip(vectors, arrays, ("a", "b", "classes")):
            if on_device and name != "classes":
                _check_range(name, t, True, -MAX_VALUE + 1, MAX_VALUE - 1, "a value is 2^30 or more in size")
        cls = arrays[2].to(torch.int64)
        if vectors[2][1]:
            _check_range("classes", cls, True, 0, (MAX_CLASSES if K is None else K) - 1, "a class lies outside [0, K)")
        if K is None:
            K = int(cls.max().item()) + 1
        order, offsets, sizes = _sorted_by_class(cls, K)
        sa, sb = (t[order].to(torch.int32).contiguous() for t in arrays[:2])
        counts, bits = _run_counts(L, sa, sb, offsets, K, tiles_per_block)
        check_status(bits)
        # (4, K, K): each field a contiguous table (a fresh tensor: ``contiguous()`` keeps the strides of a (1, 1, 4) view)
        tables = torch.empty((4, K, K), dtype=torch.int64, device=counts.device)
        tables.copy_(counts.permute(2, 0, 1))
        if out == "numpy":
            tables = tables.cpu().numpy()
        fields = [tables[i] for i in range(4)]
        return PairCounts(*fields, class_pairs(sizes))


def tree_moments(h, classes, J, h2, c2, J2, *, ticks=1, tiles_per_block=0, out="numpy"):
    """``PairMoments`` of the cells' depths and branches on two trees, as arrays (the module docstring's definition).

    ``h``, ``classes``: (N,) depth in 0 .. 65 535 and true branch in [0, K) of every cell; ``J``: the (K, K) junction table of
    the true tree; ``h2``, ``c2``, ``J2`` (K2, K2): the same for the second tree; K, K2 <= 64.  Host arrays or device tensors
    for the vectors, host arrays for the tables.  ``ticks`` is recorded in the result.  ``tiles_per_block``, ``out``: as in
    ``pair_counts``.

    Raises ValueError as ``pair_counts`` does, and for a table that is not square, symmetric and of integers."""
    _out(out)
    tiles_per_block = _integer("tiles_per_block", tiles_per_block, 0, MAX_TILES_PER_BLOCK)
    ticks = _integer("ticks", ticks, 1, MAX_DEPTH)
    tables = []
    for name, table in (("J", J), ("J2", J2)):
        t = np.asarray(table)
        if t.ndim != 2 or t.shape[0] != t.shape[1] or t.dtype.kind not in "iu" or not 1 <= t.shape[0] <= MAX_CLASSES:
            raise ValueError("%s must be a square integer table of 1 to %d branches" % (name, MAX_CLASSES))
        if not np.array_equal(t, t.T):
            raise ValueError("%s must be symmetric" % name)
        tables.append(np.clip(t, 0, MAX_DEPTH).astype(np.int32))
    K, K2 = tables[0].shape[0], tables[1].shape[0]
    names = ("h", "classes", "h2", "c2")
    vectors = [_vector(name, x) for name, x in zip(names, (h, classes, h2, c2))]
    N = _cells(int(vectors[0][0].shape[0]))
    if any(int(v.shape[0]) != N for v, _ in vectors):
        raise ValueError("h, classes, h2 and c2 differ in length")
    bounds = ((0, MAX_DEPTH, "a depth is outside 0 .. %d" % MAX_DEPTH), (0, K - 1, "a class lies outside [0, K)"),
              (0, MAX_DEPTH, "a depth is outside 0 .. %d" % MAX_DEPTH), (0, K2 - 1, "a branch lies outside [0, K2)"))
    for (arr, on_device), name, (lo, hi, what) in zip(vectors, names, bounds):
        if not on_device:
            _check_range(name, arr, False, lo, hi, what)
    L = device.need_device("evaluate")
    torch = _torch()
    arrays = _place([v for v, _ in vectors], _first_device([v for v, _ in vectors]))
    dev = arrays[0].device
    with torch.cuda.device(dev):
        cls = arrays[1].to(torch.int64)
        if vectors[1][1]:
            _check_range("classes", cls, True, 0, K - 1, "a class lies outside [0, K)")
        order, offsets, sizes = _sorted_by_class(cls, K)
        # (device depths and branches are clamped into int32 for the pass, which reports what is out of range)
        sh, sh2, sc2 = (t[order].clamp(-1, MAX_DEPTH + 1).to(torch.int32).contiguous() for t in (arrays[0], arrays[2], arrays[3]))
        Jd, J2d = (torch.from_numpy(t).to(dev) for t in tables)
        words, bits = _run_moments(L, sh, sh2, sc2, offsets, Jd, J2d, K, K2, tiles_per_block)
        check_status(bits)
        return moments_from_words(words if out == "torch" else words.cpu().numpy().view(np.uint64), class_pairs(sizes), ticks)


def _depths(nodes, pseudotime, branches, ticks, what):
    """(depths int32, branch codes int64, the junction table int32) of cells on a tree, host arrays; ValueError otherwise."""
    t = _host(pseudotime)
    if t.ndim != 1 or t.dtype.kind not in "iuf":
        raise ValueError("%s: pseudotime must be a 1-D array of numbers" % what)
    t = t.astype(np.float64)
    if not np.all(np.isfinite(t)):
        raise ValueError("%s: a pseudotime value is not finite" % what)
    codes = nodes.codes(_host(branches), t.shape[0])
    origin = float(nodes.first.min())
    h = np.rint((t - origin) * ticks)
    if h.min() < 0 or h.max() > MAX_DEPTH:
        raise ValueError("%s: a depth rint((t - %g) * %d) lies outside 0 .. %d: lower ticks" % (what, origin, ticks, MAX_DEPTH))
    B = len(nodes.names)
    if B > MAX_CLASSES:
        raise ValueError("%s: %d branches, more than %d" % (what, B, MAX_CLASSES))
    J = np.full((B, B), MAX_DEPTH, dtype=np.int32)
    for p in range(B):
        for q in range(B):
            e = nodes.junction(p, q)
            if e is not None:
                J[p, q] = min(int(np.rint((e - origin) * ticks)), MAX_DEPTH)
    return h.astype(np.int32), codes, J


def pair_moments(tree, pt, br, tree2, pt2, br2, *, ticks=16, tiles_per_block=0, out="numpy"):
    """``PairMoments`` of the geodesic distances of all pairs of cells on the true tree and on a second tree.

    ``tree``, ``pt``, ``br``: the simulation's ``Tree`` and the absolute pseudotime and branch label of every cell;
    ``tree2``, ``pt2``, ``br2``: the same of the second tree (an inferred one: ``LineageFit.tree``, ``.position`` or
    ``.pseudotime``, ``.branches``); each tree has at most 64 branches.  ``ticks``: depth steps per unit of pseudotime, 1 ..
    65 535: positions are rounded to 1 / ticks, and the deepest cell times ``ticks`` must stay within 65 535.

    Raises ValueError, before any device use, for labels that are no branch of their tree, pseudotimes that are not finite
    numbers, one per cell, or too deep for ``ticks``, and a bad ``ticks``, ``tiles_per_block`` or ``out``."""
    _out(out)
    ticks = _integer("ticks", ticks, 1, MAX_DEPTH)
    h, codes, J = _depths(_Nodes(tree), pt, br, ticks, "the true tree")
    h2, codes2, J2 = _depths(_Nodes(tree2), pt2, br2, ticks, "the second tree")
    if h.shape[0] != h2.shape[0]:
        raise ValueError("the two trees hold %d and %d cells" % (h.shape[0], h2.shape[0]))
    return tree_moments(h, codes, J, h2, codes2, J2, ticks=ticks, tiles_per_block=tiles_per_block, out=out)


def ordering(tree, pt, br, pseudotime, *, tiles_per_block=0):
    """``Ordering`` of a found pseudotime against the true one, by true branch.

    ``tree``, ``pt``, ``br``: as in ``pair_moments``; ``pseudotime``: (N,) finite numbers, a host array or a device tensor.
    Both are ranked densely (the signs of their differences are those of the ranks), and ``pair_counts`` runs with a = the
    true rank, b = the found rank and classes = the true branch.

    Raises ValueError, before any device use, for a bad tree, label or pseudotime."""
    nodes = _Nodes(tree)
    true_t = _host(pt)
    if true_t.ndim != 1 or true_t.dtype.kind not in "iuf" or not np.all(np.isfinite(true_t.astype(np.float64))):
        raise ValueError("pt must be a 1-D array of finite numbers")
    true_t = _signed("pt", true_t)
    codes = nodes.codes(_host(br), true_t.shape[0])
    N = _cells(int(true_t.shape[0]))
    B = len(nodes.names)
    if B > MAX_CLASSES:
        raise ValueError("%d branches, more than %d" % (B, MAX_CLASSES))
    found, on_device = _vector("pseudotime", pseudotime, "iuf")
    if int(found.shape[0]) != N:
        raise ValueError("need one pseudotime per cell: %d, not %d" % (N, int(found.shape[0])))
    if not on_device and not np.all(np.isfinite(found.astype(np.float64))):
        raise ValueError("a pseudotime value is not finite")
    device.need_device("evaluate")
    torch = _torch()
    dev = found.device if on_device else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        found_d, true_d, cls = _place([found, true_t, codes], dev)
        if on_device and found_d.dtype.is_floating_point and not bool(torch.isfinite(found_d).all()):
            raise ValueError("a pseudotime value is not finite")
        ra, rb = _dense_ranks(true_d), _dense_ranks(found_d)
        counts = pair_counts(ra, rb, cls, B, tiles_per_block=tiles_per_block)
        rho = _spearman(ra, rb)
    comparable = np.array([[nodes.junction(p, q) is None for q in range(B)] for p in range(B)], dtype=bool)
    return Ordering(counts, comparable, counts.scores(), counts.scores(comparable), counts.scores(np.eye(B, dtype=bool)),
                    counts.per_pair(), rho, list(nodes.names))


def _encode(name, x):
    """(codes int64 with -1 for "no label", the label values, on a device?) of a label vector."""
    torch = _torch()
    if isinstance(x, torch.Tensor) and x.device.type != "cpu":
        if x.dim() != 1 or x.dtype.is_floating_point or x.dtype.is_complex:
            raise ValueError("%s must be a 1-D array of integer or string labels" % name)
        x = x.detach().to(torch.int64)
        values, inverse = torch.unique(x, sorted=True, return_inverse=True)
        keep = values >= 0
        first = int((~keep).sum().item())                  # (the negative values come first)
        return torch.where(x >= 0, inverse - first, -1), values[keep].cpu().numpy(), True
    arr = _host(x)
    if arr.ndim != 1 or arr.dtype.kind not in "iuUSO":
        raise ValueError("%s must be a 1-D array of integer or string labels" % name)
    labelled = arr >= 0 if arr.dtype.kind in "iu" else np.ones(arr.shape[0], dtype=bool)
    values, inverse = np.unique(arr[labelled], return_inverse=True)
    codes = np.full(arr.shape[0], -1, dtype=np.int64)
    codes[labelled] = inverse
    return codes, values, False


def labels(true, found):
    """``LabelScores`` of the found labels against the true ones (the module docstring's definition).

    ``true``, ``found``: (N,) integer or string labels, host arrays or (integers) device tensors; a negative integer means
    "no label" and leaves the cell out.  The labels are encoded by ``unique`` and the table is a ``bincount`` on the device.

    Raises ValueError for other kinds or shapes, differing lengths, and when no cell is labelled on both sides."""
    t_codes, t_values, _ = _encode("true", true)
    f_codes, f_values, _ = _encode("found", found)
    if int(t_codes.shape[0]) != int(f_codes.shape[0]):
        raise ValueError("true and found differ in length")
    if len(t_values) == 0 or len(f_values) == 0:
        raise ValueError("no cell is labelled on both sides")
    device.need_device("evaluate")
    torch = _torch()
    dev = _first_device([t_codes, f_codes])
    t_d, f_d = _place([t_codes, f_codes], dev)
    with torch.cuda.device(t_d.device):
        both = (t_d >= 0) & (f_d >= 0)
        Kt, Kf = len(t_values), len(f_values)
        table = torch.bincount((t_d * Kf + f_d)[both], minlength=Kt * Kf).reshape(Kt, Kf).cpu().numpy()
    if table.sum() == 0:
        raise ValueError("no cell is labelled on both sides")
    return label_scores(table, t_values, f_values)


def trajectory(tree, pt, br, found, *, ticks=16):
    """``Evaluation`` of a found trajectory against the simulation's ``tree``, ``pt`` and ``br``.

    ``found``: a ``ptree.LineageFit`` (labels, ordering of its ``position``, distances on its tree); a ``dpt.DPT`` (ordering;
    labels of its ``groups`` when it has them, 0 = the branching region included as a label); a ``mapping.CellMapping``
    (labels and ordering); or a tuple (branches or None, pseudotime or None[, tree]) -- what is missing is None in the
    result, and ``distances`` needs all three.

    Raises ValueError for anything else, and what ``labels``, ``ordering`` and ``pair_moments`` raise."""
    from . import dpt as _dpt, mapping as _mapping, ptree as _ptree
    if isinstance(found, _ptree.LineageFit):
        parts = (found.branches, found.position, found.tree)
    elif isinstance(found, _dpt.DPT):
        parts = (found.groups, found.pseudotime, None)
    elif isinstance(found, _mapping.CellMapping):
        parts = (found.branches, found.pseudotime, None)
    elif isinstance(found, tuple) and len(found) in (2, 3):
        parts = tuple(found) + (None,) * (3 - len(found))
    else:
        raise ValueError("found must be a LineageFit, a DPT, a CellMapping or a (branches, pseudotime[, tree]) tuple")
    branches, pseudotime, tree2 = parts
    return Evaluation(None if branches is None else labels(br, branches),
                      None if pseudotime is None else ordering(tree, pt, br, pseudotime),
                      None if tree2 is None or branches is None or pseudotime is None
                      else pair_moments(tree, pt, br, tree2, pseudotime, branches, ticks=ticks))
