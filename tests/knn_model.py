"""The scalar model of neighbors.knn (include/prosstt_amd_knn.h's definition) in numpy, a binary64 brute force to hold
it against, and the inputs the knn tests share.  A helper: nothing here is collected."""
import numpy as np


def model(P, k):
    """(indices int32 (N, k), sq_distances float32 (N, k)) of a float32 (N, d) panel: d2 by a separate float32 subtract,
    multiply and add per coordinate in ascending order; the k smallest keys (bits(d2) << 32 | j), self excluded."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    N, d = P.shape
    acc = np.zeros((N, N), np.float32)
    for c in range(d):
        t = P[:, None, c] - P[None, :, c]
        acc += t * t                                             # float32 throughout
    key = (acc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    key[np.arange(N), np.arange(N)] = np.uint64(2 ** 64 - 1)     # self
    order = np.argsort(key, axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(acc, order, axis=1)


def brute64(P, k):
    """The same neighbours from binary64 distances of the float32 panel (ties to the lower index): (indices, d2)."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    N = P.shape[0]
    d2 = np.zeros((N, N), np.float64)
    for c in range(P.shape[1]):
        d2 += (P[:, None, c] - P[None, :, c]) ** 2
    d2[np.arange(N), np.arange(N)] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(d2, order, axis=1)


def no_subnormal_terms(P):
    """True if every non-zero |P| is at least 2^-36: a non-zero difference of two such float32 values is a multiple of
    2^-59, so every non-zero |t_c| is above 2^-60 and no term t_c^2 is subnormal."""
    a = np.abs(np.asarray(P, dtype=np.float32))
    return bool(np.all((a == 0) | (a >= 2.0 ** -36)))


def gaussian(N, d, seed):
    return np.random.default_rng(seed).standard_normal((N, d)).astype(np.float32)


def scaled(N, d, seed):
    """Gaussian columns scaled by 10^(-3 .. 3): small terms added to large accumulators."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** rng.integers(-3, 4, size=d)
    return (rng.standard_normal((N, d)) * scale[None, :]).astype(np.float32)


def lattice(N, seed, d=4):
    """Points of {0, 1, 2}^d: most rows have exact ties across any k-th place."""
    return np.random.default_rng(seed).integers(0, 3, size=(N, d)).astype(np.float32)


def duplicates(d, seed, distinct=40, copies=30):
    """``distinct`` Gaussian points each repeated ``copies`` times, shuffled: whole rows of zero distances."""
    rng = np.random.default_rng(seed)
    P = np.repeat(rng.standard_normal((distinct, d)).astype(np.float32), copies, axis=0)
    return P[rng.permutation(P.shape[0])]


KINDS = {"gaussian": gaussian, "scaled": scaled,
         "lattice": lambda N, d, seed: lattice(N, seed, d),
         "duplicates": lambda N, d, seed: duplicates(d, seed, distinct=N // 30),
         "copies100": lambda N, d, seed: duplicates(d, seed, distinct=N // 100, copies=100)}


def tie_spans(P, k, seg=1024):
    """(crosses, cut), two bool (N,) arrays, of the keys equal to T, the k-th smallest d2 of a row (self excluded), when
    the row is walked in segments of ``seg`` consecutive candidates.  With need = k - (keys below T): crosses is True where
    some segment after the first starts with 0 < (equal keys met so far) < need, so that the equal keys taken come from a
    later segment after an earlier one supplied some but not all of them; cut is True where there are more keys equal to
    T than need, so that which of them are taken decides the result."""
    P = np.ascontiguousarray(P, dtype=np.float32)
    N, d = P.shape
    acc = np.zeros((N, N), np.float32)
    for c in range(d):
        t = P[:, None, c] - P[None, :, c]
        acc += t * t
    bits = acc.view(np.uint32).astype(np.int64)
    bits[np.arange(N), np.arange(N)] = np.int64(1) << 40         # self: above every key
    T = np.partition(bits, k - 1, axis=1)[:, k - 1]
    need = k - (bits < T[:, None]).sum(axis=1)
    equal = bits == T[:, None]
    cut = equal.sum(axis=1) > need
    starts = np.arange(seg, N, seg)
    if starts.size == 0:
        return np.zeros(N, bool), cut
    so_far = np.cumsum(equal, axis=1)[:, starts - 1]             # equal keys before each later segment's start
    crosses = np.any((so_far > 0) & (so_far < need[:, None]), axis=1)
    return crosses, cut
