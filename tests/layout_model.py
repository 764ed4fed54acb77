"""The model of prosstt_amd.layout (include/prosstt_amd_layout.h's definition) in numpy: one epoch in binary64 from binary32
positions, the hash of the negative samples, the spectral start from dense eigh, and a trustworthiness score.  A helper:
nothing here is collected."""
import collections
import functools

import numpy as np

import graph_model

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
A, B = 0.5830300, 1.3341670            # find_ab_params(1.0, 0.5), the published values


def mix(x):
    """The definition's mix of uint64 arrays (arithmetic modulo 2^64)."""
    x = np.array(x, dtype=np.uint64, ndmin=1)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return x


def negatives(seed, epoch, e, s, N):
    """k of the definition for arrays (or scalars) of CSR positions ``e`` and samples ``s``: int64."""
    base = mix(np.array([seed], dtype=np.uint64) + GOLDEN * np.array([epoch + 1], dtype=np.uint64))[0]
    e, s = np.broadcast_arrays(np.asarray(e, dtype=np.uint64), np.asarray(s, dtype=np.uint64))
    h = mix(base ^ (np.uint64(32) * e + s))
    return (((h >> np.uint64(32)) * np.uint64(N)) >> np.uint64(32)).astype(np.int64).reshape(e.shape)


def weights(W):
    """p of the definition for every CSR position of the scipy matrix W."""
    return W.data / W.data.max()


def active(p, n):
    return np.floor((n + 1.0) * p) > np.floor(float(n) * p)


def _coefficients(d2, a, b, gamma, attract):
    out = np.zeros_like(d2)
    pos = d2 > 0
    x = d2[pos]
    if attract:
        out[pos] = -2.0 * a * b * x ** (b - 1.0) / (a * x ** b + 1.0)
    else:
        out[pos] = 2.0 * gamma * b / ((0.001 + x) * (a * x ** b + 1.0))
    return out


# Y: the unrounded new positions (N, c); S: sum |term| per row and coordinate (N, c); L: the number of terms per row (N,);
# own: the negative samples that hit their own row (no term); coincident: the pairs at distance 0 (a term of 0)
Epoch = collections.namedtuple("Epoch", "Y S L own coincident")


def epoch(W, Y, n, n_epochs, a=A, b=B, gamma=1.0, alpha0=1.0, rate=5, seed=0):
    """One epoch of the definition in binary64 from the binary32 positions ``Y`` (N, c) on the scipy CSR matrix ``W``: an
    ``Epoch``."""
    assert Y.dtype == np.float32
    a, b, gamma = (float(np.float32(v)) for v in (a, b, gamma))           # the kernel rounds them once
    alpha = float(np.float32(alpha0 * (1.0 - n / n_epochs)))
    y = Y.astype(np.float64)
    N, c = y.shape
    indptr, indices = W.indptr.astype(np.int64), W.indices.astype(np.int64)
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(indptr))
    e = np.flatnonzero(active(weights(W), n))
    i, j = rows[e], indices[e]
    total, S, L = np.zeros((N, c)), np.zeros((N, c)), np.zeros(N, dtype=np.int64)

    coincident = [0]

    def add(i, other, attract):
        delta = y[i] - y[other]
        d2 = np.sum(delta * delta, axis=1)
        coincident[0] += int(np.sum(d2 == 0))
        coef = _coefficients(d2, a, b, gamma, attract)
        term = (2.0 if attract else 1.0) * np.clip(coef[:, None] * delta, -4.0, 4.0)
        for col in range(c):                                             # (bincount adds in entry order, in binary64)
            total[:, col] += np.bincount(i, weights=term[:, col], minlength=N)
            S[:, col] += np.bincount(i, weights=np.abs(term[:, col]), minlength=N)
        L[:] += np.bincount(i, minlength=N)

    add(i, j, True)
    own = 0
    if rate:
        k = negatives(seed, n, e[:, None], np.arange(rate)[None, :], N)
        ii = np.repeat(i, rate)
        k = k.ravel()
        keep = k != ii
        own = int(np.sum(~keep))
        add(ii[keep], k[keep], False)
    return Epoch(y + alpha * total, S, L, own, coincident[0])


def run(W, start, n_epochs, **kw):
    """``n_epochs`` epochs from ``start``, rounding to binary32 after each, as the device does."""
    Y = np.asarray(start, dtype=np.float32)
    for n in range(n_epochs):
        Y = epoch(W, Y, n, n_epochs, **kw)[0].astype(np.float32)
    return Y


def spectral_vectors(W, c):
    """(eigenvalues, unit eigenvectors with graph's sign rule) of components 1 .. c of S = D^(-1/2) W D^(-1/2), dense."""
    q = np.asarray(W.sum(axis=1)).ravel()
    dense = W.toarray() / np.sqrt(q[:, None] * q[None, :])
    lam, vec = np.linalg.eigh(dense)
    order = np.argsort(-lam, kind="stable")[:c + 1]
    return lam[order][1:], graph_model.fix_signs(vec[:, order])[:, 1:]


def scale_start(vectors, seed):
    """The definition's scaling of the spectral start, written out once more."""
    x = vectors * (10.0 / np.abs(vectors).max()) + 1e-4 * np.random.default_rng(seed).standard_normal(vectors.shape)
    out = np.empty_like(x)
    for col in range(x.shape[1]):
        lo, hi = x[:, col].min(), x[:, col].max()
        out[:, col] = 10.0 * (x[:, col] - lo) / (hi - lo)
    return out.astype(np.float32)


def spectral_start(W, c, seed=0):
    return scale_start(spectral_vectors(W, c)[1], seed)


def _ranks(D):
    """rank[i, j] = the position of j among the others ordered by distance from i (1 = nearest; the row itself 0)."""
    D = D.copy()
    np.fill_diagonal(D, -1.0)
    order = np.argsort(D, axis=1, kind="stable")
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(D.shape[1]), D.shape), axis=1)
    return order, ranks


def _distances(X):
    X = np.asarray(X, dtype=np.float64)
    sq = np.sum(X * X, axis=1)
    return np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2.0 * (X @ X.T), 0.0))


def trustworthiness(X, Y, k):
    """1 - 2 / (N k (2 N - 3 k - 1)) sum_i sum_{j in the k nearest of i in Y} max(0, rank_X(i, j) - k)   (Venna and Kaski;
    scikit-learn's ``manifold.trustworthiness`` with the Euclidean metric)."""
    N = len(X)
    _, ranks_x = _ranks(_distances(X))
    order_y, _ = _ranks(_distances(Y))
    near = order_y[:, 1:k + 1]
    excess = np.maximum(np.take_along_axis(ranks_x, near, axis=1) - k, 0)
    return 1.0 - excess.sum() * 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0))


@functools.lru_cache(maxsize=None)
def reference_run(N, k, n_epochs, init, seed=0):
    """(start, result) of the model's whole run on graph_model.case(N, k): shared and read-only."""
    W = graph_model.case(N, k)["W"]
    if init == "spectral":
        start = spectral_start(W, 2, seed)
    else:
        start = np.random.default_rng(seed).uniform(-10, 10, (N, 2)).astype(np.float32)
    out = run(W, start, n_epochs, seed=seed)
    for arr in (start, out):
        arr.setflags(write=False)
    return start, out
