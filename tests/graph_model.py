"""The binary64 model of prosstt_amd.graph (include/prosstt_amd_graph.h's definitions) in numpy and scipy, and the inputs the
graph tests share.  A helper: nothing here is collected."""
import functools

import numpy as np
import scipy.sparse as sparse

import knn_model

BISECTIONS = 64


def tree_points(N, d, seed):
    """A noisy Y in d dimensions, float32 (N, d): three arms of length 10 from the origin, Gaussian noise of 0.3."""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((3, d))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs[0] = -dirs[0]
    b = rng.integers(0, 3, N)
    t = rng.random(N)
    return np.float32(10 * t[:, None] * dirs[b] + 0.3 * rng.standard_normal((N, d)))


def memberships(sq_distances):
    """(a (N, k), rho (N,), sigma (N,)) of float32 squared distances."""
    d = np.sqrt(np.asarray(sq_distances, dtype=np.float32).astype(np.float64))
    N, k = d.shape
    rho = np.where(d > 0, d, np.inf).min(axis=1)
    rho[np.isinf(rho)] = 0.0
    g = np.maximum(d - rho[:, None], 0.0)
    target = np.log2(k + 1)
    lo, hi, mid = np.zeros(N), np.full(N, np.inf), np.ones(N)
    for _ in range(BISECTIONS):
        above = np.exp(-g / mid[:, None]).sum(axis=1) > target
        hi = np.where(above, mid, hi)
        lo = np.where(above, lo, mid)
        with np.errstate(invalid="ignore"):
            mid = np.where(~above & np.isinf(hi), 2 * mid, (lo + hi) / 2)
    sigma = np.maximum(mid, 1e-3 * d.mean(axis=1))
    a = np.where(g == 0, 1.0, np.exp(-g / sigma[:, None]))
    return a, rho, sigma


def f_of_sigma(sq_distances, rho, sigma):
    d = np.sqrt(np.asarray(sq_distances, dtype=np.float32).astype(np.float64))
    return np.exp(-np.maximum(d - rho[:, None], 0.0) / sigma[:, None]).sum(axis=1)


def connectivities(indices, sq_distances):
    """(W as a scipy CSR matrix, columns ascending within a row; rho; sigma)."""
    indices = np.asarray(indices)
    N, k = indices.shape
    a, rho, sigma = memberships(sq_distances)
    i = np.repeat(np.arange(N, dtype=np.int64), k)
    j = indices.ravel().astype(np.int64)
    keys = np.concatenate([(i << 32) | j, (j << 32) | i])
    vals = np.concatenate([a.ravel(), a.ravel()])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    head = np.r_[True, keys[1:] != keys[:-1]]
    assert not np.any(~head[1:] & ~head[:-1]), "more than two entries of one key: a row lists a cell twice"
    slot = np.cumsum(head) - 1
    data = vals[head]
    second = np.flatnonzero(~head)
    data[slot[second]] = (data[slot[second]] + vals[second]) - data[slot[second]] * vals[second]
    rows = keys[head] >> 32
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    W = sparse.csr_matrix((data, (keys[head] & 0xFFFFFFFF).astype(np.int32), indptr), shape=(N, N))
    W.has_sorted_indices = True
    return W, rho, sigma


def transitions(W):
    """(T as a scipy CSR matrix of W's sparsity, q, z)."""
    rows = np.repeat(np.arange(W.shape[0]), np.diff(W.indptr))
    q = np.asarray(W.sum(axis=1)).ravel()
    K = W.copy()
    K.data = W.data / (q[rows] * q[W.indices])
    z = np.sqrt(np.asarray(K.sum(axis=1)).ravel())
    T = K.copy()
    T.data = K.data / (z[rows] * z[W.indices])
    return T, q, z


def fix_signs(vectors):
    """Columns flipped so that the entry of largest magnitude (the lowest index among equals) is positive."""
    first = np.argmax(np.abs(vectors), axis=0)
    return vectors * np.where(vectors[first, np.arange(vectors.shape[1])] < 0, -1.0, 1.0)


def dense_spectrum(T):
    """(every eigenvalue of T ordered by descending magnitude, its eigenvectors) from dense eigh."""
    lam, vec = np.linalg.eigh(T.toarray())
    order = np.argsort(-np.abs(lam), kind="stable")
    return lam[order], vec[:, order]


def leading(lam, vec, n_comps):
    """The n_comps pairs of largest magnitude of ``dense_spectrum``, listed by descending value, signs fixed."""
    pick = np.argsort(-lam[:n_comps], kind="stable")
    return lam[:n_comps][pick], fix_signs(vec[:, :n_comps][:, pick])


def lanczos(T, n_comps=15, tol=1e-10, seed=0, max_steps=None, check_every=16):
    """The solver of prosstt_amd.graph in numpy: (eigenvalues, eigenvectors, steps, residual estimates)."""
    N = T.shape[0]
    limit = min(N, 2048) if max_steps is None else min(N, max_steps)
    V = np.zeros((limit + 1, N))
    V[0] = np.random.default_rng(seed).standard_normal(N)
    V[0] /= np.linalg.norm(V[0])
    alpha, beta = np.zeros(limit), np.zeros(limit)
    for j in range(limit):
        w = T @ V[j]
        alpha[j] = w @ V[j]
        for _ in range(2):
            w = w - V[:j + 1].T @ (V[:j + 1] @ w)
        beta[j] = np.linalg.norm(w)
        m = j + 1
        broke = not beta[j] >= N * 2.0 ** -52
        if not broke:
            V[j + 1] = w / beta[j]
        if not (broke or (m % check_every == 0 and m >= n_comps) or m == limit):
            continue
        if m >= n_comps:
            tri = np.diag(alpha[:m]) + np.diag(beta[:m - 1], 1) + np.diag(beta[:m - 1], -1)
            theta, S = np.linalg.eigh(tri)
            pick = np.argsort(-np.abs(theta), kind="stable")[:n_comps]
            pick = pick[np.argsort(-theta[pick], kind="stable")]
            res = np.abs(beta[m - 1] * S[m - 1, pick])
            if np.all(res < tol):
                vec = V[:m].T @ S[:, pick]
                return theta[pick], fix_signs(vec / np.linalg.norm(vec, axis=0)), m, res
        if broke:
            break
    raise RuntimeError("the model's Lanczos run did not converge")


@functools.lru_cache(maxsize=None)
def case(N, k, d=10, kind="tree"):
    """The shared, read-only model of one test input: a dict with the panel P, the model's neighbours (idx, d2) and
    graph (W, rho, sigma, T, q, z).  kind: "tree" (tree_points with seed N + k) or a kind of knn_model.KINDS."""
    P = tree_points(N, d, N + k) if kind == "tree" else knn_model.KINDS[kind](N, d, N + k)
    idx, d2 = knn_model.model(P, k)
    W, rho, sigma = connectivities(idx, d2)
    T, q, z = transitions(W)
    out = dict(P=P, idx=idx, d2=d2, W=W, rho=rho, sigma=sigma, T=T, q=q, z=z)
    for v in out.values():
        for arr in ((v.data, v.indices, v.indptr) if sparse.issparse(v) else (v,)):
            arr.setflags(write=False)
    return out
