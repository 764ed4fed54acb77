"""The numpy model of prosstt_amd.ptree (include/prosstt_amd_ptree.h's definition): both passes operation by operation in the
header's orders, the bound of the soft pass, the whole fit through the package's own host steps
(``ptree.spanning_tree``, ``centre_step``, ``energy``, ``lloyd``, ``fit_tree``, ``lineage_fit``: the same code the device path
runs), and the inputs the ptree tests share.  exp and log are the C library's, through ``math``: glibc documents both within
1 ulp.  A helper: nothing here is collected."""
import math

import numpy as np

from prosstt_amd import ptree

CHUNK = 128
ETA = 2.0 ** -52                # one ulp, relative
SLACK = 1.0 + 2.0 ** -30        # the second-order terms of the first-order bounds
TINY = 1e-300                   # a w in the subnormal range has an absolute, not a relative, error


def d2(Y, C):
    """(N, R) float32: a separate float32 subtract, multiply and add per coordinate in ascending order."""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    C = np.ascontiguousarray(C, dtype=np.float32)
    acc = np.zeros((Y.shape[0], C.shape[0]), np.float32)
    for c in range(Y.shape[1]):
        t = Y[:, None, c] - C[None, :, c]
        acc += t * t
    return acc


def argmin_key(D):
    """(best int32, m float32): the smallest (bits(d2), k) of every row."""
    R = D.shape[1]
    key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(R, dtype=np.uint64)[None, :]
    best = np.argmin(key, axis=1).astype(np.int32)
    return best, D[np.arange(D.shape[0]), best]


def _map(fn, x):
    return np.array([fn(v) for v in np.asarray(x, dtype=np.float64).ravel().tolist()], dtype=np.float64).reshape(np.shape(x))


def butterfly_sum(w):
    """Z of every row of w (N, R): 64 lane sums over k = l, l + 64, ... ascending from 0.0, then the stages 32 .. 1."""
    N, R = w.shape
    J = -(-R // 64)
    padded = np.zeros((N, J * 64), dtype=np.float64)
    padded[:, :R] = w
    p = np.zeros((N, 64), dtype=np.float64)
    for j in range(J):
        p = p + padded[:, 64 * j:64 * j + 64]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = p + p[:, lanes ^ off]
    return p[:, 0]


def chunk_sums(r, Y):
    """(gamma (R,), sums (R, d)) of r (N, R) float64 and Y (N, d) float32 in the header's order: chunks of 128 cells, ascending
    cell within a chunk, ascending chunk."""
    N, R = r.shape
    d = Y.shape[1]
    chunks = -(-N // CHUNK)
    rp = np.zeros((chunks * CHUNK, R), dtype=np.float64)
    yp = np.zeros((chunks * CHUNK, d), dtype=np.float64)
    rp[:N], yp[:N] = r, np.asarray(Y, dtype=np.float32).astype(np.float64)
    rp, yp = rp.reshape(chunks, CHUNK, R), yp.reshape(chunks, CHUNK, d)
    g = np.zeros((chunks, R), dtype=np.float64)
    s = np.zeros((chunks, R, d), dtype=np.float64)
    for j in range(CHUNK):                              # (a padded cell adds +0.0, which changes no bit)
        g = g + rp[:, j, :]
        s = s + rp[:, j, :, None] * yp[:, j, None, :]
    gamma, sums = np.zeros(R, dtype=np.float64), np.zeros((R, d), dtype=np.float64)
    for ch in range(chunks):
        gamma = gamma + g[ch]
        sums = sums + s[ch]
    return gamma, sums


def assign(Y, C, sigma=0.0, responsibilities=True):
    """``ptree.Assignment`` of the model; ``resp`` is always computed."""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    D = d2(Y, C)
    best, m = argmin_key(D)
    m64 = m.astype(np.float64)
    if sigma > 0:
        a = D.astype(np.float64) - m64[:, None]
        w = _map(math.exp, -(a / sigma))
        Z = butterfly_sum(w)
        r = w / Z[:, None]
        F = m64 - sigma * _map(math.log, Z)
    else:
        r = np.zeros(D.shape, dtype=np.float64)
        r[np.arange(D.shape[0]), best] = 1.0
        F = m64
    gamma, sums = chunk_sums(r, Y)
    return ptree.Assignment(best, m, F, gamma, sums, r if responsibilities else None)


def soft_bound(Y, C, sigma, model):
    """(bound of F (N,), of resp (N, R), of gamma (R,), of sums (R, d)) between two evaluations of the soft pass whose exp and
    log are within 1 ulp.  With eta = 2^-52: w differs by 2 eta w; Z, a sum of R positive terms of depth
    ceil(R / 64) + 6, by (2 + depth) eta Z; r by (5 + depth) eta r; the per-node sums of n = min(N, 128) + ceil(N / 128)
    additions by (5 + depth + n) eta Gamma and (6 + depth + n) eta sum_i r |y|; F by sigma (2 + depth) eta +
    3 eta sigma |log Z| + eta |F|."""
    Y64 = np.asarray(Y, dtype=np.float32).astype(np.float64)
    N, R = model.resp.shape
    depth = -(-R // 64) + 6
    n = min(N, CHUNK) + -(-N // CHUNK)
    log_z = np.abs((model.sq_distance.astype(np.float64) - model.free_energy) / sigma)
    f = (sigma * (2 + depth) * ETA + 3 * ETA * sigma * log_z + ETA * np.abs(model.free_energy)) * SLACK + TINY
    r = (5 + depth) * ETA * model.resp * SLACK + TINY
    g = (5 + depth + n) * ETA * model.resp.sum(axis=0) * SLACK + N * TINY
    s = (6 + depth + n) * ETA * (model.resp.T @ np.abs(Y64)) * SLACK + N * TINY
    return f, r, g, s


def project(Y, C, edges):
    """``ptree.Projection`` of the model."""
    Y = np.asarray(Y, dtype=np.float32).astype(np.float64)
    C = np.asarray(C, dtype=np.float32).astype(np.float64)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    a, b = C[e[:, 0]], C[e[:, 1]]                       # (E, d)
    N, E, d = Y.shape[0], e.shape[0], Y.shape[1]
    u, l = np.zeros((N, E)), np.zeros((N, E))
    for c in range(d):
        dy = Y[:, None, c] - a[None, :, c]
        db = (b[:, c] - a[:, c])[None, :]
        u = u + dy * db
        l = l + db * db
    with np.errstate(divide="ignore", invalid="ignore"):
        t = u / l
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    t = np.where(l == 0.0, 0.0, t)
    q = np.zeros((N, E))
    for c in range(d):
        dy = Y[:, None, c] - a[None, :, c]
        db = (b[:, c] - a[:, c])[None, :]
        r = dy - t * db
        q = q + r * r
    bits = q.view(np.uint64)
    low = bits.min(axis=1)
    edge = np.argmax(bits == low[:, None], axis=1).astype(np.int32)
    rows = np.arange(N)
    return ptree.Projection(edge, t[rows, edge], q[rows, edge])


def initial_centres(Y, k, seed):
    picks = np.sort(np.random.default_rng(seed).choice(Y.shape[0], size=k, replace=False))
    return np.ascontiguousarray(Y, dtype=np.float32)[picks].copy()


def kmeans(Y, k, n_iter=100, seed=0, init=None):
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    centres = initial_centres(Y, k, seed) if init is None else np.asarray(init, dtype=np.float32)
    return ptree.lloyd(Y, centres, lambda C: assign(Y, C, 0.0, False), n_iter)


def principal_tree(Y, n_nodes=ptree.N_NODES, sigma=None, lam=ptree.LAM, n_iter=ptree.N_ITER, tol=ptree.TOL, seed=0,
                   init="kmeans"):
    """``ptree.principal_tree`` over the model's passes: (centres, edges, energies, sigma, steps, converged, best)."""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    N = Y.shape[0]
    centres = initial_centres(Y, n_nodes, seed) if isinstance(init, str) else np.asarray(init, dtype=np.float32)
    if isinstance(init, str) and init == "kmeans":
        centres = ptree.lloyd(Y, centres, lambda C: assign(Y, C, 0.0, False), ptree.KMEANS_ITER).centres
    if sigma is None:
        sigma = float(np.mean(assign(Y, centres, 0.0, False).sq_distance.astype(np.float64)))
    C, edges, energies, a, steps, converged = ptree.fit_tree(N, centres, lambda c: assign(Y, c, sigma, False),
                                                             lam * N / n_nodes, n_iter, tol)
    return C, edges, energies, sigma, steps, converged, a.best


def to_tree(Y, centres, edges, best, root, min_branch_nodes=ptree.MIN_BRANCH_NODES, G=500):
    """``PrincipalTree.to_tree`` over the model's passes."""
    Y = np.ascontiguousarray(Y, dtype=np.float32)
    return ptree.lineage_fit(centres.shape[0], edges, int(best[root]), min_branch_nodes, G,
                             lambda kept: assign(Y, centres[kept], 0.0, False).best,
                             lambda kept_edges: project(Y, centres, kept_edges)[:2])


def prim_margin(D):
    """The least amount by which a chosen edge of Prim's tree on D beats every other edge that crosses the cut at its step
    (inf for fewer than three nodes): a matrix within half of it of D, entry by entry, has the same tree."""
    D = np.asarray(D, dtype=np.float64)
    R = D.shape[0]
    inside = np.zeros(R, dtype=bool)
    inside[0] = True
    margin = np.inf
    for a, b in ptree.prim(D):
        crossing = np.sort(D[np.ix_(inside, ~inside)].ravel())
        if crossing.size > 1:
            margin = min(margin, crossing[1] - crossing[0])
        inside[b] = True
    return margin


# ------------------------------------------------------------------------------------------------------- shared inputs

def three_branches(N, d, seed, noise=0.15):
    """N cells on a Y of three straight branches of length 3 that meet at the origin of the first three coordinates (one
    branch along -e0, two along e0 +- e1 from the fork), Gaussian noise in all d coordinates: (Y float32, branch (N,),
    position along the branch (N,))."""
    rng = np.random.default_rng(seed)
    branch = rng.integers(0, 3, size=N)
    s = rng.random(N) * 3.0
    Y = rng.standard_normal((N, d)) * noise
    direction = np.zeros((3, d))
    direction[0, 0] = -1.0
    direction[1, 0], direction[1, 1 % d] = 0.7, 0.7
    direction[2, 0], direction[2, 1 % d] = 0.7, -0.7
    Y += s[:, None] * direction[branch]
    return Y.astype(np.float32), branch, s


def eighths(N, d, seed, span=64):
    """Coordinates that are small integers over 8: every sum of up to 2^20 of them is exact in binary64 in any order."""
    return (np.random.default_rng(seed).integers(-span, span + 1, size=(N, d)) / 8.0).astype(np.float32)
