"""The numpy model of prosstt_amd.trends (the definition in its module docstring and in include/prosstt_amd_trends.h), written
for clarity: the tree distance between any two positions, the dense R x N table of weights, the CSR matrix cut from it, and
the exact sums in Python integers.  Nothing here is windowed, and nothing imports the module under test."""
import numpy as np

ONE = 4096


# ------------------------------------------------------------------------------------------------------- the tree

class Nodes:
    """Branches in ``tree.branches`` order: ``first``, ``last``, ``length``, ``offset`` per branch; ``parent`` (index or -1);
    per node its branch and absolute time."""

    def __init__(self, tree):
        self.names = list(tree.branches)
        index = {b: i for i, b in enumerate(self.names)}
        B = len(self.names)
        self.length = [int(tree.time[b]) for b in self.names]
        self.parent = [-1] * B
        for p, c in tree.topology:
            self.parent[index[c]] = index[p]
        self.first = [None] * B
        self.first[index[tree.root]] = 0
        for p, c in tree.topology:                   # parents come first in a valid topology
            self.first[index[c]] = self.first[index[p]] + self.length[index[p]]
        self.last = [f + n - 1 for f, n in zip(self.first, self.length)]
        self.offset = list(np.cumsum([0] + self.length[:-1]))
        self.R = sum(self.length)
        self.node_branch = np.concatenate([np.full(n, b) for b, n in enumerate(self.length)])
        self.node_time = np.concatenate([f + np.arange(n, dtype=np.float64) for f, n in zip(self.first, self.length)])

    def ancestors(self, b):
        out = [b]
        while self.parent[out[-1]] >= 0:
            out.append(self.parent[out[-1]])
        return out

    def codes(self, branches):
        index = {b: i for i, b in enumerate(self.names)}
        return np.array([index[b] for b in list(branches)], dtype=np.int64)


def distance(nodes, b, t, b2, t2):
    """The tree distance of (b, t) and (b2, t2): binary64 scalars in, one out, each operation rounded on its own."""
    t, t2 = np.float64(t), np.float64(t2)
    up, up2 = nodes.ancestors(b), nodes.ancestors(b2)
    if b in up2 or b2 in up:
        return abs(t - t2)
    common = next(a for a in up if a in up2)
    e = np.float64(nodes.last[common])
    return (t - e) + (t2 - e)


def tricube_q(d, h):
    d, h = np.float64(d), np.float64(h)
    u = d / h
    if u >= 1.0:
        return 0
    c = (u * u) * u
    v = np.float64(1.0) - c
    w = (v * v) * v
    return int(np.floor(w * np.float64(ONE) + np.float64(0.5)))


def nearest_label(nodes, b, t):
    j = int(np.floor((np.float64(t) - np.float64(nodes.first[b])) + np.float64(0.5)))
    return int(nodes.offset[b]) + min(max(j, 0), nodes.length[b] - 1)


def dense_weights(tree, pseudotime, branches, bandwidth=3.0, kernel="tricube"):
    """(Q, labels): the (R, N) int32 table of weights, entry by entry, and the nearest node of every cell."""
    nodes = Nodes(tree)
    t = np.asarray(pseudotime, dtype=np.float64)
    codes = nodes.codes(branches)
    N = t.shape[0]
    Q = np.zeros((nodes.R, N), dtype=np.int32)
    labels = np.array([nearest_label(nodes, int(codes[i]), t[i]) for i in range(N)], dtype=np.int32)
    if kernel == "nearest":
        Q[labels, np.arange(N)] = ONE
        return Q, labels
    for r in range(nodes.R):
        for i in range(N):
            d = distance(nodes, int(nodes.node_branch[r]), nodes.node_time[r], int(codes[i]), t[i])
            Q[r, i] = tricube_q(d, bandwidth)
    return Q, labels


def csr_of(Q):
    """(indptr int64, indices int32, weights int32) of the positive entries of a dense table, columns ascending."""
    R = Q.shape[0]
    indptr = np.zeros(R + 1, dtype=np.int64)
    indices, weights = [], []
    for r in range(R):
        cols = np.flatnonzero(Q[r] > 0)
        indices.append(cols.astype(np.int32))
        weights.append(Q[r, cols].astype(np.int32))
        indptr[r + 1] = indptr[r] + len(cols)
    return indptr, np.concatenate(indices) if R else np.zeros(0, np.int32), np.concatenate(weights) if R else np.zeros(0, np.int32)


# ----------------------------------------------------------------------------------------------------------- sums

def node_sums_exact(X, indptr, indices, weights):
    """(S1, S2): (R, G) object arrays of Python integers, term by term."""
    R, G = len(indptr) - 1, X.shape[1]
    S1 = np.zeros((R, G), dtype=object)
    S2 = np.zeros((R, G), dtype=object)
    for r in range(R):
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            q = int(weights[e])
            row = [int(v) for v in X[int(indices[e])]]
            for g in range(G):
                S1[r, g] += q * row[g]
                S2[r, g] += q * row[g] * row[g]
    return S1, S2


def node_sums(X, indptr, indices, weights):
    """The same (S1, S2), vectorised: uint64 sums of q x and of q times the two 32-bit halves of x^2 (each below 2^64 for rows
    of fewer than 2^20 entries), put together in Python integers.  tests/test_trends_model.py holds it against the above."""
    R, G = len(indptr) - 1, X.shape[1]
    S1 = np.zeros((R, G), dtype=object)
    S2 = np.zeros((R, G), dtype=object)
    Xu = np.asarray(X).astype(np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    for r in range(R):
        lo, hi = int(indptr[r]), int(indptr[r + 1])
        assert hi - lo < 1 << 20
        if hi == lo:
            continue
        rows = Xu[np.asarray(indices[lo:hi], dtype=np.int64)]
        q = np.asarray(weights[lo:hi]).astype(np.uint64)[:, None]
        sq = rows * rows
        s1 = (q * rows).sum(axis=0, dtype=np.uint64)
        a = (q * (sq & mask)).sum(axis=0, dtype=np.uint64)
        b = (q * (sq >> np.uint64(32))).sum(axis=0, dtype=np.uint64)
        S1[r] = s1.astype(object)
        S2[r] = a.astype(object) + b.astype(object) * (1 << 32)
    return S1, S2


def words(S2):
    """(R, G, 2) uint64: the (low, high) words of an object array of integers below 2^128."""
    flat = [(int(v) & ((1 << 64) - 1), int(v) >> 64) for v in np.asarray(S2, dtype=object).reshape(-1)]
    return np.array(flat, dtype=np.uint64).reshape(tuple(np.shape(S2)) + (2,))


def as_int64(S1):
    return np.array([int(v) for v in np.asarray(S1, dtype=object).reshape(-1)], dtype=np.int64).reshape(np.shape(S1))


def row_constants(indptr, indices, weights, sc):
    """(weight, weight_sq, exposure, effective_cells): exposure adds q_e s_e in binary64, entry after entry from 0."""
    R = len(indptr) - 1
    weight = np.zeros(R, dtype=np.int64)
    weight_sq = np.zeros(R, dtype=np.int64)
    exposure = np.zeros(R, dtype=np.float64)
    s = np.asarray(sc, dtype=np.float32)
    for r in range(R):
        acc = np.float64(0.0)
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            q = int(weights[e])
            weight[r] += q
            weight_sq[r] += q * q
            acc = acc + np.float64(q) * np.float64(s[int(indices[e])])
        exposure[r] = acc
    with np.errstate(invalid="ignore", divide="ignore"):
        effective = weight.astype(np.float64) ** 2 / weight_sq.astype(np.float64)
    return weight, weight_sq, exposure, effective
