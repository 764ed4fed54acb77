"""The model of prosstt_amd.cluster (include/prosstt_amd_cluster.h's definition) in numpy: quantise, sweep, totals, quality,
round, level, aggregate, louvain and the order of the labels.  Every integer array is int64, the gain is computed with
numpy's binary64 operations in the written order, Q with math.fsum.  A helper: nothing here is collected."""
import math
from typing import NamedTuple

import numpy as np


class Level(NamedTuple):
    """A level graph: symmetric integer CSR (columns ascending within a row), k its row sums, M2 their sum."""
    indptr: np.ndarray
    indices: np.ndarray
    u: np.ndarray
    k: np.ndarray
    M2: int

    @property
    def n(self):
        return len(self.indptr) - 1

    def rows(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.indptr))


def level_from_csr(indptr, indices, u):
    indptr, indices, u = (np.asarray(a).astype(np.int64) for a in (indptr, indices, u))
    n = len(indptr) - 1
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, np.repeat(np.arange(n), np.diff(indptr)), u)
    return Level(indptr, indices, u, k, int(k.sum()))


def quantize(W):
    """The level-0 graph of a scipy CSR matrix W with weights in [0, 1]."""
    w = np.asarray(W.data, dtype=np.float64)
    if not np.all((w >= 0) & (w <= 1)):
        raise ValueError("a weight outside [0, 1]")
    u = np.floor(w * np.float64(2.0 ** 32) + np.float64(0.5)).astype(np.int64)
    return level_from_csr(W.indptr, W.indices, u)


def gain(e, k, T, gamma, M2):
    e, k, T = (np.asarray(a, dtype=np.int64).astype(np.float64) for a in (e, k, T))
    return e - (np.float64(gamma) * (k * T)) / np.float64(M2)


def totals(level, c):
    c = np.asarray(c, dtype=np.int64)
    tot = np.zeros(level.n, dtype=np.int64)
    inn = np.zeros(level.n, dtype=np.int64)
    np.add.at(tot, c, level.k)
    rows = level.rows()
    same = c[rows] == c[level.indices]
    np.add.at(inn, c[rows[same]], level.u[same])
    return tot, inn


def quality(tot, inn, M2, gamma):
    t = tot.astype(np.float64) / np.float64(M2)
    terms = inn.astype(np.float64) / np.float64(M2) - np.float64(gamma) * (t * t)
    return math.fsum(terms.tolist())


def sweep(level, c, tot, parity, gamma):
    """(c_new, moved) of one synchronous sweep."""
    c = np.asarray(c, dtype=np.int64)
    n = level.n
    rows = level.rows()
    keep = level.indices != rows
    i, d, w = rows[keep], c[level.indices[keep]], level.u[keep]
    key = i * n + d
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    c_new = c.copy()
    if len(key) == 0:
        return c_new, 0
    head = np.r_[True, key[1:] != key[:-1]]
    e = np.add.reduceat(w, np.flatnonzero(head))
    ki, kd = key[head] // n, key[head] % n
    own = kd == c[ki]
    e_stay = np.zeros(n, dtype=np.int64)
    e_stay[ki[own]] = e[own]
    stay = gain(e_stay, level.k, tot[c] - level.k, gamma, level.M2)
    cand = ~own & (kd < c[ki] if parity == 0 else kd > c[ki])
    gi, gd = ki[cand], kd[cand]
    g = gain(e[cand], level.k[gi], tot[gd], gamma, level.M2)
    order = np.lexsort((gd, -g, gi))                  # by node, then gain descending, then community ascending
    gi, gd, g = gi[order], gd[order], g[order]
    if len(gi) == 0:
        return c_new, 0
    best = np.r_[True, gi[1:] != gi[:-1]]
    gi, gd, g = gi[best], gd[best], g[best]
    move = g > stay[gi]
    c_new[gi[move]] = gd[move]
    return c_new, int(move.sum())


def run_level(level, gamma, tol, max_rounds):
    """(c, rounds, Q, the Q of every accepted round) of one level."""
    c = np.arange(level.n, dtype=np.int64)
    tot, inn = totals(level, c)
    Q = quality(tot, inn, level.M2, gamma)
    trace = []
    rounds = 0
    while rounds < max_rounds:
        c1, m0 = sweep(level, c, tot, 0, gamma)
        tot1, _ = totals(level, c1)
        c2, m1 = sweep(level, c1, tot1, 1, gamma)
        tot2, in2 = totals(level, c2)
        Q2 = quality(tot2, in2, level.M2, gamma)
        if m0 + m1 == 0 or not Q2 > Q + tol:
            break
        c, tot, Q = c2, tot2, Q2
        rounds += 1
        trace.append(Q)
    return c, rounds, Q, trace


def aggregate(level, c):
    """(the next level graph, the renumbered community of every node)."""
    c = np.asarray(c, dtype=np.int64)
    present = np.unique(c)
    cp = np.searchsorted(present, c).astype(np.int64)
    n_new = len(present)
    rows = level.rows()
    key = (cp[rows] << 32) | cp[level.indices]
    keys, inverse = np.unique(key, return_inverse=True)
    u = np.zeros(len(keys), dtype=np.int64)
    np.add.at(u, inverse.ravel(), level.u)
    indptr = np.zeros(n_new + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys >> 32, minlength=n_new), out=indptr[1:])
    return level_from_csr(indptr, keys & 0xFFFFFFFF, u), cp


def order_labels(communities):
    """(labels, sizes): the communities numbered by size descending, equal sizes by their lowest cell index."""
    communities = np.asarray(communities)
    ids, first, inverse, sizes = np.unique(communities, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -sizes))
    rank = np.empty(len(ids), dtype=np.int64)
    rank[order] = np.arange(len(ids))
    return rank[inverse.ravel()].astype(np.int32), sizes[order].astype(np.int64)


class Result(NamedTuple):
    labels: np.ndarray
    sizes: np.ndarray
    modularity: float
    levels: tuple
    level_labels: tuple
    trace: tuple              # per level: the Q of every accepted round


def louvain_level0(level, gamma=1.0, tol=1e-7, max_rounds=1000, max_levels=32):
    if level.M2 == 0:
        raise ValueError("the graph has no weight")
    comp = np.arange(level.n, dtype=np.int64)
    levels, level_labels, traces = [], [], []
    Q = None
    for _ in range(max_levels):
        c, rounds, Q, trace = run_level(level, gamma, tol, max_rounds)
        nxt, cp = aggregate(level, c)
        comp = cp[comp]
        levels.append((level.n, nxt.n, rounds, Q))
        level_labels.append(comp.astype(np.int32))
        traces.append(tuple(trace))
        if nxt.n == level.n:
            break
        level = nxt
    labels, sizes = order_labels(comp)
    return Result(labels, sizes, Q, tuple(levels), tuple(level_labels), tuple(traces))


def louvain(W, gamma=1.0, tol=1e-7, max_rounds=1000, max_levels=32):
    return louvain_level0(quantize(W), gamma, tol, max_rounds, max_levels)


def modularity(W, labels, gamma=1.0):
    """The exact Q (of the quantised weights) of any labelling of the cells."""
    level = quantize(W)
    c = np.unique(np.asarray(labels), return_inverse=True)[1].ravel().astype(np.int64)
    tot, inn = totals(level, c)
    return quality(tot, inn, level.M2, gamma)


# ------------------------------------------------------------------------- inputs that kNN graphs of test size do not give

SPECIAL_ROWS = (16, 17, 64, 65, 512, 513)


def hand_built(n, weight=1 << 32, vary=False):
    """A symmetric integer level graph of n >= 5 nodes: node 0's row is dense (n entries, its diagonal among them); node 1
    has the single entry (1, 0), of weight 0, so k_1 = 0; node 2 + t has exactly SPECIAL_ROWS[t] entries where n leaves
    room (node 0, its own diagonal and a run of the other nodes); the other nodes hold what symmetry gives them and a few
    chords.  Every weight is ``weight`` (plus (i + j) % 3 with ``vary``) except the pairs with (i + j) % 7 == 1, which weigh 0.  Returns
    (Level, lengths of the rows)."""
    pairs = {(0, j) for j in range(n)}
    lengths = [L for L in SPECIAL_ROWS if L + len(SPECIAL_ROWS) + 2 <= n]
    first_filler = 2 + len(lengths)
    for t, L in enumerate(lengths):
        i = 2 + t
        pairs.add((i, i))
        for s in range(L - 2):
            pairs.add((i, first_filler + s))
    for j in range(first_filler, n - 1, 2):
        pairs.add((j, j + 1))
    for j in range(first_filler, n, 5):
        pairs.add((j, j))
    pairs |= {(j, i) for i, j in pairs}
    pairs = np.array(sorted(pairs), dtype=np.int64)
    i, j = pairs[:, 0], pairs[:, 1]
    u = np.where((i + j) % 7 == 1, 0, weight + ((i + j) % 3 if vary else 0)).astype(np.int64)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=indptr[1:])
    level = level_from_csr(indptr, j, u)
    return level, np.diff(indptr)


def tie_graph(weight=1 << 32):
    """Five nodes, the edges 4-1, 4-2, 1-3, 2-3 of one weight: from c_i = i, node 4 finds the communities 1 and 2 with
    equal e and equal tot, an exact tie of two gains above its stay; parity 0 must send it to 1."""
    pairs = [(4, 1), (4, 2), (1, 3), (2, 3)]
    pairs = np.array(sorted(pairs + [(j, i) for i, j in pairs]), dtype=np.int64)
    indptr = np.zeros(6, dtype=np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=5), out=indptr[1:])
    return level_from_csr(indptr, pairs[:, 1], np.full(len(pairs), weight, dtype=np.int64))
