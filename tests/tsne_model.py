"""The binary64 model of prosstt_amd.tsne (include/prosstt_amd_tsne.h's definition) in numpy and scipy, and the runs the t-SNE
tests share.  Affinities, gradient and objective are binary64 throughout; the update rule is the definition's binary32 one.
The pair sums use no N x N x c temporary: sum_j q^2 (y_i - y_j) = y_i sum_j q^2 - (Q^2 Y)_i.  A helper: nothing here is
collected."""
import functools
from typing import Any, NamedTuple

import numpy as np
import scipy.sparse as sparse

import graph_model

BISECTIONS = 64
TILE = 256


def entropy(g, beta):
    """(H (N,), p (N, k) unnormalised, S (N,)) of the shifted distances g (N, k) at beta (N,)."""
    p = np.exp(-beta[:, None] * g)
    S = p.sum(axis=1)
    return np.log(S) + beta * (g * p).sum(axis=1) / S, p, S


def conditional(sq_distances, perplexity):
    """(p_{j|i} (N, k), beta (N,)) of float32 squared distances."""
    d2 = np.asarray(sq_distances, dtype=np.float32).astype(np.float64)
    N = d2.shape[0]
    g = d2 - d2.min(axis=1)[:, None]
    target = np.log(perplexity)
    lo, hi, beta = np.zeros(N), np.full(N, np.inf), np.ones(N)
    for _ in range(BISECTIONS):
        above = entropy(g, beta)[0] > target
        lo = np.where(above, beta, lo)
        hi = np.where(above, hi, beta)
        with np.errstate(invalid="ignore"):
            beta = np.where(above & np.isinf(hi), 2 * beta, (lo + hi) / 2)
    _, p, S = entropy(g, beta)
    return p / S[:, None], beta


def row_entropy(sq_distances, p):
    """H of the normalised rows p: sum -p log p, what the perplexity of a row is the exp of."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)


def joint(indices, cond):
    """P = (A + A^T) / (2 N) as a scipy CSR matrix, columns ascending within a row; each value one addition and one
    division."""
    indices = np.asarray(indices)
    N, k = indices.shape
    i = np.repeat(np.arange(N, dtype=np.int64), k)
    j = indices.ravel().astype(np.int64)
    keys = np.concatenate([(i << 32) | j, (j << 32) | i])
    vals = np.concatenate([cond.ravel(), cond.ravel()])
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    head = np.r_[True, keys[1:] != keys[:-1]]
    assert not np.any(~head[1:] & ~head[:-1]), "more than two entries of one key: a row lists a cell twice"
    slot = np.cumsum(head) - 1
    data = vals[head]
    second = np.flatnonzero(~head)
    data[slot[second]] = data[slot[second]] + vals[second]
    data = data / (2.0 * N)
    rows = keys[head] >> 32
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    P = sparse.csr_matrix((data, (keys[head] & 0xFFFFFFFF).astype(np.int32), indptr), shape=(N, N))
    P.has_sorted_indices = True
    return P


def affinities(indices, sq_distances, perplexity):
    """(P, beta)."""
    cond, beta = conditional(sq_distances, perplexity)
    return joint(indices, cond), beta


class Gradient(NamedTuple):
    grad: Any       # (N, c)
    Z: float
    kl: Any         # float, or False when left out
    S_A: Any        # (N, c): sum of |attraction terms|, or None
    S_R: Any        # (N, c): sum of |q^2 delta|, or None
    L: Any          # (N,): entries per row


def _q(Y):
    """q = 1 / (1 + d2) of all pairs, N x N, the diagonal 1 (in place: one N x N array)."""
    sq = np.sum(Y * Y, axis=1)
    D2 = Y @ Y.T
    D2 *= -2.0
    D2 += sq[:, None]
    D2 += sq[None, :]
    np.maximum(D2, 0.0, out=D2)
    np.fill_diagonal(D2, 0.0)
    D2 += 1.0
    return np.reciprocal(D2, out=D2)


def gradient(P, Y, exaggeration=1.0, sums=False, kl=True):
    """The definition's gradient, Z and KL at Y in binary64 (the exaggeration multiplies the attraction only; KL is that of
    P itself; ``kl=False`` leaves it out, for the descent)."""
    Y = np.asarray(Y, dtype=np.float64)
    N, c = Y.shape
    Q = _q(Y)
    Z = Q.sum() - N
    Q2 = Q * Q
    rep = Y * Q2.sum(axis=1)[:, None] - Q2 @ Y
    rows = np.repeat(np.arange(N), np.diff(P.indptr))
    delta = Y[rows] - Y[P.indices]
    d2 = np.sum(delta * delta, axis=1)
    terms = (P.data / (1.0 + d2))[:, None] * delta
    assert np.all(np.diff(P.indptr) > 0)                          # (reduceat wants no empty row)
    att = np.add.reduceat(terms, P.indptr[:-1], axis=0)
    if kl:
        live = P.data > 0
        kl = float(np.sum(P.data[live] * (np.log(P.data[live]) + np.log1p(d2[live]))) + P.data.sum() * np.log(Z))
    S_A = S_R = None
    if sums:
        S_A = np.add.reduceat(np.abs(terms), P.indptr[:-1], axis=0)
        S_R = np.stack([(Q2 * np.abs(Y[:, None, a] - Y[None, :, a])).sum(axis=1) for a in range(c)], axis=1)
    return Gradient(4.0 * (exaggeration * att - rep / Z), float(Z), kl, S_A, S_R, np.diff(P.indptr))


def step(Y, update, gains, grad, mu, eta):
    """The definition's binary32 update rule: new (Y, update, gains), every operation rounded on its own."""
    f = np.float32
    Y, update, gains, grad = (np.asarray(a, dtype=f) for a in (Y, update, gains, grad))
    gains = np.where(update * grad < f(0), gains + f(0.2), gains * f(0.8)).astype(f)
    gains = np.maximum(gains, f(0.01))
    update = (f(mu) * update - (f(eta) * gains) * grad).astype(f)
    return (Y + update).astype(f), update, gains


def schedule(n, exploration, early_exaggeration):
    """(x, mu) of iteration n."""
    return (early_exaggeration, 0.5) if n < exploration else (1.0, 0.8)


def run(P, start, n_iter, learning_rate, exploration=250, early_exaggeration=12.0, keep=()):
    """The model's descent: binary64 gradients rounded to binary32, the binary32 update rule.  (Y after n_iter iterations,
    {n: (Y, update, gains) before iteration n} for n in keep)."""
    Y = np.asarray(start, dtype=np.float32)
    update, gains = np.zeros_like(Y), np.ones_like(Y)
    shots = {}
    for n in range(n_iter):
        if n in keep:
            shots[n] = (Y, update, gains)
        x, mu = schedule(n, exploration, early_exaggeration)
        grad = gradient(P, Y, x, kl=False).grad.astype(np.float32)
        Y, update, gains = step(Y, update, gains, grad, mu, learning_rate)
    if n_iter in keep:
        shots[n_iter] = (Y, update, gains)
    return Y, shots


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def pca_start(panel, c):
    first = np.asarray(panel, dtype=np.float64)[:, :c]
    return (first / first[:, 0].std() * 1e-4).astype(np.float32)


def random_start(N, c, seed=0):
    return (1e-4 * np.random.default_rng(seed).standard_normal((N, c))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(N, k, perplexity, kind="tree"):
    """The shared, read-only model of one test input: graph_model.case's panel and neighbours with the model's cond, beta
    and P."""
    base = graph_model.case(N, k, kind=kind)
    cond, beta = conditional(base["d2"], perplexity)
    P = joint(base["idx"], cond)
    out = dict(P_panel=base["P"], idx=base["idx"], d2=base["d2"], cond=cond, beta=beta, P=P)
    for arr in (cond, beta, P.data, P.indices, P.indptr):
        arr.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_run(N, k, perplexity, n_iter, init, c=2, keep=()):
    """(start, result, shots) of the model's whole run on case(N, k, perplexity): shared and read-only."""
    cs = case(N, k, perplexity)
    start = pca_start(cs["P_panel"], c) if init == "pca" else random_start(N, c)
    out, shots = run(cs["P"], start, n_iter, auto_learning_rate(N), keep=keep)
    for arr in (start, out) + tuple(a for shot in shots.values() for a in shot):
        arr.setflags(write=False)
    return start, out, shots
