"""The numpy model of prosstt_amd.dpt (include/prosstt_amd_dpt.h's definition), stage by stage, and the truth of the inputs the
DPT tests share.  A helper: nothing here is collected."""
import functools

import numpy as np

import graph_model

THRESHOLD = 0.9994

# (N, k) of graph_model.case -> the share of cells with a non-zero group, their agreement with the true arm, Kendall's tau of
# the pseudotime against the true time: what a numpy prototype on the dense spectrum gave with the root at the far end of arm
# 0.  A result on other eigenvectors (graph_model.lanczos, the device's) may differ by their rounding near a split: each
# figure may fall short by SLACK.
TABLE = {(1000, 14): (0.963, 0.9917, 0.936), (2000, 14): (0.956, 0.9911, 0.926), (300, 5): (0.973, 0.9726, 0.893)}
SLACK = 0.01


def weights(eigenvalues, n_dcs):
    lam = np.array(eigenvalues[:n_dcs], dtype=np.float64)
    w = np.ones_like(lam)
    for l in range(lam.size):
        if lam[l] < THRESHOLD:
            w[l] = lam[l] / (1.0 - lam[l])
    return w


def rows(vectors, w, sources):
    """d(s, .) for s of ``sources``: (len(sources), N) float64, every operation rounded on its own."""
    psi = np.asarray(vectors, dtype=np.float64)
    src = np.asarray(sources, dtype=np.int64)
    acc = np.zeros((src.size, psi.shape[0]))
    for l in range(len(w)):
        t = w[l] * (psi[src, l][:, None] - psi[None, :, l])
        acc = acc + t * t
    return np.sqrt(acc)


def ulp_distance(a, b):
    """|a - b| in units of the last place of b (finite binary64 arrays)."""
    return np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b)))


def tips(vectors, w, root):
    """(t0, t1, t2) and the distance rows (3, N) of the tips; np.argmax takes the lowest index among equals."""
    t0 = int(np.argmax(rows(vectors, w, [root])[0]))
    d0 = rows(vectors, w, [t0])[0]
    t1 = int(np.argmax(d0))
    d1 = rows(vectors, w, [t1])[0]
    t2 = int(np.argmax(d0 + d1))
    return (t0, t1, t2), np.stack([d0, d1, rows(vectors, w, [t2])[0]])


def ranks(D):
    """(order, ru, rv), (3, N) each, of the three rotations of the tips' distance rows ``D`` (3, N)."""
    order = np.stack([np.argsort(D[a], kind="stable") for a in range(3)])
    ru = np.stack([np.unique(D[(a + 1) % 3][order[a]], return_inverse=True)[1] for a in range(3)]).astype(np.int32)
    rv = np.stack([np.unique(D[(a + 2) % 3][order[a]], return_inverse=True)[1] for a in range(3)]).astype(np.int32)
    return order, ru, rv


def sign_matrix(ru, rv):
    """s_pq of one sequence pair as a dense (N, N) int64 matrix."""
    ru, rv = np.asarray(ru, dtype=np.int64), np.asarray(rv, dtype=np.int64)
    return np.sign(ru[:, None] - ru[None, :]) * np.sign(rv[:, None] - rv[None, :])


def concordance(ru, rv, block=1024):
    """(lower, upper) int64 of int32 rank arrays (batch, N), by blocks of rows of the sign matrix."""
    ru, rv = np.asarray(ru, dtype=np.int64), np.asarray(rv, dtype=np.int64)
    batch, N = ru.shape
    lower, upper = np.zeros((batch, N), dtype=np.int64), np.zeros((batch, N), dtype=np.int64)
    cols = np.arange(N)
    for b in range(batch):
        for r0 in range(0, N, block):
            r = np.arange(r0, min(N, r0 + block))
            s = np.sign(ru[b, r, None] - ru[b, None, :]) * np.sign(rv[b, r, None] - rv[b, None, :])
            lower[b, r] = np.where(cols[None, :] < r[:, None], s, 0).sum(axis=1)
            upper[b, r] = np.where(cols[None, :] > r[:, None], s, 0).sum(axis=1)
    return lower, upper


def split_diff(lower, upper, m):
    """(the candidates n = m .. N - m, diff(n)) of one sequence pair."""
    lower, upper = np.asarray(lower, dtype=np.int64), np.asarray(upper, dtype=np.int64)
    N = lower.size
    n = np.arange(m, N - m + 1, dtype=np.int64)
    head = np.concatenate([[0], np.cumsum(lower)])[n]
    tail = upper.sum() - np.concatenate([[0], np.cumsum(upper)])[n]
    head_pairs, tail_pairs = (n * (n - 1)) // 2, ((N - n) * (N - n - 1)) // 2
    return n, head.astype(np.float64) / head_pairs.astype(np.float64) - tail.astype(np.float64) / tail_pairs.astype(np.float64)


def splits(lower, upper, m):
    """n* per row of (batch, N) sums."""
    out = []
    for lo, up in zip(lower, upper):
        n, diff = split_diff(lo, up, m)
        out.append(int(n[np.argmax(diff)]))
    return tuple(out)


def groups(order, heads):
    N = order.shape[1]
    in_head = np.zeros((3, N), dtype=bool)
    for a in range(3):
        in_head[a, order[a, :heads[a]]] = True
    label = (in_head * np.array([[1], [2], [3]])).sum(axis=0)
    return np.where(in_head.sum(axis=0) == 1, label, 0).astype(np.int8)


def dpt(eigenvalues, vectors, root, n_dcs=None, min_group_size=5):
    """The whole call with one branching: a dict of pseudotime, tips, rows, order, ru, rv, lower, upper, splits, groups."""
    n_dcs = min(10, len(eigenvalues)) if n_dcs is None else n_dcs
    w = weights(eigenvalues, n_dcs)
    d_root = rows(vectors, w, [root])[0]
    t, D = tips(vectors, w, root)
    order, ru, rv = ranks(D)
    lower, upper = concordance(ru, rv)
    heads = splits(lower, upper, min_group_size)
    return dict(pseudotime=d_root / d_root.max(), tips=t, rows=D, order=order, ru=ru, rv=rv, lower=lower, upper=upper,
                splits=heads, groups=groups(order, heads))


def tree_truth(N, d, seed):
    """(arm (N,) in {0, 1, 2}, position along the arm (N,) in [0, 1)) of the cells of graph_model.tree_points(N, d, seed),
    by replaying its generator."""
    rng = np.random.default_rng(seed)
    rng.standard_normal((3, d))
    arm = rng.integers(0, 3, N)
    return arm, rng.random(N)


def truth(N, k, d=10):
    """(arm, position, root, true time from the root) of graph_model.case(N, k): the root is the far end of arm 0, and the
    time runs down arm 0 and up the other two."""
    arm, pos = tree_truth(N, d, N + k)
    root = int(np.argmax(np.where(arm == 0, pos, -1.0)))
    return arm, pos, root, np.where(arm == 0, pos[root] - pos, pos[root] + pos)


def structure(res, arm):
    """What the tests ask of a result on a noisy Y: (the tips' true arms, cells per group 1 .. 3, the share of cells with
    a non-zero group, the agreement of those with the true arm under the tips' naming)."""
    tip_arms = [int(arm[t]) for t in res["tips"]]
    g = np.asarray(res["groups"])
    assigned = g > 0
    named = np.array(tip_arms)[np.maximum(g, 1) - 1]
    return tip_arms, [int((g == i).sum()) for i in (1, 2, 3)], float(assigned.mean()), float((named == arm)[assigned].mean())


@functools.lru_cache(maxsize=None)
def case(N, k, n_comps=15):
    """The shared, read-only model of one DPT input: graph_model.case(N, k)'s diffusion map from graph_model.lanczos (values,
    vectors), the truth, and the model's result with the defaults."""
    values, vectors, _, _ = graph_model.lanczos(graph_model.case(N, k)["T"], n_comps)
    arm, pos, root, time = truth(N, k)
    out = dict(values=values, vectors=vectors, arm=arm, pos=pos, root=root, time=time, model=dpt(values, vectors, root))
    for v in (values, vectors, arm, pos, time):
        v.setflags(write=False)
    return out
