"""The numpy model of prosstt_amd.mapping (include/prosstt_amd_mapping.h), written from the definition alone: the panel, the
scores in binary64 from the same float32 panel, the argmax with its tie rule, the log-sum-exps, the derived tolerance of the
device's binary32 chains against this model, and the argmax rule that follows from it.  tests/test_mapping_model.py pins it
to rational arithmetic, math.fsum and scipy.  No GPU, and nothing of the package is imported here."""
import math

import numpy as np

U32 = 2.0 ** -24            # the unit roundoff of binary32
U64 = 2.0 ** -53
TINY = 2.0 ** -100


def poisson_panel(means, gene_weights=None, floor=1e-7):
    """(panel float32, exposure float64): L = w (log max(m, floor) - its mean over the nodes), entries below 2^-100 in
    magnitude zero; exposure = sum_g w max(m, floor) minus its mean over the nodes.  Sums by math.fsum."""
    m = np.maximum(np.asarray(means, dtype=np.float64), float(floor))
    R, G = m.shape
    w = np.ones(G) if gene_weights is None else np.asarray(gene_weights, dtype=np.float64)
    logs = np.log(m)
    centre = np.array([math.fsum(logs[:, g]) / R for g in range(G)])
    panel = (w[None, :] * (logs - centre[None, :])).astype(np.float32)
    panel[np.abs(panel) < TINY] = 0.0
    total = np.array([math.fsum(m[r] * w) for r in range(R)])
    return panel, total - math.fsum(total) / R


def gene_sums(X, P):
    """D in binary64 from the float32 panel: the counts and the panel widened, the products exact, numpy's binary64 sums."""
    return np.asarray(X).astype(np.float64) @ np.asarray(P).astype(np.float64).T


def scores(X, s, P, m, c=None):
    """S = (D - s m) + c, every operation rounded on its own."""
    D = gene_sums(X, P)
    s, m = np.asarray(s, dtype=np.float64), np.asarray(m, dtype=np.float64)
    c = np.zeros(len(m)) if c is None else np.asarray(c, dtype=np.float64)
    return (D - s[:, None] * m[None, :]) + c[None, :]


def best(S):
    """The node of the largest score of every row: ties go to the lower node, a NaN never wins; node 0 for a row of NaNs."""
    S = np.asarray(S, dtype=np.float64)
    out = np.zeros(S.shape[0], dtype=np.int32)
    for i, row in enumerate(S):
        at, top = -1, 0.0
        for r, v in enumerate(row.tolist()):
            if v == v and (at < 0 or v > top):
                at, top = r, v
        out[i] = max(at, 0)
    return out


def lse(S, lo=0, hi=None):
    """log sum exp of the columns [lo, hi) of every row around the row's largest score there; -inf for no columns."""
    S = np.asarray(S, dtype=np.float64)[:, lo:hi]
    if S.shape[1] == 0:
        return np.full(S.shape[0], -np.inf)
    top = S.max(axis=1)
    return np.array([math.log(math.fsum(np.exp(row - t))) + t for row, t in zip(S, top)])


def branch_lse(S, offsets):
    return np.stack([lse(S, int(a), int(b)) for a, b in zip(offsets[:-1], offsets[1:])], axis=1)


def bound(X, s, P, m, c, genes_per_chain):
    """b[i][r] of the device's S against ``scores``: with C = min(genes_per_chain, G), A = sum_g |x| |P| and u = 2^-24,
    (C + 2) u A + (ceil(G / C) + 3) 2^-53 (A + |s m| + |c|): C fused multiply-adds, one rounding of a count of 2^24 or more
    and one unit for the 1 / (1 - C u) factor; then the binary64 additions."""
    X = np.asarray(X)
    G = X.shape[1]
    C = min(int(genes_per_chain), G)
    A = np.abs(X.astype(np.float64)) @ np.abs(np.asarray(P).astype(np.float64)).T
    s, m = np.asarray(s, dtype=np.float64), np.asarray(m, dtype=np.float64)
    c = np.zeros(len(m)) if c is None else np.asarray(c, dtype=np.float64)
    rest = A + np.abs(s[:, None] * m[None, :]) + np.abs(c)[None, :]
    return (C + 2) * U32 * A + (-(-G // C) + 3) * U64 * rest


def lse_bound(b, value):
    """The bound of lse and branch_lse: max_r b[i][r] + 2^-40 (1 + |lse|)."""
    return b.max(axis=1) + 2.0 ** -40 * (1.0 + np.abs(value))


def check_argmax(S, b, device_best):
    """The argmax rule, for every cell: the device's best node d must have S[d] >= max S - (b[d] + b[argmax]); where the
    model's best node beats every other node by more than the sum of the two bounds, d must be the model's.  Returns the
    share of cells with such a margin; AssertionError otherwise."""
    S, b = np.asarray(S), np.asarray(b)
    d = np.asarray(device_best).astype(np.int64)
    want = best(S).astype(np.int64)
    rows = np.arange(S.shape[0])
    assert np.all((d >= 0) & (d < S.shape[1]))
    slack = b[rows, d] + b[rows, want]
    short = S[rows, d] < S[rows, want] - slack
    assert not short.any(), "cells %s: the device's node scores below the model's best by more than the bounds" \
        % np.flatnonzero(short)[:10].tolist()
    clear = margins(S, b)
    wrong = clear & (d != want)
    assert not wrong.any(), "cells %s have a clear best node that the device missed" % np.flatnonzero(wrong)[:10].tolist()
    return float(clear.mean())


def margins(S, b):
    """Per cell: does the model's best node beat EVERY other node by more than the sum of the two bounds?"""
    S, b = np.asarray(S), np.asarray(b)
    want = best(S).astype(np.int64)
    rows = np.arange(S.shape[0])
    gap = S[rows, want][:, None] - S
    need = b[rows, want][:, None] + b
    ok = gap > need
    ok[rows, want] = True
    return ok.all(axis=1)


def node_table(topology, time, branches, root):
    """(offsets (B + 1,), branch code per node, absolute pseudotime per node) of a tree given as plain data: the nodes are the
    time steps of every branch in ``branches`` order; a child's first step follows its parent's last."""
    first = {root: 0}
    for parent, child in topology:
        first[child] = first[parent] + int(time[parent])
    offsets, code, when = [0], [], []
    for k, b in enumerate(branches):
        n = int(time[b])
        offsets.append(offsets[-1] + n)
        code += [k] * n
        when += list(range(first[b], first[b] + n))
    return np.array(offsets, dtype=np.int64), np.array(code, dtype=np.int32), np.array(when, dtype=np.int64)


def tree_distance(topology, time, branches, root, node_a, node_b):
    """The graph distance on the node tree (a child's first node hangs on its parent's last) between the nodes of two
    arrays, by the ancestors of every branch."""
    offsets, code, when = node_table(topology, time, branches, root)
    index = {b: k for k, b in enumerate(branches)}
    parent = {index[c]: index[p] for p, c in topology}
    last = {k: when[offsets[k + 1] - 1] for k in range(len(branches))}

    def chain(k):
        out = [k]
        while out[-1] in parent:
            out.append(parent[out[-1]])
        return out

    chains = [chain(k) for k in range(len(branches))]
    out = np.empty(len(node_a), dtype=np.int64)
    for i, (a, b) in enumerate(zip(np.asarray(node_a).tolist(), np.asarray(node_b).tolist())):
        ka, kb, ta, tb = int(code[a]), int(code[b]), int(when[a]), int(when[b])
        if ka in chains[kb] or kb in chains[ka]:
            out[i] = abs(ta - tb)
        else:
            common = next(k for k in chains[ka] if k in chains[kb])
            out[i] = (ta - last[common]) + (tb - last[common])
    return out
