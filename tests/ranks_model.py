"""A numpy restatement of the rank-sum step (include/prosstt_amd_ranks.h, prosstt_amd/ranks.py), independent of the package:
Q and T straight from their definition -- comparisons of the entries it is given, no sort -- and the Wilcoxon statistics on
them.  Nothing here imports prosstt_amd."""
import numpy as np
import scipy.stats

from markers_model import bh, rank  # noqa: F401  (rank: the ranking by score, ties to the lower index)


def position_counts(a, member):
    """Per entry q of the vector ``a``: #{c in C: a_c < a_q} + #{c in C: a_c <= a_q}, C the entries where ``member``; and
    the number of entries equal to a_q.  All by comparison, O(n^2)."""
    a = np.asarray(a)
    c = a[np.asarray(member, dtype=bool)]
    both = np.zeros(a.size, dtype=np.int64)
    equal = np.zeros(a.size, dtype=np.int64)
    for lo in range(0, a.size, 1024):                       # (blocks of entries: bounded memory)
        part = a[lo:lo + 1024, None]
        both[lo:lo + 1024] = (c[None, :] < part).sum(1) + (c[None, :] <= part).sum(1)
        equal[lo:lo + 1024] = (a[None, :] == part).sum(1)
    return both, equal


def rank_sums(A, labels, groups=None, reference=None):
    """(Q (K, G) int64, T (G,) int64, n (K,) int64) of the matrix ``A`` (cells x genes, any float type; compared as given) for
    one label per row (below 0: left out).  ``reference``: None for all labelled rows, or a group index.  A run of t equal
    values adds t^3 - t to T: each of its t entries adds t^2 - 1."""
    A = np.asarray(A)
    labels = np.asarray(labels)
    K = int(labels.max()) + 1 if groups is None else groups
    keep = labels >= 0
    A, labels = A[keep], labels[keep]
    member = np.ones(labels.size, dtype=bool) if reference is None else labels == reference
    G = A.shape[1]
    Q, T = np.zeros((K, G), dtype=np.int64), np.zeros(G, dtype=np.int64)
    for j in range(G):
        both, equal = position_counts(A[:, j], member)
        Q[:, j] = [int(both[labels == k].sum()) for k in range(K)]
        T[j] = int((equal * equal - 1).sum())
    return Q, T, np.bincount(labels, minlength=K).astype(np.int64)


def wilcoxon(Q, T, n, reference="rest", tie_correct=False):
    """dict of (K, G) arrays z, pvals, pvals_adj from the integers, group by group and gene by gene.  ``reference``: "rest" or
    a group index."""
    Q, T, n = np.asarray(Q), np.asarray(T), np.asarray(n, dtype=np.int64)
    K, G = Q.shape
    total = int(n.sum())
    out = {key: np.empty((K, G)) for key in ("z", "pvals", "pvals_adj")}
    if tie_correct and reference != "rest":
        raise ValueError("the pairwise tie term is not defined here")
    for k in range(K):
        n1 = int(n[k])
        n2 = total - n1 if reference == "rest" else int(n[reference])
        if n1 < 2 or n2 < 2:
            raise ValueError("fewer than two cells")
        z, p = np.zeros(G), np.ones(G)
        for j in range(G):
            if reference == "rest":
                c = 1.0 - float(T[j]) / (float(total) ** 3 - total) if tie_correct else 1.0
                above = (float(Q[k, j]) + n1) / 2.0 - n1 * (total + 1.0) / 2.0
                var = n1 * float(total - n1) * (total + 1.0) / 12.0 * c
            else:
                above = float(Q[k, j]) / 2.0 - n1 * float(n2) / 2.0
                var = n1 * float(n2) * (n1 + n2 + 1.0) / 12.0
            if var > 0:
                z[j] = above / np.sqrt(var)
                p[j] = 2.0 * scipy.stats.norm.sf(abs(z[j]))
        out["z"][k], out["pvals"][k], out["pvals_adj"][k] = z, p, bh(p)
    return out
