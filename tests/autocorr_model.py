"""A numpy restatement of the autocorrelation step (include/prosstt_amd_autocorr.h, prosstt_amd/autocorr.py), independent of
the package: the four sums per gene of a given float32 entry matrix in the kernel's order with the kernel's roundings, the
smoothed panel, the two statistics, their exact values in rational arithmetic and their moments over every permutation of
the cells.  Nothing here imports prosstt_amd."""
import itertools
from fractions import Fraction

import numpy as np

MIN_ROWS, CELL_BLOCKS = 16, 512


def default_rows_per_block(N):
    """The library's rule for ``rows_per_block`` = 0: a function of the number of cells alone."""
    return max(MIN_ROWS, -(-N // CELL_BLOCKS))


def lag(A, indptr, indices, data, mu=None, squares=True):
    """(m, q): per cell and gene m = sum_e w_e z_j and q = sum_e w_e (a_i - a_j)^2 over the row's entries in CSR order, both
    from 0 and every operation rounded on its own: slot by slot over the positions of the rows (numpy's ufuncs do not fuse).
    ``A``: (N, G) float32 entries, widened here; ``mu``: (G,) binary64 or None for 0."""
    A = np.asarray(A).astype(np.float64)
    Z = A if mu is None else A - np.asarray(mu, dtype=np.float64)[None, :]
    deg = np.diff(indptr)
    m, q = np.zeros(A.shape), np.zeros(A.shape)
    for slot in range(int(deg.max()) if deg.size else 0):
        rows = np.flatnonzero(deg > slot)
        e = indptr[rows] + slot
        j, w = indices[e], data[e][:, None]
        m[rows] = m[rows] + w * Z[j]
        if squares:
            d = A[rows] - A[j]
            q[rows] = q[rows] + w * (d * d)
    return m, q


def _over_cells(T, rows_per_block):
    """The sum over the rows of T in the kernel's order: blocks of ``rows_per_block`` consecutive rows, row after row from 0
    within a block, then the blocks ascending from 0."""
    N, G = T.shape
    blocks = -(-N // rows_per_block)
    part = np.zeros((blocks, G))
    for k in range(rows_per_block):
        rows = np.arange(k, N, rows_per_block)
        part[:rows.size] = part[:rows.size] + T[rows]
    total = np.zeros(G)
    for b in range(blocks):
        total = total + part[b]
    return total


def sums(A, indptr, indices, data, mu, rows_per_block, cell_of_row=None):
    """(cross, sqdiff, m2, m4), each (G,), to the bit what the kernel gives for these float32 entries.  ``A``'s rows are the
    cells in plan order (the graph's nodes); ``cell_of_row``: the cell that each row of the device's matrix holds (None: row i
    is cell i) -- the cells are summed in the order of those rows."""
    A64 = np.asarray(A).astype(np.float64)
    Z = A64 - np.asarray(mu, dtype=np.float64)[None, :]
    m, q = lag(A, indptr, indices, data, mu)
    zz = Z * Z
    order = slice(None) if cell_of_row is None else np.asarray(cell_of_row)
    return tuple(_over_cells(T[order], rows_per_block) for T in (Z * m, q, zz, zz * zz))


def smooth(A, indptr, indices, data, normalize):
    """The smoothed float32 panel: m with mu = 0, times 1 / d_i (d_i the row's weights added in CSR order from 0) when
    ``normalize``, one product and one rounding to float32; zeros where d_i == 0."""
    m, _ = lag(A, indptr, indices, data, None, squares=False)
    if not normalize:
        return m.astype(np.float32)
    deg = np.diff(indptr)
    d = np.zeros(len(deg))
    for slot in range(int(deg.max()) if deg.size else 0):
        rows = np.flatnonzero(deg > slot)
        d[rows] = d[rows] + data[indptr[rows] + slot]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (m * (1.0 / d)[:, None]).astype(np.float32)
    out[d == 0] = 0.0
    return out


def morans_i(cross, m2, N, W0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (N / W0) * (cross / m2)


def gearys_c(sqdiff, m2, N, W0):
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((N - 1) / (2 * W0)) * (sqdiff / m2)


def dense(indptr, indices, data):
    N = len(indptr) - 1
    W = np.zeros((N, N))
    for i in range(N):
        for e in range(indptr[i], indptr[i + 1]):
            W[i, indices[e]] += data[e]
    return W


def exact_sums(A, indptr, indices, data, mu):
    """((cross, sqdiff, m2, m4), (their sums of |terms|), (their numbers of terms)) of the definitions in rational arithmetic,
    per gene as Fractions: the entries, the weights and mu are taken as the exact values of their floats."""
    A = np.asarray(A)
    N, G = A.shape
    values, masses = [[] for _ in range(4)], [[] for _ in range(4)]
    nnz = int(indptr[-1])
    for g in range(G):
        a = [Fraction(float(v)) for v in A[:, g]]
        z = [v - Fraction(float(mu[g])) for v in a]
        terms = [[], [], [z[i] * z[i] for i in range(N)], [z[i] ** 4 for i in range(N)]]
        for i in range(N):
            for e in range(indptr[i], indptr[i + 1]):
                j, w = int(indices[e]), Fraction(float(data[e]))
                terms[0].append(w * z[i] * z[j])
                terms[1].append(w * (a[i] - a[j]) ** 2)
        for k in range(4):
            values[k].append(sum(terms[k], Fraction(0)))
            masses[k].append(sum((abs(t) for t in terms[k]), Fraction(0)))
    return values, masses, (nnz, nnz, N, N)


def permutation_moments(x, W):
    """(mean I, var I, mean C, var C) over ALL permutations of the values ``x`` on the nodes of the dense weight matrix ``W``
    (population variance): the definitions evaluated len(x)! times in binary64."""
    x = np.asarray(x, dtype=np.float64)
    N = x.size
    W0 = W.sum()
    z = x - x.mean()
    m2 = float(np.sum(z * z))
    P = np.array(list(itertools.permutations(range(N))))
    Z = z[P]
    cross = np.einsum("pi,ij,pj->p", Z, W, Z)
    D = Z[:, :, None] - Z[:, None, :]
    sq = np.einsum("pij,ij->p", D * D, W)
    I = (N / W0) * cross / m2
    C = ((N - 1) / (2 * W0)) * sq / m2
    return I.mean(), I.var(), C.mean(), C.var()


def graph_constants(W):
    """(W0, S1, S2) of a dense weight matrix."""
    S = W + W.T
    margins = W.sum(1) + W.sum(0)
    return W.sum(), 0.5 * np.sum(S * S), np.sum(margins * margins)


def entries32(X, s):
    """float32 entries log1p(x * fl32(1 / s)) by numpy's float32 log1p: the device's entries to within a few ulp, for the
    tests that need no device."""
    inv = (1.0 / np.asarray(s, dtype=np.float64)).astype(np.float32)
    return np.log1p(np.asarray(X).astype(np.float32) * inv[:, None]).astype(np.float32)


def path_graph(N, chords=()):
    """CSR (indptr int64, indices int32 ascending, data float64) of the path 0 - 1 - ... - N - 1 with unit weights and the
    listed chords (i, j, w), symmetric."""
    W = np.zeros((N, N))
    for i in range(N - 1):
        W[i, i + 1] = W[i + 1, i] = 1.0
    for i, j, w in chords:
        W[i, j] = W[j, i] = w
    return csr_of(W)


def csr_of(W):
    indptr, indices, data = [0], [], []
    for row in W:
        at = np.flatnonzero(row)
        indices.extend(at)
        data.extend(row[at])
        indptr.append(len(indices))
    return np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int32), np.asarray(data, dtype=np.float64)
