"""The numpy model of prosstt_amd/factors.py and libprosstt_amd_factors.so (include/prosstt_amd_factors.h holds the
definition), in the same operation order: every product and sum below is one rounded binary64 operation, eta is added from +0
with j ascending, a cell's terms are added in ascending gene order within a block of genes (``factors.gene_blocks``: np.cumsum
adds one after the other; the tiles of 32 genes inside a block change no order) and the blocks' sums in ascending order.  exp,
log1p and log are numpy's.

    eta = sum_j L[g][j] C[i][j];  mu = s exp(eta);  d = a mu + b;  w = mu / d;  u = (x - mu) / d
    U[i][j] += L[g][j] u;  I[i][j,k] += (L[g][j] L[g][k]) w
    L1 = log1p((a mu) / b);  T = a > 0 ? L1 / a : mu / b;  Q[i] += x = 0 ? -T : (x / b) ((eta + log s) - (log b + L1)) - T

``cell_equations`` also returns, per output, the sum of the magnitudes of the parts of its terms, what the tolerances of the
tests are relative to (as tests/regress_model.py has them): for U |L_j| (x + mu) / d, for I |L_j L_k| w, for Q
(x / b) (|eta| + |log s| + |log b| + L1) + T.  ``glmpca`` is the whole loop through ``factors.glmpca_with``, its gene half
tests/regress_model.py's normal equations with one design row per cell."""
from typing import NamedTuple

import numpy as np

import regress_model

from prosstt_amd import factors, regress

ETA_MAX = 700.0
LARGEST = 1e150
BIG = 1.7976931348623157e308


class Sums(NamedTuple):
    """What ``cell_equations`` returns: ``eq`` a ``factors.CellEquations`` of host arrays, ``s_score`` (N, p),
    ``s_information`` (N, P2) and ``s_q`` (N,) the sums of magnitudes, ``status`` the bits the device would set."""
    eq: factors.CellEquations
    s_score: np.ndarray
    s_information: np.ndarray
    s_q: np.ndarray
    status: int


def _blocked_sum(terms, genes_per_block):
    """The sum over axis 1 in the device's order: one after the other within a block of genes, then block after block, from
    +0.  ``genes_per_block`` None: numpy's own (pairwise) sum."""
    if genes_per_block is None:
        return terms.sum(axis=1)
    total = np.zeros(terms.shape[0])
    for lo in range(0, terms.shape[1], genes_per_block):
        total = total + np.cumsum(terms[:, lo:lo + genes_per_block], axis=1)[:, -1]
    return total


def cell_equations(X, size, loadings, coef, alpha, beta, use=None, genes_per_block=0, ordered=True):
    """``Sums`` of host arrays: X (N, G) integers, size (N,), loadings (G, p), coef (N, p), alpha and beta numbers or (G,),
    use (G,) integers (negative: left out) or None.  ``ordered=False`` adds with numpy's own sums (matrix products for U and I) instead of
    the device's order."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    L = np.array(loadings, dtype=np.float64)
    p = L.shape[1]
    size = np.asarray(size, dtype=np.float64)
    C = np.array(coef, dtype=np.float64)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (G,)).copy()
    b = np.broadcast_to(np.asarray(beta, dtype=np.float64), (G,)).copy()
    gene_ok = np.ones(G, dtype=bool) if use is None else np.asarray(use) >= 0
    status = 0
    with np.errstate(invalid="ignore"):
        bad_par = gene_ok & ~((a >= 0) & np.isfinite(a) & (b >= 1) & np.isfinite(b))
        cell_ok = (size > 0) & (size <= LARGEST)
    if bad_par.any():
        status |= factors.PARAMETER
    a[bad_par | ~gene_ok], b[bad_par | ~gene_ok] = 0.0, 2.0
    if not np.all(np.isfinite(C)) or not np.all(np.isfinite(L[gene_ok])):
        status |= factors.COEFFICIENT
    C[~np.isfinite(C)] = 0.0
    L[~np.isfinite(L)] = 0.0
    L[~gene_ok] = 0.0
    if not cell_ok.all():
        status |= factors.SIZE
    per = factors.gene_blocks(N, G, genes_per_block)[0] if ordered else None
    s = np.where(cell_ok, size, 1.0)[:, None]
    x = X.astype(np.float64)
    pair = np.triu_indices(p)
    P2 = pair[0].size
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = np.zeros((N, G))
        for j in range(p):
            eta = eta + L[None, :, j] * C[:, j, None]
        ok = cell_ok[:, None] & gene_ok[None, :]
        if np.any(ok & (X < 0)):
            status |= factors.NEGATIVE
        ok = ok & (X >= 0)
        eta_ok = np.abs(eta) <= ETA_MAX
        if np.any(ok & ~eta_ok):
            status |= factors.ETA
        ok &= eta_ok
        eta = np.where(ok, eta, 0.0)
        mu = s * np.exp(eta)
        amu = a[None, :] * mu
        d = amu + b[None, :]
        d_ok = d <= BIG
        if np.any(ok & ~d_ok):
            status |= factors.ETA
        ok &= d_ok
        mu, amu, d = np.where(ok, mu, 1.0), np.where(ok, amu, 0.0), np.where(ok, d, 1.0)
        w = mu / d
        u = (x - mu) / d
        both = (np.abs(x) + mu) / d
        pairs = L[:, pair[0]] * L[:, pair[1]]                      # (G, P2): the two loadings are multiplied first
        s_score = np.where(ok, both, 0.0) @ np.abs(L)
        s_info = np.where(ok, w, 0.0) @ np.abs(pairs)
        if per is None:                                            # numpy's own sums: two matrix products
            score, info = np.where(ok, u, 0.0) @ L, np.where(ok, w, 0.0) @ pairs
        else:
            score, info = np.empty((N, p)), np.empty((N, P2))
            for j in range(p):
                score[:, j] = _blocked_sum(np.where(ok, L[None, :, j] * u, 0.0), per)
            for at in range(P2):
                info[:, at] = _blocked_sum(np.where(ok, pairs[None, :, at] * w, 0.0), per)
        logs, logb = np.log(s), np.log(b)[None, :]
        l1 = np.log1p(amu / b[None, :])
        t = np.where(a[None, :] > 0, l1 / np.where(a > 0, a, 1.0)[None, :], mu / b[None, :])
        xb = x / b[None, :]
        full = xb * ((eta + logs) - (logb + l1)) - t
        q = _blocked_sum(np.where(ok, np.where(X == 0, -t, full), 0.0), per)
        s_q = np.where(ok, np.abs(xb) * (np.abs(eta) + np.abs(logs) + np.abs(logb) + l1) + t, 0.0).sum(axis=1)
    eq = factors.CellEquations(score, info, q, ok.sum(axis=1), G)
    return Sums(eq, s_score, s_info, s_q, status)


def evaluators(X, size, alpha, beta, no_counts=None, ordered=True, transposed=False):
    """(gene_evaluate, cell_evaluate) as ``factors.glmpca_with`` takes them: the models in place of the two device passes.
    The gene half is tests/regress_model.py's normal equations with one design row per cell; ``transposed`` (one alpha and
    one beta for all genes, every gene with a count): ``cell_equations`` on the transposed matrix in its place, with size 1
    and log s_i as the fixed coefficient of one more loading column -- the same sums up to rounding
    (tests/test_factors_model.py), many times faster with ``ordered=False``, for the calibrations."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    size = np.asarray(size, dtype=np.float64)
    use = None if no_counts is None else np.where(no_counts, -1, 0)

    def gene_evaluate(scores, coef):
        design = np.concatenate([np.ones((N, 1)), scores], axis=1)
        if not transposed:
            return regress_model.normal_equations(X, size, np.arange(N), design, coef, alpha, beta, False, ordered).ne
        p = coef.shape[1]
        eq = cell_equations(X.T, np.ones(G), np.concatenate([design, np.log(size)[:, None]], axis=1),
                            np.concatenate([coef, np.ones((G, 1))], axis=1), float(alpha), float(beta), None, 0, ordered).eq
        return regress.NormalEquations(eq.score[:, :p], eq.symmetric()[:, :p, :p], eq.q, eq.used, N)

    def cell_evaluate(L, coef):
        return cell_equations(X, size, L, coef, alpha, beta, use, 0, ordered).eq

    return gene_evaluate, cell_evaluate


def glmpca(X, size, scores, alpha, beta, loadings=None, ordered=True, rotated=True, history=None, transposed=False, **options):
    """``factors.Factors`` of host arrays from the start ``scores`` (N, k) (and ``loadings``, 0 when None): ``factors.glmpca``
    with the models in place of the device."""
    X = np.asarray(X, dtype=np.int64)
    size = np.asarray(size, dtype=np.float64)
    scores = np.asarray(scores, dtype=np.float64)
    totals = X.sum(axis=0)
    no_counts = ~(totals > 0)
    loadings = np.zeros((X.shape[1], scores.shape[1])) if loadings is None else loadings
    gene_evaluate, cell_evaluate = evaluators(X, size, alpha, beta, no_counts, ordered, transposed)
    penalty, tol = options.get("penalty", factors.PENALTY), options.get("tol", factors.TOL)
    sco, lo, b, objective, converged, no_counts = factors.glmpca_with(gene_evaluate, cell_evaluate, scores, loadings, totals,
                                                                      float(size.sum()), history=history, **options)
    shift = transform = None
    if rotated:
        sco, lo, b, shift, transform = factors.rotate(sco, lo, b, full=True)
    return factors.Factors(sco, lo, b, objective, len(objective), converged, no_counts, penalty, alpha, beta, tol, shift, transform)
