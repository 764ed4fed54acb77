"""The numpy model of prosstt_amd/regress.py and libprosstt_amd_regress.so (include/prosstt_amd_regress.h holds the
definition), in the same operation order: every product and sum below is one rounded binary64 operation, eta is added from +0
with j ascending, a gene's terms are added in ascending row order within a block of rows (``regress.row_blocks``: np.cumsum
adds one after the other) and the blocks' sums in ascending order.  exp, log1p and log are numpy's.

    eta = sum_j D[l][j] C[g][j];  mu = s exp(eta);  d = a mu + b;  w = mu / d;  u = (x - mu) / d
    U[g][j] += D[l][j] u;  I[g][j,k] += (D[l][j] D[l][k]) w;  M[g][j,k] += (D[l][j] D[l][k]) (u u)
    L1 = log1p((a mu) / b);  T = a > 0 ? L1 / a : mu / b;  Q[g] += x = 0 ? -T : (x / b) ((eta + log s) - (log b + L1)) - T

``normal_equations`` also returns, per output, the sum of the magnitudes of the parts of its terms, what the tolerances of the
tests are relative to: for U |D_j| (x + mu) / d (the two parts of u, which cancel where x is near mu), for I |D_j D_k| w, for
M |D_j D_k| ((x + mu) / d)^2, for Q (x / b) (|eta| + |log s| + |log b| + L1) + T.  ``regression`` is the whole fit through
``regress.regression_with``."""
from typing import NamedTuple

import numpy as np

from prosstt_amd import regress

ETA_MAX = 700.0
LARGEST = 1e150


class Sums(NamedTuple):
    """What ``normal_equations`` returns: ``ne`` a ``regress.NormalEquations`` of host arrays, ``s_score`` (G, p),
    ``s_information`` (G, p, p) and ``s_q`` (G,) the sums of magnitudes, ``status`` the bits the device would set."""
    ne: regress.NormalEquations
    s_score: np.ndarray
    s_information: np.ndarray
    s_q: np.ndarray
    status: int


def _blocked_sum(terms, rows_per_block):
    """The sum over axis 0 in the device's order: one after the other within a block of rows, then block after block.
    ``rows_per_block`` None: numpy's own (pairwise) sum, several times faster, for statistics that need no bits."""
    if rows_per_block is None:
        return terms.sum(axis=0)
    total = np.zeros(terms.shape[1:])
    for lo in range(0, terms.shape[0], rows_per_block):
        total = total + np.cumsum(terms[lo:lo + rows_per_block], axis=0)[-1]
    return total


def normal_equations(X, size, labels, design, coef, alpha, beta, meat=False, ordered=True):
    """``Sums`` of host arrays: X (N, G) integers, size (N,), labels (N,) integers (negative: left out), design (K, p), coef
    (G, p), alpha and beta numbers or (G,).  ``ordered=False`` adds with numpy's own sum instead of the device's order."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    D = np.asarray(design, dtype=np.float64)
    K, p = D.shape
    size = np.asarray(size, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    C = np.array(coef, dtype=np.float64)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (G,)).copy()
    b = np.broadcast_to(np.asarray(beta, dtype=np.float64), (G,)).copy()
    status = 0
    with np.errstate(invalid="ignore"):
        bad_par = ~((a >= 0) & np.isfinite(a) & (b >= 1) & np.isfinite(b))
        row_ok = (labels >= 0) & (labels < K)
        bad_size = row_ok & ~((size > 0) & (size <= LARGEST))
    if bad_par.any():
        status |= regress.PARAMETER
        a[bad_par], b[bad_par] = 0.0, 2.0
    if not np.all(np.isfinite(C)):
        status |= regress.COEFFICIENT
        C[~np.isfinite(C)] = 0.0
    if np.any(labels >= K):
        status |= regress.LABEL
    if bad_size.any():
        status |= regress.SIZE
    use = row_ok & ~bad_size
    rows_per_block = regress.row_blocks(N, G)[0] if ordered else None
    lab = np.where(use, labels, 0)
    Dl = D[lab]                                                    # (N, p)
    s = np.where(use, size, 1.0)[:, None]
    x = X.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        eta = np.zeros((N, G))
        for j in range(p):
            eta = eta + Dl[:, j, None] * C[None, :, j]
        if np.any(X[use] < 0):
            status |= regress.NEGATIVE
        ok = use[:, None] & (X >= 0)
        eta_ok = np.abs(eta) <= ETA_MAX
        if np.any(ok & ~eta_ok):
            status |= regress.ETA
        ok &= eta_ok
        eta = np.where(ok, eta, 0.0)
        mu = s * np.exp(eta)
        amu = a[None, :] * mu
        d = amu + b[None, :]
        d_ok = d <= 1.7976931348623157e308
        if np.any(ok & ~d_ok):
            status |= regress.ETA
        ok &= d_ok
        mu, amu, d = np.where(ok, mu, 1.0), np.where(ok, amu, 0.0), np.where(ok, d, 1.0)
        w = mu / d
        u = (x - mu) / d
        both = (np.abs(x) + mu) / d
        second, s_second = (u * u, both * both) if meat else (w, w)
        sums_ok = ok & (second <= 1.7976931348623157e308)         # (u u overflowed: the bit, and no sum of U or M takes the entry)
        if np.any(ok & ~sums_ok):
            status |= regress.ETA
        score, s_score = np.empty((G, p)), np.empty((G, p))
        info, s_info = np.empty((G, p, p)), np.empty((G, p, p))
        for j in range(p):
            f = Dl[:, j, None]
            score[:, j] = _blocked_sum(np.where(sums_ok, f * u, 0.0), rows_per_block)
            s_score[:, j] = np.where(sums_ok, np.abs(f) * both, 0.0).sum(axis=0)
            for k in range(j, p):
                f = (Dl[:, j] * Dl[:, k])[:, None]
                info[:, j, k] = info[:, k, j] = _blocked_sum(np.where(sums_ok, f * second, 0.0), rows_per_block)
                s_info[:, j, k] = s_info[:, k, j] = np.where(sums_ok, np.abs(f) * s_second, 0.0).sum(axis=0)
        logs, logb = np.log(s), np.log(b)[None, :]
        l1 = np.log1p(amu / b[None, :])
        t = np.where(a[None, :] > 0, l1 / np.where(a > 0, a, 1.0)[None, :], mu / b[None, :])
        xb = x / b[None, :]
        full = xb * ((eta + logs) - (logb + l1)) - t
        q = _blocked_sum(np.where(ok, np.where(X == 0, -t, full), 0.0), rows_per_block)
        s_q = np.where(ok, np.abs(xb) * (np.abs(eta) + np.abs(logs) + np.abs(logb) + l1) + t, 0.0).sum(axis=0)
    ne = regress.NormalEquations(score, info, q, ok.sum(axis=0), N, meat)
    return Sums(ne, s_score, s_info, s_q, status)


def evaluator(X, size, labels, design, alpha, beta, ordered=True):
    """evaluate(coef, meat) -> NormalEquations, as ``regress.regression_with`` takes it."""
    def evaluate(coef, meat):
        return normal_equations(X, size, labels, design, coef, alpha, beta, meat, ordered).ne
    return evaluate


def regression(X, size, labels, design, alpha, beta, ordered=True, **options):
    """``regress.Regression`` of host arrays: ``regress.regression`` with the model in place of the device."""
    X = np.asarray(X, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    D = design.matrix if isinstance(design, regress.TreeDesign) else np.asarray(design, dtype=np.float64)
    keep = labels >= 0
    totals = X[keep].sum(axis=0)
    return regress.regression_with(evaluator(X, size, labels, D, alpha, beta, ordered), D, totals,
                                   float(np.asarray(size, dtype=np.float64)[keep].sum()), **options)
