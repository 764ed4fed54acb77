"""
Maximum-likelihood fit of the count model to a count matrix, computed where the matrix lies: on the device.  The way back
from counts to the parameters the simulator is given (``count_model.get_pr_umi``: negative binomial with mean mu = s_i m and
variance alpha mu^2 + beta mu), per gene:

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    f = fit.count_model(X, sc, sim.cell_rows(t, pt, br), fit.simulation_means(t))    # refit against the true means
    f = fit.count_model(X, sc, clusters)                     # any matrix: the means are the clusters' pseudobulk
    fit.hyperparameters(f)                                   # mean and spread of log alpha, log(beta - 1) over the genes

The reference fits one parabola of variance on mean over all genes (``learn_data_summary``) and draws per-gene values around
that average with a hand-set spread; this gives every gene its own (alpha, beta) and their standard errors.

The pass over the cells x genes matrix runs in libprosstt_amd_fit.so (include/prosstt_amd_fit.h): for up to 16 candidate
pairs per gene at once, in binary64,

    mu = s_i m[k][g]   (k: the cell's label, the row of ``means``; a negative label leaves the cell out)
    mu = 0:  the entry contributes 0; an entry x > 0 there is counted in bad[g]
    theta = a mu + (b - 1);  r = mu / theta;  L1 = log1p(theta)
    term = lgd(r, x) - r L1 + x (log theta - L1);  lgd(r, x) = lgamma(r + x) - lgamma(r)
    ll[c][g] = sum_i term;  base[g] = sum_i lgamma(x + 1);  ll - base is the full log-likelihood

Admissible parameters are finite with a >= 0, b >= 1 and a + b - 1 > 0.  There is no CPU fallback for the pass: host
matrices are refused.  The optimiser (``maximize``) runs on the host in numpy, vectorised over the genes, and knows the device
only through a callable, so that it is tested against the numpy model of the pass without a device.
"""
from typing import Any, NamedTuple

import numpy as np

from . import _cellpass, _native, markers
from . import device as _device
from ._cellpass import _codes, _host
from .device import _ptr, _torch

MAX_CANDIDATES = 16             # PROSSTT_AMD_FIT_MAX_CANDIDATES
NEGATIVE, LABEL, PARAMETER, SIZE, MEAN = 1, 2, 4, 8, 16         # the bits of the pass's status word
STATUS_MESSAGES = (
    (NEGATIVE, "NEGATIVE", _device.NEGATIVE_ENTRY),
    (LABEL, "LABEL", "a label is not below the number of rows of means"),
    (PARAMETER, "PARAMETER", "alpha and beta must be finite with alpha >= 0, beta >= 1 and alpha + beta - 1 > 0"),
    (SIZE, "SIZE", "a size factor is not positive and finite (at most 1e150)"),
    (MEAN, "MEAN", "a mean is negative or not finite (at most 1e150)"),
)
PARAMETERS = ("alpha", "beta")
HESSIAN_STEP = 1e-2             # step of the stencil that the Hessian at the optimum comes from


class LogLik:
    """The sums of one call (or of several chunks of cells, ``concat``): ``values`` (C, G) float64, ll of the module
    docstring; ``base`` (G,) float64; ``bad`` (G,) int64; ``n_cells``.  ``values`` and ``base`` are numpy arrays, or device
    tensors for ``out="torch"``."""

    def __init__(self, values, base, bad, n_cells):
        self.values, self.base = values, base
        self.bad = np.asarray(bad, dtype=np.int64)
        self.n_cells = int(n_cells)
        if len(values.shape) != 2 or tuple(base.shape) != (values.shape[1],) or self.bad.shape != (values.shape[1],):
            raise ValueError("values must be (candidates, genes), base and bad (genes,)")

    @property
    def n_genes(self):
        return int(self.values.shape[1])

    @staticmethod
    def concat(parts):
        """The sums over the cells of all ``parts`` (chunks of one matrix over cells, evaluated at the same parameters):
        added in list order."""
        parts = list(parts)
        if not parts:
            raise ValueError("concat needs at least one LogLik")
        for p in parts:
            if not isinstance(p, LogLik):
                raise TypeError("concat takes LogLik, not %s" % type(p).__name__)
            if tuple(p.values.shape) != tuple(parts[0].values.shape):
                raise ValueError("the parts cover different candidates or genes")
        values, base, bad = parts[0].values, parts[0].base, parts[0].bad
        for p in parts[1:]:
            values, base, bad = values + p.values, base + p.base, bad + p.bad
        return LogLik(values, base, bad, sum(p.n_cells for p in parts))

    def __repr__(self):
        return "LogLik(candidates=%d, genes=%d, cells=%d)" % (self.values.shape[0], self.n_genes, self.n_cells)


def check_status(bits):
    """ValueError naming every bit of the pass's status word that is set."""
    _cellpass.check_status(bits, STATUS_MESSAGES)


def _parameters(alpha, beta, n_genes):
    """(alpha, beta) as contiguous (C, G) float64 host arrays, or raise."""
    out = []
    for name, value in (("alpha", alpha), ("beta", beta)):
        v = np.asarray(_host(value), dtype=np.float64)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2 or v.shape[1] != n_genes:
            raise ValueError("%s must be (genes,) or (candidates, genes) with %d genes, not %s" % (name, n_genes, v.shape))
        out.append(np.ascontiguousarray(v))
    if out[0].shape != out[1].shape:
        raise ValueError("alpha and beta must have the same shape (got %s and %s)" % (out[0].shape, out[1].shape))
    if not 1 <= out[0].shape[0] <= MAX_CANDIDATES:
        raise ValueError("need 1 <= candidates <= %d (got %d)" % (MAX_CANDIDATES, out[0].shape[0]))
    return out


class _Pass(_cellpass.LabelledPass):
    """The device side of repeated ``loglik`` calls over one matrix: the checked matrix view, the size factors, labels and
    means on the device, and the workspace (sized for the largest C)."""

    def __init__(self, X, sc, codes, means, who):
        super().__init__(X, sc, who)
        G = self.m.G
        torch = _torch()
        if isinstance(means, torch.Tensor):
            if means.dim() != 2 or means.shape[1] != G or means.shape[0] < 1:
                raise ValueError("means must be (rows, %d genes), not %s" % (G, tuple(means.shape)))
        else:
            means = np.asarray(means, dtype=np.float64)
            if means.ndim != 2 or means.shape[1] != G or means.shape[0] < 1:
                raise ValueError("means must be (rows, %d genes), not %s" % (G, means.shape))
        dev = self.place(codes, "fit", "prosstt_amd_fit_workspace_bytes", MAX_CANDIDATES)
        if isinstance(means, torch.Tensor):
            self.means = means.to(device=dev, dtype=torch.float64).contiguous()
        else:
            self.means = torch.as_tensor(np.ascontiguousarray(means)).to(dev)
        self.K = int(self.means.shape[0])

    def __call__(self, alpha, beta, out="numpy"):
        m = self.m
        alpha, beta = _parameters(alpha, beta, m.G)
        C, G = alpha.shape
        torch = _torch()
        with torch.cuda.device(m.device):
            par = torch.as_tensor(np.stack([alpha, beta])).to(m.device)
            sums = torch.empty((C + 1, G), dtype=torch.float64, device=m.device)        # ll, then base
            bad = torch.empty(G, dtype=torch.int64, device=m.device)
            status = torch.zeros(1, dtype=torch.int32, device=m.device)
            _native.check(self.lib.prosstt_amd_fit_loglik(
                m.stream(), _ptr(m.X), m.N, G, m.ld, _ptr(self.size), _ptr(self.labels), self.K, _ptr(self.means),
                self.means.stride(0) if self.K > 1 else G, _ptr(par[0]), _ptr(par[1]), C, _ptr(self.ws), self.ws.numel(),
                _ptr(sums[:C]), _ptr(sums[C]), _ptr(bad), _ptr(status)), "fit")
            check_status(int(status.item()))
            bad = bad.cpu().numpy()
            if out == "numpy":
                sums = sums.cpu().numpy()
        return LogLik(sums[:C], sums[C], bad, m.N)


def loglik(X, sc, labels, means, alpha, beta, *, out="numpy"):
    """``LogLik`` of an int32 device count matrix at the candidates (``alpha``, ``beta``).

    ``X`` and ``sc``: as ``markers.group_moments`` takes them (a device tensor with unit column stride or a
    ``device.PresentedCounts``; host size factors per cell in plan order).  ``labels``: one per cell in plan order as for
    ``markers.encode_labels`` -- the row of ``means`` of the cell, integers as they are, a negative one leaves the cell
    out; None puts every cell in row 0.  ``means``: (K, G) host or device float64, the means at unit size.  ``alpha``,
    ``beta``: (G,) or (C, G) with C <= 16.  ``out``: "numpy", or "torch" for device tensors.  Runs on the current stream.

    Raises TypeError for a host matrix or another dtype; ValueError for a CPU tensor, shapes that do not fit, C > 16, a bad
    ``out``, and for each bit of the pass's status word, with the bit named: a negative count (NEGATIVE), a label that is
    not below K (LABEL), an inadmissible or non-finite parameter (PARAMETER), a size factor that is not positive and finite
    (SIZE), a negative or non-finite mean (MEAN); size factors and means above 1e150 count as not finite."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    m = _device.CountMatrix(X, "fit.loglik")
    alpha, beta = _parameters(alpha, beta, m.G)
    return _Pass(m, sc, _codes(labels, m.N), means, "fit.loglik")(alpha, beta, out)


# ------------------------------------------------------------------------------------------------------ the optimiser

def _check_free(free):
    free = (free,) if isinstance(free, str) else tuple(free)
    if not free or len(set(free)) != len(free) or any(p not in PARAMETERS for p in free):
        raise ValueError("free must name 'alpha', 'beta' or both, once each (got %r)" % (free,))
    return tuple(p for p in PARAMETERS if p in free)


def _check_options(free, alpha0, beta0, fixed_alpha, fixed_beta, bounds, tol, max_rounds):
    free = _check_free(free)
    try:
        lo, hi = (float(b) for b in bounds)
    except (TypeError, ValueError):
        raise ValueError("bounds must be a pair (low, high) of log values (got %r)" % (bounds,)) from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("bounds must be finite with low < high (got %r)" % (bounds,))
    if not (np.isfinite(tol) and tol > 0):
        raise ValueError("tol must be positive (got %r)" % (tol,))
    if isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or max_rounds < 1:
        raise ValueError("need an integer max_rounds >= 1 (got %r)" % (max_rounds,))
    if "alpha" in free and not np.all(np.asarray(alpha0, dtype=np.float64) > 0):
        raise ValueError("alpha0 must be positive")
    if "beta" in free and not np.all(np.asarray(beta0, dtype=np.float64) > 1):
        raise ValueError("beta0 must be above 1")
    if "alpha" not in free and not (np.isfinite(fixed_alpha) and fixed_alpha >= 0):
        raise ValueError("fixed_alpha must be finite and >= 0 (got %r)" % (fixed_alpha,))
    if "beta" not in free and not (np.isfinite(fixed_beta) and fixed_beta >= 1):
        raise ValueError("fixed_beta must be finite and >= 1 (got %r)" % (fixed_beta,))
    return free, lo, hi


class Maximum(NamedTuple):
    """What ``maximize`` returns, per gene: ``u`` = log alpha and ``v`` = log(beta - 1) at the best point seen (NaN for a
    fixed parameter), ``alpha``, ``beta``, ``value`` (the callable's value there), ``rounds`` (until the gene converged),
    ``converged``, ``at_bound`` (a free coordinate ended on the box)."""
    u: np.ndarray
    v: np.ndarray
    alpha: np.ndarray
    beta: np.ndarray
    value: np.ndarray
    rounds: np.ndarray
    converged: np.ndarray
    at_bound: np.ndarray


class _Coordinates:
    """(u, v) -> (alpha, beta) for the free parameters; a fixed one keeps its value."""

    def __init__(self, free, fixed_alpha, fixed_beta):
        self.free_u, self.free_v = "alpha" in free, "beta" in free
        self.fixed_alpha, self.fixed_beta = float(fixed_alpha), float(fixed_beta)

    def alpha(self, u):
        return np.exp(u) if self.free_u else np.full(u.shape, self.fixed_alpha)

    def beta(self, v):
        return 1.0 + np.exp(v) if self.free_v else np.full(v.shape, self.fixed_beta)


# the stencil in units of h: the centre first, so that a tie stays at the centre
_STENCIL_2 = np.array([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)], dtype=np.float64)
_STENCIL_1 = np.array([(0, 0), (-1, 0), (1, 0)], dtype=np.float64)


def _stencil(cu, cv, h, co, lo, hi):
    """(U, V, whole): the stencil's points (P, G), clipped to the box, and per gene whether none was clipped."""
    if co.free_u and co.free_v:
        du, dv = _STENCIL_2[:, 0], _STENCIL_2[:, 1]
    elif co.free_u:
        du, dv = _STENCIL_1[:, 0], _STENCIL_1[:, 1]
    else:
        du, dv = _STENCIL_1[:, 1], _STENCIL_1[:, 0]
    U = cu[None, :] + du[:, None] * h[None, :]
    V = cv[None, :] + dv[:, None] * h[None, :]
    Uc, Vc = np.clip(U, lo, hi), np.clip(V, lo, hi)
    whole = np.all(Uc == U, axis=0) & np.all(Vc == V, axis=0)
    return Uc, Vc, whole


def _derivatives(F, h, co):
    """(gu, gv, huu, huv, hvv) by central differences of a stencil's values F (P, G) of step h (G,)."""
    zero = np.zeros(F.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        if co.free_u and co.free_v:
            gu = (F[2] - F[1]) / (2 * h)
            gv = (F[4] - F[3]) / (2 * h)
            huu = (F[2] - 2 * F[0] + F[1]) / (h * h)
            hvv = (F[4] - 2 * F[0] + F[3]) / (h * h)
            huv = (F[8] - F[7] - F[6] + F[5]) / (4 * h * h)
            return gu, gv, huu, huv, hvv
        g = (F[2] - F[1]) / (2 * h)
        hh = (F[2] - 2 * F[0] + F[1]) / (h * h)
    return (g, zero, hh, zero, zero) if co.free_u else (zero, g, zero, zero, hh)


def _newton_step(F, h, co):
    """(su, sv, ok): the Newton step from a stencil's central differences, cut to 2 h per coordinate; ok where the Hessian
    is negative definite and the step finite."""
    gu, gv, huu, huv, hvv = _derivatives(F, h, co)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if co.free_u and co.free_v:
            det = huu * hvv - huv * huv
            ok = (huu < 0) & (hvv < 0) & (det > 0)
            su = -(hvv * gu - huv * gv) / det
            sv = -(huu * gv - huv * gu) / det
        elif co.free_u:
            ok, su, sv = huu < 0, -gu / huu, np.zeros(h.shape)
        else:
            ok, su, sv = hvv < 0, np.zeros(h.shape), -gv / hvv
    ok = ok & np.isfinite(su) & np.isfinite(sv)
    su = np.where(ok, np.clip(su, -2 * h, 2 * h), 0.0)
    sv = np.where(ok, np.clip(sv, -2 * h, 2 * h), 0.0)
    return su, sv, ok


def maximize(evaluate, n_genes, *, free=("alpha", "beta"), alpha0=0.1, beta0=2.0, fixed_alpha=0.0, fixed_beta=1.0,
             bounds=(-12.0, 4.0), tol=1e-4, max_rounds=60):
    """Per gene the (alpha, beta) that maximise ``evaluate(alpha (C, G), beta (C, G)) -> (C, G)``: ``Maximum``.

    Works in u = log alpha, v = log(beta - 1) inside the box ``bounds`` (for both coordinates), from (``alpha0``, ``beta0``)
    (scalars or one per gene); a parameter that is not in ``free`` stays at ``fixed_alpha`` / ``fixed_beta``.  Each round
    evaluates, in ONE call, per gene a 3 x 3 stencil of step h around the centre (3 points with one free parameter) and
    one quasi-Newton point: the Newton step from the previous round's stencil by central differences, where its Hessian
    is negative definite and no point of it was clipped, cut to 2 h per coordinate and clipped to the box (C = 10, or 4).
    The centre moves to the best point seen (ties to the lowest candidate index, the centre first); h starts at 1, is
    halved when the centre stays or moves by less than h / 2, and doubled (never past 1) when the centre has moved by a
    full step or more two rounds running -- a centre that creeps along a flat ridge towards the box at a small h would
    otherwise use up ``max_rounds``; a gene has converged when h < ``tol``, and is left alone from then on.  A NaN value counts as minus infinity.  Deterministic."""
    free, lo, hi = _check_options(free, alpha0, beta0, fixed_alpha, fixed_beta, bounds, tol, max_rounds)
    G = int(n_genes)
    co = _Coordinates(free, fixed_alpha, fixed_beta)
    with np.errstate(divide="ignore", invalid="ignore"):
        cu = np.clip(np.broadcast_to(np.log(np.asarray(alpha0, dtype=np.float64)), (G,)), lo, hi).copy() if co.free_u else np.zeros(G)
        cv = np.clip(np.broadcast_to(np.log(np.asarray(beta0, dtype=np.float64) - 1.0), (G,)), lo, hi).copy() if co.free_v else np.zeros(G)
    h = np.ones(G)
    best = np.full(G, -np.inf)
    rounds = np.zeros(G, dtype=np.int64)
    done = np.zeros(G, dtype=bool)
    streak = np.zeros(G, dtype=np.int64)
    qu, qv = cu.copy(), cv.copy()                  # the quasi-Newton point; the centre itself while there is none
    for _ in range(int(max_rounds)):
        if done.all():
            break
        U, V, whole = _stencil(cu, cv, h, co, lo, hi)
        U, V = np.vstack([U, qu[None, :]]), np.vstack([V, qv[None, :]])
        F = np.asarray(evaluate(co.alpha(U), co.beta(V)), dtype=np.float64)
        if F.shape != U.shape:
            raise ValueError("evaluate must return %s values, not %s" % (U.shape, F.shape))
        F = np.where(np.isnan(F), -np.inf, F)
        pick = np.argmax(F, axis=0)                # the first of equal maxima
        cols = np.arange(G)
        nu, nv, nf = U[pick, cols], V[pick, cols], F[pick, cols]
        su, sv, ok = _newton_step(F[:-1], h, co)
        ok &= whole
        move = ~done
        step = np.maximum(np.abs(nu - cu), np.abs(nv - cv))
        halve = move & (step < h / 2)
        # the next quasi-Newton point is laid from THIS stencil's centre
        qu_next = np.where(ok, np.clip(cu + su, lo, hi), nu)
        qv_next = np.where(ok, np.clip(cv + sv, lo, hi), nv)
        cu, cv = np.where(move, nu, cu), np.where(move, nv, cv)
        best = np.where(move, nf, best)
        qu, qv = np.where(move, qu_next, cu), np.where(move, qv_next, cv)
        # a centre that moved by a full step twice running is far from the top: the step grows again (never past 1)
        streak = np.where(move & (step >= h), streak + 1, 0)
        grow = streak >= 2
        h = np.where(halve, h / 2, np.where(grow, np.minimum(2 * h, 1.0), h))
        streak = np.where(grow, 0, streak)
        rounds = rounds + move
        done = done | (h < tol)
    at_bound = np.zeros(G, dtype=bool)
    if co.free_u:
        at_bound |= (cu <= lo) | (cu >= hi)
    if co.free_v:
        at_bound |= (cv <= lo) | (cv >= hi)
    return Maximum(np.where(co.free_u, cu, np.nan), np.where(co.free_v, cv, np.nan), co.alpha(cu), co.beta(cv), best,
                   rounds, done, at_bound)


# ----------------------------------------------------------------------------------------------------- the whole fit

class CountModelFit(NamedTuple):
    """Per gene: ``alpha``, ``beta`` (G,) the estimates; ``loglik`` the full log-likelihood there (``base`` taken off);
    ``rounds``, ``converged``, ``at_bound`` of ``maximize``; ``hessian`` (G, 3): d2/du2, d2/du dv, d2/dv2 of the
    log-likelihood in u = log alpha, v = log(beta - 1) from a stencil of step 1e-2 at the optimum (NaN for a fixed
    parameter); ``se_log_alpha``, ``se_log_beta_minus_1``: from the inverse of the negated Hessian, NaN where it is not
    negative definite or the parameter is fixed; ``means`` (K, G) the means that were used; ``bad`` (G,) int64 the
    entries x > 0 at a mean of 0; ``free``.  A gene with ``bad`` > 0 or without any count has NaN estimates and
    ``converged`` False."""
    alpha: np.ndarray
    beta: np.ndarray
    loglik: np.ndarray
    rounds: np.ndarray
    converged: np.ndarray
    at_bound: np.ndarray
    hessian: np.ndarray
    se_log_alpha: np.ndarray
    se_log_beta_minus_1: np.ndarray
    means: Any
    bad: np.ndarray
    free: tuple


def fit_with(evaluate, n_genes, *, base, bad, has_counts, means=None, free=("alpha", "beta"), alpha0=0.1, beta0=2.0,
             fixed_alpha=0.0, fixed_beta=1.0, bounds=(-12.0, 4.0), tol=1e-4, max_rounds=60):
    """``CountModelFit`` through ``maximize`` of any ``evaluate`` (the device pass, or its numpy model): ``base`` (G,) and
    ``bad`` (G,) of the pass, ``has_counts`` (G,) bool whether the gene has any count above 0."""
    return _fit(evaluate, n_genes, lambda: (base, bad, has_counts), means, free=free, alpha0=alpha0, beta0=beta0,
                fixed_alpha=fixed_alpha, fixed_beta=fixed_beta, bounds=bounds, tol=tol, max_rounds=max_rounds)


def _fit(evaluate, n_genes, sums, means, *, free, alpha0, beta0, fixed_alpha, fixed_beta, bounds, tol, max_rounds):
    """``fit_with``, with (base, bad, has_counts) asked of ``sums()`` once ``evaluate`` has run: the device's first call of the
    optimiser brings base and bad with it."""
    G = int(n_genes)
    mx = maximize(evaluate, G, free=free, alpha0=alpha0, beta0=beta0, fixed_alpha=fixed_alpha, fixed_beta=fixed_beta,
                  bounds=bounds, tol=tol, max_rounds=max_rounds)
    base, bad, has_counts = sums()
    free, lo, hi = _check_options(free, alpha0, beta0, fixed_alpha, fixed_beta, bounds, tol, max_rounds)
    co = _Coordinates(free, fixed_alpha, fixed_beta)
    cu, cv = np.where(co.free_u, mx.u, 0.0), np.where(co.free_v, mx.v, 0.0)
    hs = np.full(G, HESSIAN_STEP)
    U, V, _ = _stencil(cu, cv, hs, co, -np.inf, np.inf)
    F = np.asarray(evaluate(co.alpha(U), co.beta(V)), dtype=np.float64)
    _, _, huu, huv, hvv = _derivatives(F, hs, co)
    nan = np.full(G, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        if co.free_u and co.free_v:
            det = huu * hvv - huv * huv
            ok = (huu < 0) & (hvv < 0) & (det > 0)
            se_u = np.where(ok, np.sqrt(np.where(ok, -hvv / det, 1.0)), np.nan)
            se_v = np.where(ok, np.sqrt(np.where(ok, -huu / det, 1.0)), np.nan)
            hessian = np.stack([huu, huv, hvv], axis=1)
        elif co.free_u:
            se_u, se_v = np.where(huu < 0, np.sqrt(np.where(huu < 0, -1.0 / huu, 1.0)), np.nan), nan
            hessian = np.stack([huu, nan, nan], axis=1)
        else:
            se_u, se_v = nan, np.where(hvv < 0, np.sqrt(np.where(hvv < 0, -1.0 / hvv, 1.0)), np.nan)
            hessian = np.stack([nan, nan, hvv], axis=1)
    bad = np.asarray(bad, dtype=np.int64)
    void = (bad > 0) | ~np.asarray(has_counts, dtype=bool)
    blank = lambda a: np.where(void, np.nan, a)                     # noqa: E731
    hessian = np.where(void[:, None], np.nan, hessian)
    return CountModelFit(blank(mx.alpha), blank(mx.beta), blank(mx.value - np.asarray(base, dtype=np.float64)), mx.rounds,
                         mx.converged & ~void, mx.at_bound & ~void, hessian, blank(se_u), blank(se_v), means, bad, free)


def count_model(X, sc, labels=None, means=None, *, free=("alpha", "beta"), alpha0=0.1, beta0=2.0, fixed_alpha=0.0,
                fixed_beta=1.0, bounds=(-12.0, 4.0), tol=1e-4, max_rounds=60):
    """``CountModelFit`` of an int32 device count matrix: per gene the (alpha, beta) of the count model that maximise the
    likelihood of its counts, given the means.

    ``X``, ``sc``, ``labels``: as for ``loglik``.  ``means``: (K, G) host or device float64 means at unit size, row k for the
    cells of label k; None takes the groups' pseudobulk, ``markers.group_moments(X, sc, labels).pseudobulk(sc)`` (at most
    1024 groups).  ``free`` and the options after it: ``maximize``'s.  With ``free=("alpha",)`` and the default
    ``fixed_beta=1`` this is the textbook negative binomial's dispersion.

    Raises what ``loglik`` and ``maximize`` raise; the argument checks come before any device use."""
    _check_options(free, alpha0, beta0, fixed_alpha, fixed_beta, bounds, tol, max_rounds)
    m = _device.CountMatrix(X, "fit.count_model")
    codes = _codes(labels, m.N)
    one = np.where(codes >= 0, 0, -1)
    if means is None:
        gm = markers.group_moments(X, sc, codes)
        means = gm.pseudobulk(sc)
        if not np.all(np.isfinite(means)):
            raise ValueError("a group has no cells (or size factors that sum to 0): its pseudobulk mean is undefined")
        total = np.asarray(gm.count_sum).sum(axis=0)
    else:
        # whether a gene has any count among the labelled cells: the exact count sums of the grouped pass with every labelled
        # cell in one group (one read of the matrix beside the optimiser's twenty to sixty; the fit library has no such sum)
        total = np.asarray(markers.group_moments(X, sc, one).count_sum).sum(axis=0)
    run = _Pass(m, sc, codes, means, "fit.count_model")
    first = []                                     # the LogLik of the optimiser's first call: base and bad come with it

    def evaluate(alpha, beta):
        ll = run(alpha, beta)
        if not first:
            first.append(ll)
        return ll.values

    return _fit(evaluate, run.m.G, lambda: (first[0].base, first[0].bad, total > 0), _host(run.means), free=free,
                alpha0=alpha0, beta0=beta0, fixed_alpha=fixed_alpha, fixed_beta=fixed_beta, bounds=bounds, tol=tol,
                max_rounds=max_rounds)


def simulation_means(tree):
    """The (sum T_b, G) float64 means of a simulation's tree in the row order of ``simulation.cell_rows``: the binary32
    values the sampler reads, widened.  ``count_model(X, sc, sim.cell_rows(tree, pt, br), simulation_means(tree))`` refits a
    simulation against its true means."""
    return tree.device_means().detach().cpu().numpy().astype(np.float64)


class Hyperparameters(NamedTuple):
    """Mean and standard deviation (ddof 1) of log alpha and of log(beta - 1) over the ``n_genes`` genes that converged
    inside the box: what the reference's notebooks feed to ``np.exp(random.normal(mean, std))``.  NaN for a fixed parameter,
    and the spread of fewer than two genes."""
    log_alpha_mean: float
    log_alpha_std: float
    log_beta_minus_1_mean: float
    log_beta_minus_1_std: float
    n_genes: int


def hyperparameters(f):
    """``Hyperparameters`` of a ``CountModelFit``."""
    if not isinstance(f, CountModelFit):
        raise TypeError("hyperparameters takes a CountModelFit, not %s" % type(f).__name__)
    keep = np.asarray(f.converged, dtype=bool) & ~np.asarray(f.at_bound, dtype=bool)
    n = int(keep.sum())

    def moments(values):
        if n == 0:
            return float("nan"), float("nan")
        return float(np.mean(values)), float(np.std(values, ddof=1)) if n > 1 else float("nan")

    nothing = (float("nan"), float("nan"))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = moments(np.log(f.alpha[keep])) if "alpha" in f.free else nothing
        b = moments(np.log(f.beta[keep] - 1.0)) if "beta" in f.free else nothing
    return Hyperparameters(a[0], a[1], b[0], b[1], n)
