"""
GLM-PCA factors of a count matrix, computed where the matrix lies: on the device.  The low-rank log-bilinear structure the
simulator draws from, log(mean[cell][gene] / s_cell) = b_gene + sum_k scores[cell][k] loadings[gene][k] (Townes et al. 2019),
fitted under the simulator's own variance law (``count_model.get_pr_umi``: variance alpha mu^2 + beta mu):

    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch")
    f = factors.glmpca(X, sc, 5, alpha=a, beta=b)
    f.scores                                                   # (cells, k): what neighbors.knn, ptree and the layouts take
    f.fitted()                                                 # (cells, genes) means at unit size
    f.project(X2, sc2)                                         # scores of other cells against the same loadings

It is ``regress`` with the design unknown, fitted by alternating two regressions.  The gene half is per gene with the design
[1 | scores]: ``regress.normal_equations`` with one design row per cell.  The cell half is per cell with the design
[intercept | loadings] over the genes: ``cell_equations``, the pass of libprosstt_amd_factors.so (include/prosstt_amd_factors.h
holds the definition), which reads the matrix along its rows and keeps a cell's sums in a lane's registers: in binary64, for
every cell and every gene with ``use`` >= 0,

    eta = sum_j L[g][j] C[i][j];  mu = s exp(eta);  d = a mu + b;  w = mu / d;  u = (x - mu) / d
    U[i][j] += L[g][j] u;  I[i][j,k] += (L[g][j] L[g][k]) w
    Q[i] += x = 0 ? -T : (x / b) ((eta + log s) - (log b + L1)) - T;  L1 = log1p(a mu / b);  T = a > 0 ? L1 / a : mu / b

There is no CPU fallback for either pass: host matrices are refused.  The loop (``glmpca_with``) runs on the host in numpy and
knows the device only through two callables, so that it is tested against the numpy model of the passes without a device.
``alpha = 0, beta = 1`` is Townes' Poisson GLM-PCA.
"""
import ctypes
from typing import NamedTuple

import numpy as np

from . import _cellpass, _native, markers, regress
from . import device as _device
from ._cellpass import _check_split, _host, _per_gene
from .device import _ptr, _torch

MAX_P = 16                      # PROSSTT_AMD_FACTORS_MAX_P
MAX_K = MAX_P - 1               # the intercept is one of a half's coefficients
TILE_GENES = 32                 # PROSSTT_AMD_FACTORS_TILE_GENES
# the bits of the pass's status word are regress's, without LABEL; a loading is a coefficient of the other half
NEGATIVE, PARAMETER, SIZE, COEFFICIENT, ETA = regress.NEGATIVE, regress.PARAMETER, regress.SIZE, regress.COEFFICIENT, regress.ETA
STATUS_MESSAGES = tuple((bit, name, "a coefficient or a loading is not finite" if bit == COEFFICIENT else text)
                        for bit, name, text in regress.STATUS_MESSAGES if bit != regress.LABEL)
HALVINGS = 8                    # of a step, while the penalised quasi-log-likelihood falls
# the defaults of ``glmpca``, chosen by tools/factors_calibration.py among penalties 1, 10, 50 (DESIGN section 35 holds the table)
PENALTY = 50.0
MAX_ROUNDS = 30
TOL = 1e-6                      # of the halving rule and of the stop: a round of the alternation gains less and less


def check_status(bits):
    """ValueError naming every bit of the pass's status word that is set."""
    _cellpass.check_status(bits, STATUS_MESSAGES)


def gene_blocks(n_cells, n_genes, genes_per_block=0):
    """(genes per block, blocks): how the pass cuts the genes of an ``n_cells`` x ``n_genes`` matrix.  With
    ``genes_per_block`` = 0 the library's choice (``gene_blocking`` of csrc/factors/factors.hip: about 1024 blocks over the
    blocks of 256 cells and no block longer than about 1024 genes, at least four tiles of 32 genes each, at most 65535
    blocks), a function of (N, G) alone; what ``regress.row_blocks`` is for the other pass.  A cell's terms are added in
    ascending gene order within a block and the blocks' sums in ascending order; tests/factors_model.py adds in the same
    order, and a caller with a matrix in chunks of cells reads here the ``genes_per_block`` to pass to every chunk."""
    n_cells, n_genes, per = int(n_cells), int(n_genes), int(genes_per_block)
    whole = -(-n_genes // TILE_GENES) * TILE_GENES
    if per == 0:
        blocks = max(1024 // -(-n_cells // 256), -(-n_genes // 1024))
        blocks = min(max(blocks, 1), -(-n_genes // (4 * TILE_GENES)), 65535)
        per = -(-(-(-n_genes // blocks)) // TILE_GENES) * TILE_GENES
    per = min(per, whole, 1 << 30)
    return per, -(-n_genes // per)


def packed(full):
    """(N, P2) from (N, p, p): the upper triangle packed by rows, as the pass returns it; the inverse of
    ``CellEquations.symmetric`` (a helper of the tests and of callers that hold symmetric matrices)."""
    j, k = np.triu_indices(full.shape[1])
    return full[:, j, k]


class CellEquations:
    """The sums of one call (or of several chunks of cells, ``concat``), cells in plan order: ``score`` (N, p) the
    quasi-score U; ``information`` (N, P2) the information I, the upper triangle packed by rows (``symmetric()``: (N, p, p));
    ``q`` (N,) the quasi-log-likelihood; ``used`` (N,) int64 the entries added; ``n_genes``.  ``score``, ``information`` and
    ``q`` are numpy arrays, or device tensors for ``out="torch"``."""

    def __init__(self, score, information, q, used, n_genes):
        self.score, self.information, self.q = score, information, q
        self.used = np.asarray(used, dtype=np.int64)
        self.n_genes = int(n_genes)
        N = self.used.shape[0]
        p = score.shape[1] if len(score.shape) == 2 else -1
        if p < 1 or score.shape[0] != N or tuple(q.shape) != (N,) or tuple(information.shape) != (N, p * (p + 1) // 2):
            raise ValueError("score must be (cells, p), information (cells, p (p + 1) / 2), q and used (cells,)")

    @property
    def n_cells(self):
        return int(self.score.shape[0])

    @property
    def p(self):
        return int(self.score.shape[1])

    def symmetric(self):
        """(N, p, p): the information as symmetric matrices."""
        info = self.information
        return regress.symmetric(info.T if isinstance(info, np.ndarray) else info.t(), self.p)

    @staticmethod
    def concat(parts):
        """The equations of the cells of all ``parts`` (chunks of one matrix over cells, evaluated against the same loadings
        and parameters): one after the other in list order.  Rows are independent, so with the same ``genes_per_block`` the
        result holds the bits of one call on the whole matrix."""
        parts = list(parts)
        if not parts:
            raise ValueError("concat needs at least one CellEquations")
        for part in parts:
            if not isinstance(part, CellEquations):
                raise TypeError("concat takes CellEquations, not %s" % type(part).__name__)
            if part.p != parts[0].p or part.n_genes != parts[0].n_genes:
                raise ValueError("the parts cover different genes or coefficients")
        if all(isinstance(part.score, np.ndarray) for part in parts):
            cat = np.concatenate
        else:
            cat = _torch().cat
        return CellEquations(cat([part.score for part in parts]), cat([part.information for part in parts]),
                             cat([part.q for part in parts]), np.concatenate([part.used for part in parts]), parts[0].n_genes)

    def __repr__(self):
        return "CellEquations(cells=%d, p=%d, genes=%d)" % (self.n_cells, self.p, self.n_genes)


def _loadings(loadings, n_genes):
    L = np.asarray(_host(loadings))
    if L.ndim != 2 or L.dtype.kind not in "iuf" or L.shape[0] != n_genes or L.shape[1] < 1:
        raise ValueError("loadings must be a (genes, p) = (%d, p) array of numbers, not %s" % (n_genes, L.shape))
    if L.shape[1] > MAX_P:
        raise ValueError("need 1 <= p <= %d coefficients (the loadings have %d columns)" % (MAX_P, L.shape[1]))
    return np.ascontiguousarray(L, dtype=np.float64)


def _cell_coefficients(coef, n_cells, p):
    c = np.asarray(_host(coef), dtype=np.float64)
    if c.shape != (n_cells, p):
        raise ValueError("coef must be (cells, p) = (%d, %d), not %s" % (n_cells, p, c.shape))
    return c


def _use(use, n_genes):
    """int32 per gene, negative: left out; None for every gene.  Booleans: True is in."""
    if use is None:
        return None
    u = np.asarray(_host(use))
    if u.shape != (n_genes,) or u.dtype.kind not in "biu":
        raise ValueError("use must be one integer or boolean per gene: shape (%d,), not %s %s" % (n_genes, u.dtype, u.shape))
    if u.dtype.kind == "b":
        return np.where(u, 0, -1).astype(np.int32)
    return np.where(u < 0, -1, 0).astype(np.int32)


def _check_genes_per_block(genes_per_block):
    g = genes_per_block
    if isinstance(g, (bool, np.bool_)) or not isinstance(g, (int, np.integer)) or g < 0 or g % TILE_GENES:
        raise ValueError("genes_per_block must be 0 (the library's choice) or a multiple of %d (got %r)" % (TILE_GENES, g))
    return int(g)


class _CellPass(_cellpass.SizedPass):
    """The device side of repeated ``cell_equations`` calls over one matrix: the checked matrix view, the size factors on the
    device in row order, and the workspace.  ``__init__`` checks on the host; the first call is the first use of the device."""

    def __init__(self, X, sc, who):
        super().__init__(X, sc, who)
        self.lib, self._ws = None, {}

    def _check_bounds(self, m, who):
        if m.N >= 1 << 31 or m.G >= 1 << 31:
            raise ValueError("%s takes fewer than 2^31 cells and fewer than 2^31 genes" % who)

    def _place(self, p, genes_per_block):
        m, torch = self.m, _torch()
        if self.lib is None:
            self.place_size("factors")
            if m.cell_of_row is not None:
                with torch.cuda.device(m.device):
                    self.row_of_cell = torch.as_tensor(_device.inverse_permutation(m.cell_of_row)).to(m.device)
        if (p, genes_per_block) not in self._ws:
            self._ws = {(p, genes_per_block): m.workspace("factors", "prosstt_amd_factors_workspace_bytes", p, genes_per_block)}
        return self._ws[p, genes_per_block]

    def __call__(self, loadings, coef, alpha, beta, use=None, out="numpy", split=0, genes_per_block=0):
        m = self.m
        N, G = m.N, m.G
        L = _loadings(loadings, G)
        p = L.shape[1]
        coef = _cell_coefficients(coef, N, p)
        alpha, beta = _per_gene(alpha, G, "alpha"), _per_gene(beta, G, "beta")
        use = _use(use, G)
        P2 = p * (p + 1) // 2
        torch = _torch()
        ws = self._place(p, genes_per_block)
        with torch.cuda.device(m.device):
            rows = markers.codes_in_row_order(coef, m.cell_of_row)
            C = torch.as_tensor(np.ascontiguousarray(rows.T)).to(m.device)                  # (p, N)
            par = torch.as_tensor(np.concatenate([alpha[None, :], beta[None, :]])).to(m.device)
            Ld = torch.as_tensor(L).to(m.device)
            used_genes = None if use is None else torch.as_tensor(use).to(m.device)
            sums = torch.empty((p + P2 + 1, N), dtype=torch.float64, device=m.device)        # U, I, then Q
            used = torch.empty(N, dtype=torch.int64, device=m.device)
            status = torch.zeros(1, dtype=torch.int32, device=m.device)
            _native.check(self.lib.prosstt_amd_factors_cell_equations(
                m.stream(), _ptr(m.X), N, G, m.ld, _ptr(self.size), _ptr(used_genes), _ptr(Ld), p, p, _ptr(C), _ptr(par[0]),
                _ptr(par[1]), split, genes_per_block, _ptr(ws), ws.numel(), _ptr(sums[:p]), _ptr(sums[p:p + P2]),
                _ptr(sums[p + P2]), _ptr(used), _ptr(status)), "factors")
            check_status(int(status.item()))
            if m.cell_of_row is not None:                                                   # rows -> cells of the plan
                sums, used = sums.index_select(1, self.row_of_cell), used.index_select(0, self.row_of_cell)
            used = used.cpu().numpy()
            if out == "numpy":
                sums = sums.cpu().numpy()
                return CellEquations(np.ascontiguousarray(sums[:p].T), np.ascontiguousarray(sums[p:p + P2].T), sums[p + P2], used, G)
            return CellEquations(sums[:p].t().contiguous(), sums[p:p + P2].t().contiguous(), sums[p + P2], used, G)


def gene_blocking(n_cells, n_genes):
    """The library's own choice of ``genes_per_block`` for an ``n_cells`` x ``n_genes`` matrix (the ABI's query; needs the
    built library, not a device)."""
    per = ctypes.c_int64(0)
    _native.check(_native.load("factors").prosstt_amd_factors_gene_blocking(int(n_cells), int(n_genes), ctypes.byref(per)), "factors")
    return int(per.value)


def cell_equations(X, sc, loadings, coef, alpha, beta, *, use=None, out="numpy", split=0, genes_per_block=0):
    """``CellEquations`` of an int32 device count matrix at the cells' coefficients ``coef``.

    ``X`` and ``sc``: as ``regress.normal_equations`` takes them (a device tensor with unit column stride or a
    ``device.PresentedCounts``; host size factors per cell in plan order).  ``loadings``: (G, p) numbers with p <= 16, the
    genes' rows of the design.  ``coef``: (N, p), per cell in plan order.  ``alpha``, ``beta``: a number or one per gene.
    ``use``: one integer (negative: the gene is left out) or boolean per gene; None takes every gene.  ``out``: "numpy", or
    "torch" for device tensors.  ``split``: how many sums a block keeps, 0 for the library's choice; the result does not
    depend on it.  ``genes_per_block``: how many genes a block adds one after the other, 0 for the library's choice for this
    matrix or a multiple of 32; the sums' bits depend on it and on nothing else, so a matrix in chunks of cells is one call
    per chunk with the same value and ``CellEquations.concat``.  Runs on the current stream.

    Raises TypeError for a host matrix or another dtype; ValueError for a CPU tensor, shapes that do not fit, p > 16, a bad
    ``out``, ``split`` or ``genes_per_block``, and for each bit of the pass's status word, with the bit named: a negative
    count (NEGATIVE), an inadmissible or non-finite parameter (PARAMETER), a size factor that is not in (0, 1e150] (SIZE), a
    coefficient or loading that is not finite (COEFFICIENT), a linear predictor beyond 700 in size (ETA)."""
    if out not in ("numpy", "torch"):
        raise ValueError("out must be 'numpy' or 'torch'")
    split = _check_split(split)
    genes_per_block = _check_genes_per_block(genes_per_block)
    run = _CellPass(X, sc, "factors.cell_equations")
    L = _loadings(loadings, run.m.G)
    _cell_coefficients(coef, run.m.N, L.shape[1])
    _per_gene(alpha, run.m.G, "alpha"), _per_gene(beta, run.m.G, "beta")
    _use(use, run.m.G)
    return run(L, coef, alpha, beta, use, out, split, genes_per_block)


# ----------------------------------------------------------------------------------------------------- the loop

def _penalised_step(score, information, coef, free, penalty):
    """(I + penalty)^-1 (U - penalty c) per unit over the ``free`` columns (the penalty applies to every free column but an
    intercept, which ``free`` marks with 2); 0 in the other columns.  A singular matrix takes the pseudo-inverse."""
    cols = np.flatnonzero(free > 0)
    lam = np.where(free[cols] == 1, float(penalty), 0.0)
    A = information[:, cols][:, :, cols] + np.diag(lam)[None, :, :]
    rhs = score[:, cols] - lam[None, :] * coef[:, cols]
    step = np.zeros_like(coef)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        step[:, cols] = regress._solve(A, rhs)
    return step


def _half(evaluate, coef, free, penalty, tol, active=None):
    """One penalised Fisher step of every unit (a gene or a cell) of a half: ``evaluate(coef) -> (score, information, q)``
    of host arrays; ``free`` per column 0 (fixed), 1 (penalised) or 2 (free of the penalty).  The step is halved up to 8
    times for the units whose penalised Q fell by more than tol (|Q| + 1); a unit whose Q still falls keeps its
    coefficients.  Returns (coef, penalised q per unit, halvings per unit, -1 for a unit that kept its coefficients)."""
    n = coef.shape[0]
    active = np.ones(n, dtype=bool) if active is None else active
    pen_cols = free == 1

    def penalised(q, c):
        return np.asarray(q, dtype=np.float64) - 0.5 * penalty * np.sum(c[:, pen_cols] ** 2, axis=1)

    score, info, q = evaluate(coef)
    pq = penalised(q, coef)
    step = _penalised_step(np.asarray(score, dtype=np.float64), np.asarray(info, dtype=np.float64), coef, free, penalty)
    lost = active & ~np.all(np.isfinite(step), axis=1)
    step[lost | ~active] = 0.0
    moving = active & ~lost
    t = np.ones(n)
    falls = moving.copy()
    trial, new_pq = coef, pq
    halvings = np.zeros(n, dtype=np.int64)
    for _halving in range(HALVINGS + 1):
        trial = np.where(falls[:, None], coef + t[:, None] * step, trial)
        new_pq = penalised(evaluate(trial)[2], trial)
        with np.errstate(invalid="ignore"):
            falls = moving & ~(new_pq >= pq - tol * (np.abs(pq) + 1.0))          # (a NaN falls)
        if not falls.any():
            break
        t = np.where(falls, t / 2, t)
        halvings = halvings + falls
    taken = moving & ~falls
    return np.where(taken[:, None], trial, coef), np.where(taken, new_pq, pq), np.where(taken | ~active, halvings, -1)


def rotate(scores, loadings, intercept, full=False):
    """(scores, loadings, intercept) with the same linear predictor: the scores centred (the shift goes into the
    intercept), the loadings orthonormal and the scores orthogonal with descending norms -- the SVD of the k x k core of two
    QRs -- and each component's sign by ``embed.pca``'s rule (its largest loading in size is positive, the first on ties).
    ``full``: also (shift (k,), transform (k, k)) with rotated scores = (scores - shift) . transform."""
    shift = scores.mean(axis=0)
    intercept = intercept + loadings @ shift
    centred = scores - shift[None, :]
    Qu, Ru = np.linalg.qr(centred)
    Qv, Rv = np.linalg.qr(loadings)
    A, S, Bt = np.linalg.svd(Ru @ Rv.T)
    scores, loadings = Qu @ (A * S[None, :]), Qv @ Bt.T
    k = loadings.shape[1]
    top = np.argmax(np.abs(loadings), axis=0)
    signs = np.where(loadings[top, np.arange(k)] < 0, -1.0, 1.0)
    scores, loadings = scores * signs[None, :], loadings * signs[None, :]
    if not full:
        return scores, loadings, intercept
    return scores, loadings, intercept, shift, np.linalg.pinv(Ru) @ (A * S[None, :]) * signs[None, :]


class Factors:
    """What ``glmpca`` returns, cells in plan order: ``scores`` (N, k) centred and orthogonal with descending norms;
    ``loadings`` (G, k) orthonormal; ``intercept`` (G,); ``objective`` the penalised quasi-log-likelihood after every round;
    ``rounds``; ``converged``; ``no_counts`` (G,) the genes left out (no count at all: their loadings are 0 and their
    intercept the rate of half a count); ``penalty``, ``alpha``, ``beta``, ``tol`` as given; ``shift`` (k,) and ``transform``
    (k, k): scores = (the loop's own scores - shift) . transform.  The penalty is not invariant under the rotation, so
    ``project`` works in the loop's own coordinates (``raw()``), where its result for the training cells is one more cell
    half of the loop."""

    def __init__(self, scores, loadings, intercept, objective, rounds, converged, no_counts, penalty, alpha, beta, tol, shift=None,
                 transform=None, project=None):
        self.scores, self.loadings, self.intercept = scores, loadings, intercept
        self.objective = np.asarray(objective, dtype=np.float64)
        self.rounds, self.converged, self.no_counts = int(rounds), bool(converged), no_counts
        self.penalty, self.alpha, self.beta, self.tol = float(penalty), alpha, beta, float(tol)
        k = scores.shape[1]
        self.shift = np.zeros(k) if shift is None else shift
        self.transform = np.eye(k) if transform is None else transform
        self._project, self._fitted = project, None

    def raw_scores(self, scores):
        """Scores in the loop's own coordinates from rotated ones."""
        return scores @ np.linalg.pinv(self.transform) + self.shift[None, :]

    def rotated_scores(self, raw):
        """Rotated scores from ones in the loop's own coordinates."""
        return (raw - self.shift[None, :]) @ self.transform

    def raw(self):
        """(scores, loadings, intercept) in the loop's own coordinates: the same linear predictor, before ``rotate``."""
        loadings = self.loadings @ self.transform.T
        return self.raw_scores(self.scores), loadings, self.intercept - loadings @ self.shift

    @property
    def k(self):
        return int(self.scores.shape[1])

    def linear_predictor(self):
        """(N, G): intercept + scores . loadings', the logarithm of the means at unit size."""
        return self.intercept[None, :] + self.scores @ self.loadings.T

    def fitted(self):
        """(N, G) means at unit size, exp(linear_predictor()); computed at the first call and kept."""
        if self._fitted is None:
            with np.errstate(over="ignore"):
                self._fitted = np.exp(self.linear_predictor())
        return self._fitted

    def project(self, X2, sc2, *, start=None, max_rounds=MAX_ROUNDS, split=0, genes_per_block=0, history=None):
        """(N2, k) scores of the cells of another int32 device count matrix over the same genes, against these loadings and
        this intercept: the cell half alone, a concave problem per cell, from ``start`` (zeros in the loop's coordinates)
        until no cell's penalised Q changes by more than tol (|Q| + 1) or ``max_rounds`` halves.  For a matrix in chunks of
        cells, call it per chunk.  ``history``: ``project_with``'s."""
        if self._project is None:
            raise RuntimeError("these Factors were not fitted on a device: use project_with")
        evaluate, n_cells = self._project(X2, sc2, split, genes_per_block)
        return self.project_with(evaluate, n_cells, start=start, max_rounds=max_rounds, history=history)

    def project_with(self, evaluate, n_cells, *, start=None, max_rounds=MAX_ROUNDS, history=None):
        """``project`` through any ``evaluate(loadings (G, k + 1), coef (N2, k + 1)) -> CellEquations``.  ``history`` (a test
        hook): a list that takes one ``ProjectRound`` per half, in the loop's own coordinates."""
        regress._check_options(max_rounds, self.tol, 700.0)
        k = self.k
        coef = np.zeros((n_cells, k + 1))
        coef[:, 0] = 1.0
        if start is not None:
            start = np.asarray(start, dtype=np.float64)
            if start.shape != (n_cells, k):
                raise ValueError("start must be (cells, k) = (%d, %d), not %s" % (n_cells, k, start.shape))
            coef[:, 1:] = self.raw_scores(start)
        _, loadings, intercept = self.raw()
        L = np.concatenate([intercept[:, None], loadings], axis=1)
        free = np.array([0] + [1] * k)
        active = np.ones(n_cells, dtype=bool)
        pq = None
        for _ in range(int(max_rounds)):
            before = coef[:, 1:].copy()
            coef, new_pq, halvings = _half(lambda c: _cell_sums(evaluate(L, c)), coef, free, self.penalty, self.tol, active)
            if history is not None:
                history.append(ProjectRound(halvings, before, coef[:, 1:].copy()))
            if pq is not None:
                active = active & ~(np.abs(new_pq - pq) <= self.tol * (np.abs(new_pq) + 1.0))
            pq = new_pq
            if not active.any():
                break
        return self.rotated_scores(coef[:, 1:])

    def __repr__(self):
        return "Factors(cells=%d, genes=%d, k=%d, rounds=%d%s)" % (self.scores.shape[0], self.loadings.shape[0], self.k, self.rounds,
                                                                   ", converged" if self.converged else "")


def _cell_sums(eq):
    return np.asarray(eq.score), np.asarray(eq.symmetric()), np.asarray(eq.q)


def _gene_sums(ne):
    return np.asarray(ne.score), np.asarray(ne.information), np.asarray(ne.q)


class Round(NamedTuple):
    """A test hook, no part of the interface: one round's bookkeeping, the halvings per gene and per cell (-1: the unit kept
    its coefficients)."""
    gene_halvings: np.ndarray
    cell_halvings: np.ndarray


class ProjectRound(NamedTuple):
    """A test hook, no part of the interface: one half of ``project_with``, the halvings per cell (-1: the cell kept its
    coefficients) and the scores before and after it in the loop's own coordinates."""
    halvings: np.ndarray
    before: np.ndarray
    after: np.ndarray


def half_round(gene_evaluate, cell_evaluate, scores, loadings, intercept, no_counts, penalty, tol, which):
    """A test hook, no part of the interface (``glmpca_with`` is built on it, and the tests take one half from a state of their
    own).  One half of a round from a given state: ``which`` "genes" returns (intercept, loadings, halvings, penalised q per gene),
    "cells" returns (scores, halvings, penalised q per cell)."""
    k = scores.shape[1]
    if which == "genes":
        coef = np.concatenate([intercept[:, None], loadings], axis=1)
        coef, pq, halvings = _half(lambda c: _gene_sums(gene_evaluate(scores, c)), coef, np.array([2] + [1] * k), penalty, tol,
                                   ~no_counts)
        return coef[:, 0], coef[:, 1:], halvings, pq
    coef = np.concatenate([np.ones((scores.shape[0], 1)), scores], axis=1)
    L = np.concatenate([intercept[:, None], loadings], axis=1)
    coef, pq, halvings = _half(lambda c: _cell_sums(cell_evaluate(L, c)), coef, np.array([0] + [1] * k), penalty, tol)
    return coef[:, 1:], halvings, pq


def start_intercept(totals, size_total):
    """(G,): log(sum x / sum s) per gene; a gene without counts starts (and stays) at the rate of half a count, as
    ``regress.start_coefficients`` has it."""
    return np.log(np.maximum(np.asarray(totals, dtype=np.float64), 0.5) / float(size_total))


def glmpca_with(gene_evaluate, cell_evaluate, scores, loadings, totals, size_total, *, penalty=PENALTY, max_rounds=MAX_ROUNDS,
                tol=TOL, history=None):
    """The GLM-PCA loop through any ``gene_evaluate(scores (N, k), coef (G, k + 1)) -> NormalEquations`` (the gene half: the
    design is [1 | scores], one row per cell) and ``cell_evaluate(loadings (G, k + 1), coef (N, k + 1)) -> CellEquations``
    (the cell half: loading column 0 is the intercept, whose coefficient is fixed at 1) with host arrays: the device passes,
    or their numpy models.  ``scores`` (N, k) and ``loadings`` (G, k): the start; ``totals`` (G,): the genes' count sums;
    ``size_total``: the sum of the size factors.  Both evaluators leave the genes without counts out of the cells' sums.

    The objective is sum Q - (penalty / 2) (|scores|^2 + |loadings|^2); intercepts are free.  A round is a gene half and then
    a cell half, each one penalised Fisher step (I + penalty)^-1 (U - penalty c), halved up to 8 times for the genes or cells
    whose penalised Q fell by more than tol (|Q| + 1).  The loop stops when a round changes the objective by at most
    tol (|objective| + 1).  Returns (scores, loadings, intercept, objective per round, converged, no_counts), not rotated;
    ``history``: a list that takes one ``Round`` per round.  Deterministic."""
    regress._check_options(max_rounds, tol, 700.0)
    if not (np.isfinite(penalty) and penalty >= 0):
        raise ValueError("penalty must be finite and not negative (got %r)" % (penalty,))
    totals = np.asarray(totals, dtype=np.float64)
    scores, loadings = np.array(scores, dtype=np.float64), np.array(loadings, dtype=np.float64)
    no_counts = ~(totals > 0)
    loadings[no_counts] = 0.0
    intercept = start_intercept(totals, size_total)
    objective, converged, before = [], False, None
    for _ in range(int(max_rounds)):
        new_b, new_l, gh, gq = half_round(gene_evaluate, cell_evaluate, scores, loadings, intercept, no_counts, penalty, tol, "genes")
        intercept, loadings = np.where(no_counts, intercept, new_b), np.where(no_counts[:, None], 0.0, new_l)
        scores, ch, cq = half_round(gene_evaluate, cell_evaluate, scores, loadings, intercept, no_counts, penalty, tol, "cells")
        value = float(np.sum(cq) - 0.5 * penalty * np.sum(loadings ** 2))
        objective.append(value)
        if history is not None:
            history.append(Round(gh, ch))
        if before is not None and abs(value - before) <= tol * (abs(value) + 1.0):
            converged = True
            break
        before = value
    return scores, loadings, intercept, np.array(objective), converged, no_counts


def _check_k(k, n_cells, n_genes):
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError("need an integer 1 <= k <= %d factors (got %r)" % (MAX_K, k))
    if k >= min(n_cells, n_genes):
        raise ValueError("k = %d factors need more than %d cells and genes (got %d x %d)" % (k, k, n_cells, n_genes))
    return int(k)


def glmpca(X, sc, k=10, *, alpha, beta, penalty=PENALTY, init="pca", seed=0, max_rounds=MAX_ROUNDS, tol=TOL, split=0):
    """``Factors`` of an int32 device count matrix: k GLM-PCA factors under the count model's variance law with the given
    ``alpha`` and ``beta`` (a number or one per gene; ``fit.count_model`` estimates them; 0 and 1 are the Poisson GLM-PCA).

    ``X`` and ``sc``: as ``cell_equations`` takes them.  ``k``: 1 .. 15.  ``penalty``: of the squared scores and loadings.
    ``init``: "pca" (``embed.pca``'s scores and loadings, each scaled by the square root of the singular value), an (N, k)
    array of scores (the loadings start at 0), or "random" (normal scores of standard deviation 0.1 by ``seed``).
    ``max_rounds``, ``tol``: ``glmpca_with``'s.  Every round is at least four passes over the matrix (two per half, more when a
    step is halved); the loop itself runs on the host.

    Raises what ``cell_equations`` and ``regress.normal_equations`` raise; the argument checks come before any device use."""
    regress._check_options(max_rounds, tol, 700.0)
    split = _check_split(split)
    if not (np.isfinite(penalty) and penalty >= 0):
        raise ValueError("penalty must be finite and not negative (got %r)" % (penalty,))
    cells = _CellPass(X, sc, "factors.glmpca")
    m = cells.m
    N, G = m.N, m.G
    k = _check_k(k, N, G)
    alpha, beta = _per_gene(alpha, G, "alpha"), _per_gene(beta, G, "beta")
    s = cells._sc
    loadings = np.zeros((G, k))
    if isinstance(init, str):
        if init not in ("pca", "random"):
            raise ValueError("init must be 'pca', 'random' or an (N, k) array of scores (got %r)" % (init,))
        if init == "random":
            scores = 0.1 * np.random.default_rng(seed).standard_normal((N, k))
    else:
        scores = np.asarray(_host(init), dtype=np.float64)
        if scores.shape != (N, k) or not np.all(np.isfinite(scores)):
            raise ValueError("init must be 'pca', 'random' or a finite (N, k) = (%d, %d) array of scores" % (N, k))
    if isinstance(init, str) and init == "pca":
        from . import embed
        pca = embed.pca(X, s, k)
        root = np.sqrt(pca.singular_values)
        scores, loadings = pca.scores / root[None, :], pca.components.T * root[None, :]
    totals = np.asarray(markers.group_moments(X, s, np.zeros(N, dtype=np.int64)).count_sum).sum(axis=0)
    no_counts = ~(totals > 0)
    use = np.where(no_counts, -1, 0)
    genes = regress._Pass(m, s, np.arange(N), np.concatenate([np.ones((N, 1)), scores], axis=1), "factors.glmpca")

    def gene_evaluate(sco, coef):
        genes.set_design(np.concatenate([np.ones((N, 1)), sco], axis=1))
        return genes(coef, alpha, beta, False, "numpy", split)

    def cell_evaluate(L, coef):
        return cells(L, coef, alpha, beta, use, "numpy", split, 0)

    scores, loadings, intercept, objective, converged, no_counts = glmpca_with(
        gene_evaluate, cell_evaluate, scores, loadings, totals, float(s.sum()), penalty=penalty, max_rounds=max_rounds, tol=tol)
    scores, loadings, intercept, shift, transform = rotate(scores, loadings, intercept, full=True)

    def project(X2, sc2, split2, genes_per_block):
        split2, genes_per_block = _check_split(split2), _check_genes_per_block(genes_per_block)
        other = _CellPass(X2, sc2, "factors.project")
        if other.m.G != G:
            raise ValueError("factors.project needs the %d genes of the fit (got %d)" % (G, other.m.G))
        return (lambda L, coef: other(L, coef, alpha, beta, use, "numpy", split2, genes_per_block)), int(other.m.N)

    return Factors(scores, loadings, intercept, objective, len(objective), converged, no_counts, penalty, alpha, beta, tol, shift, transform,
                   project)
