"""The numpy model of prosstt_amd/fit.py and libprosstt_amd_fit.so (include/prosstt_amd_fit.h holds the definition): the
term of one entry by the same regime split as the device, ``loglik`` with the sum S of the magnitudes of the term's three
parts (what the tolerances of the tests are relative to), and the whole ``count_model`` through ``fit.maximize``.

    mu = s_i m[k][g];  theta = a mu + (b - 1);  inv = 1 / theta;  r = mu inv;  L1 = log1p(theta);  D = -log1p(inv)
    term = (lgd(r, x) - r L1) + x D;  x = 0: -(r L1);  mu = 0: 0, and bad[g] counts the entries with x > 0
    lgd(r, x), 1 <= x <= 12:  log(prod_{j < x} (r + j)), or x log r when r > 1e17
    lgd(r, x), x > 12:        k = ceil(16 - r) for r < 16, else 0;  P = prod_{j < k} (r + j);  z = r + k;  n = x - k;  t = z + n
                              n log t + ((z - 1/2) log1p(n / z) - n) + (S(t) - S(z)) + log P
    S(t) = u (1/12 - u^2 (1/360 - u^2 (1/1260 - u^2 (1/1680 - u^2 / 1188)))),  u = 1 / t
"""
import numpy as np

from prosstt_amd import fit

# How far fit.maximize's likelihood may end below the one scipy's L-BFGS-B reaches on the same function
# (tests/test_fit_model.py measures it: 9.1e-13 with both parameters free, 1.8e-11 with alpha alone): ten times the larger
# measured shortfall, and never above 1e-3.  The shortfall measured is rounding noise (the sum of 3 000 terms of size 1
# to 10 is good to about 1e-11), so this bound sits within an order of magnitude of ordinary rounding: tests/test_gpu_fit.py
# compares the device's and the model's likelihood of 257 cells with it, where the sums alone differ by up to 2e-15 S,
# about 1e-11.  Another numpy, libm or ROCm may move either figure by a few units of that size; a failure by a factor
# of two or three there is that, not a worse optimum -- the rule for the bound is the one stated above all the same.
OPTIMISER_BOUND = 1.8e-10


def stirling(t):
    u = 1.0 / t
    u2 = u * u
    s = 1.0 / 1680.0 - u2 * (1.0 / 1188.0)
    s = 1.0 / 1260.0 - u2 * s
    s = 1.0 / 360.0 - u2 * s
    s = 1.0 / 12.0 - u2 * s
    return u * s


def lgd(r, x):
    """lgamma(r + x) - lgamma(r) for r > 0 and integers x >= 0, elementwise (0 where x = 0)."""
    r, x = np.broadcast_arrays(np.asarray(r, dtype=np.float64), np.asarray(x, dtype=np.int64))
    out = np.zeros(r.shape)
    small = (x >= 1) & (x <= 12)
    if small.any():
        rs, xs = r[small], x[small]
        p = rs.copy()
        for j in range(1, 12):
            p = np.where(j < xs, p * (rs + j), p)
        huge = rs > 1e17
        with np.errstate(over="ignore"):
            out[small] = np.where(huge, xs * np.log(rs), np.log(np.where(huge, 1.0, p)))
    big = x > 12
    if big.any():
        rb, xb = r[big], x[big]
        k = np.where(rb < 16.0, np.ceil(16.0 - np.minimum(rb, 16.0)), 0.0).astype(np.int64)
        p = np.ones(rb.shape)
        for j in range(16):
            p = np.where(j < k, p * (rb + j), p)
        z = rb + k
        n = (xb - k).astype(np.float64)
        t = z + n
        main = n * np.log(t) + ((z - 0.5) * np.log1p(n / z) - n)
        out[big] = (main + (stirling(t) - stirling(z))) + np.log(p)
    return out


def term(mu, x, a, bm1):
    """(term, magnitude) of entries with mu > 0 and x >= 0, elementwise: magnitude = |lgd| + r L1 + x |D|."""
    mu, x, a, bm1 = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(x, dtype=np.int64),
                                        np.asarray(a, dtype=np.float64), np.asarray(bm1, dtype=np.float64))
    theta = a * mu + bm1
    inv = 1.0 / theta
    r = mu * inv
    rl = r * np.log1p(theta)
    d = -np.log1p(inv)
    lg = lgd(r, x)
    xd = x.astype(np.float64) * d
    value = np.where(x == 0, -rl, (lg - rl) + xd)
    return value, np.abs(lg) + rl + np.abs(xd)


def log_factorial(x):
    """lgamma(x + 1) as the device forms it: lgd(1, x), 0 for x <= 1."""
    x = np.asarray(x, dtype=np.int64)
    return np.where(x > 1, lgd(np.ones(x.shape), x), 0.0)


def loglik(X, size, labels, means, alpha, beta):
    """(ll (C, G), base (G,), bad (G,) int64, S (C, G)) of host arrays: X (N, G) integers >= 0, size (N,), labels (N,)
    integers (negative: left out), means (K, G), alpha and beta (C, G) or (G,)."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    labels = np.asarray(labels, dtype=np.int64)
    keep = labels >= 0
    X = X[keep]
    mu = np.asarray(size, dtype=np.float64)[keep][:, None] * np.asarray(means, dtype=np.float64)[labels[keep]]
    alpha = np.atleast_2d(np.asarray(alpha, dtype=np.float64))
    beta = np.atleast_2d(np.asarray(beta, dtype=np.float64))
    live = mu > 0
    bad = ((~live) & (X > 0)).sum(axis=0).astype(np.int64)
    base = np.where(live, log_factorial(X), 0.0).sum(axis=0)
    mu1 = np.where(live, mu, 1.0)
    ll = np.empty(alpha.shape)
    S = np.empty(alpha.shape)
    for c in range(alpha.shape[0]):
        value, mag = term(mu1, X, alpha[c][None, :], (beta[c] - 1.0)[None, :])
        ll[c] = np.where(live, value, 0.0).sum(axis=0)
        S[c] = np.where(live, mag, 0.0).sum(axis=0)
    return ll, base, bad, S


def pseudobulk(X, size, labels, n_groups):
    """(K, G): per group the sum of counts over the sum of size factors (markers.GroupMoments.pseudobulk)."""
    X = np.asarray(X, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    keep = labels >= 0
    total = np.bincount(labels[keep], weights=np.asarray(size, dtype=np.float64)[keep], minlength=n_groups)
    sums = np.zeros((n_groups, X.shape[1]))
    np.add.at(sums, labels[keep], X[keep].astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums / total[:, None]


def evaluator(X, size, labels, means):
    """evaluate(alpha (C, G), beta (C, G)) -> (C, G), as ``fit.maximize`` takes it."""
    def evaluate(alpha, beta):
        return loglik(X, size, labels, means, alpha, beta)[0]
    return evaluate


def count_model(X, size, labels=None, means=None, **options):
    """``fit.CountModelFit`` of host arrays: ``fit.count_model`` with the model in place of the device."""
    X = np.asarray(X, dtype=np.int64)
    N, G = X.shape
    labels = np.zeros(N, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    if means is None:
        means = pseudobulk(X, size, labels, int(labels.max()) + 1)
    means = np.asarray(means, dtype=np.float64)
    _, base, bad, _ = loglik(X, size, labels, means, np.full(G, 0.1), np.full(G, 2.0))
    total = X[labels >= 0].sum(axis=0)
    return fit.fit_with(evaluator(X, size, labels, means), G, base=base, bad=bad, has_counts=total > 0, means=means,
                        **options)
