"""The checking model of prosstt_amd/hvg.py: plain numpy and pandas on the whole matrix, written the slow and obvious way --
``np.minimum(X, clip)`` in binary64 for the clip, one ``np.linalg.lstsq`` per gene for the loess, ``pd.cut`` and ``groupby`` for
the bins.  Every function also takes the sums it would form itself, so that a test can feed it the device's and compare
stage by stage."""
import numpy as np
import pandas as pd

# How far prosstt_amd.hvg.loess_fit (normal equations in u / h, solved by a pseudo-inverse) may lie from ``loess`` below (one
# lstsq per gene), as |a - b| <= LOESS_TOL * max(1, |b|).  Measured on the host: 8.0e-15 at 300 genes and 2.0e-14 at 1100
# genes (the two inputs of tests/test_gpu_hvg.py's whole calls), 1.5e-15 and 3.3e-15 on the two tie-heavy inputs of
# tests/test_hvg_host.py; 16 x the largest, as headroom for other numpy / BLAS builds and for the device's sums (with those
# on an MI355X: 1.3e-14 and 4.45e-14 on the two inputs).
LOESS_MEASURED = 2.0e-14
LOESS_TOL = 16 * LOESS_MEASURED


def within_loess_tol(a, b):
    """The largest |a - b| / max(1, |b|), for the assertion against LOESS_TOL."""
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))


def loess(x, y, span=0.3):
    """The local quadratic fit of y on x at every x: q nearest neighbours, tricube weights, least squares on (1, u, u^2)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = x.size
    q = min(n, max(3, int(np.floor(span * n + 1e-5))))
    out = np.empty(n)
    for i in range(n):
        u = x - x[i]
        d = np.abs(u)
        h = np.partition(d, q - 1)[q - 1]
        if h == 0:
            out[i] = y[d == 0].mean()
            continue
        w = np.where(d < h, (1.0 - (d / h) ** 3) ** 3, 0.0)
        keep = w > 0
        r = np.sqrt(w[keep])
        A = np.stack([np.ones(keep.sum()), u[keep], u[keep] ** 2], axis=1) * r[:, None]
        out[i] = np.linalg.lstsq(A, y[keep] * r, rcond=None)[0][0]
    return out


def top(score, n_top):
    """Mask of the n_top largest scores: NaN last, ties to the lower index."""
    key = np.where(np.isnan(score), -np.inf, score)
    order = np.lexsort((np.arange(score.size), -key))[:n_top]
    mask = np.zeros(score.size, dtype=bool)
    mask[order] = True
    return mask


def gap(score, mask):
    """The distance between the last selected and the first unselected score."""
    return float(np.min(score[mask]) - np.max(score[~mask]))


def count_moments(X):
    Xf = np.asarray(X, dtype=np.float64)
    return Xf.mean(axis=0), Xf.var(axis=0, ddof=1)


def seurat_v3_fit(mean, var, n_cells, span=0.3):
    """(reg_std, clip) from the genes' mean and ddof-1 variance."""
    varying = var > 0
    reg_std = np.ones(mean.shape)
    reg_std[varying] = np.sqrt(10.0 ** loess(np.log10(mean[varying]), np.log10(var[varying]), span))
    return reg_std, reg_std * np.sqrt(n_cells) + mean


def clipped_moments(X, clip):
    """(sum, sum of squares) per gene of np.minimum(X, clip) in binary64: the clip route."""
    C = np.minimum(np.asarray(X, dtype=np.float64), clip[None, :])
    return C.sum(axis=0), (C * C).sum(axis=0)


def variances_norm(n_cells, mean, var, reg_std, sum_c, sq_c):
    vn = (n_cells * mean ** 2 + sq_c - 2.0 * sum_c * mean) / ((n_cells - 1) * reg_std ** 2)
    vn[~(var > 0)] = 0.0
    return vn


def seurat_v3(X, n_top, span=0.3, clip=True):
    """dict of every stage of the "seurat_v3" flavour on the whole matrix; clip=False: no clipping (clip = inf)."""
    n = X.shape[0]
    mean, var = count_moments(X)
    reg_std, c = seurat_v3_fit(mean, var, n, span)
    if not clip:
        c = np.full(c.shape, np.inf)
    sum_c, sq_c = clipped_moments(X, c)
    vn = variances_norm(n, mean, var, reg_std, sum_c, sq_c)
    return dict(mean=mean, var=var, reg_std=reg_std, clip=c, variances_norm=vn, mask=top(vn, n_top))


def normalized(X, size_factors):
    """y = float32(x) * float32(1 / s) as binary64: the device's products to the bit."""
    inv = (1.0 / np.asarray(size_factors, dtype=np.float64)).astype(np.float32)
    return (np.asarray(X).astype(np.float32) * inv[:, None]).astype(np.float64)


def seurat(s1, s2, n_cells, n_top=None, n_bins=20, min_mean=0.0125, max_mean=3.0, min_disp=0.5, max_disp=np.inf):
    """dict of every stage of the "seurat" flavour from the per-gene sums of y and y^2."""
    s1 = np.asarray(s1, dtype=np.float64)
    mean = s1 / n_cells
    var = np.maximum(0.0, (np.asarray(s2, dtype=np.float64) - s1 * mean) / (n_cells - 1))
    mean_d = mean.copy()
    mean_d[mean_d == 0] = 1e-12
    with np.errstate(divide="ignore", invalid="ignore"):
        disp = var / mean_d
        disp[disp == 0] = np.nan
        disp = np.log(disp)
    m = np.log1p(mean_d)
    df = pd.DataFrame(dict(m=m, d=disp))
    df["bin"] = pd.cut(df["m"], bins=n_bins)
    grouped = df.groupby("bin", observed=False)["d"]
    mean_bin, std_bin = grouped.mean(), grouped.std(ddof=1)
    lone = std_bin.isnull()
    std_bin[lone] = mean_bin[lone]
    mean_bin[lone] = 0
    dn = (df["d"].values - mean_bin[df["bin"].values].values) / std_bin[df["bin"].values].values
    if n_top is not None:
        mask = top(dn, n_top)
    else:
        with np.errstate(invalid="ignore"):
            mask = (m > min_mean) & (m < max_mean) & (dn > min_disp) & (dn < max_disp)
    return dict(mean=mean, var=var, dispersions=disp, dispersions_norm=dn, mask=mask)


def tie_heavy(kind):
    """(x, y) with heavy ties in x: log10 of means S1 / N with small integer S1; "flat": more than a span's worth of equal
    x, so that h = 0 there."""
    rng = np.random.default_rng(5)
    S1 = rng.integers(1, 12, size=800) if kind == "ties" else np.r_[np.full(500, 3), rng.integers(1, 40, size=300)]
    x = np.log10(S1 / 400.0)
    return x, 1.1 * x + rng.normal(0.0, 0.1, size=800)


def inputs(which):
    """The two inputs of the whole-call tests: (X, planted genes, n_top, size factors)."""
    n_cells, n_genes, n_top, seed = {"small": (500, 300, 30, 1), "wide": (257, 1100, 100, 2)}[which]
    X, planted = planted_counts(n_cells, n_genes, n_top // 2, seed)
    total = X.sum(axis=1)
    return X, planted, n_top, total / np.median(total)


def planted_counts(n_cells, n_genes, n_planted, seed):
    """(X int32, planted gene indices): negative-binomial counts whose gene means spread over two decades, with planted
    genes whose mean is 6 x higher in half the cells."""
    rng = np.random.default_rng(seed)
    mu = 10.0 ** rng.uniform(-1.0, 1.0, size=n_genes)
    planted = np.sort(rng.choice(n_genes, size=n_planted, replace=False))
    M = np.broadcast_to(mu, (n_cells, n_genes)).copy()
    M[: n_cells // 2, planted] *= 6.0
    r = 2.0
    X = rng.negative_binomial(r, r / (r + M)).astype(np.int32)
    return X, planted
