"""Times prosstt_amd.regress on one device: one ``normal_equations`` pass per number of coefficients and per split, beside
``fit.loglik`` with one candidate on the same matrix and (``--torch``) the same sums by torch in binary64 on the same device;
``regression`` end to end with its rounds, and step by step: its setup, its passes and the scoring on the host; and
(``--numpy``) the numpy model of the pass at 5 000 x 2 000.  One JSON line per measurement.

    python tools/regress_bench.py [--cells 50000] [--genes 20000] [--nodes 400] [--reps 5] [--torch] [--numpy]

The matrix is synthetic: ``--nodes`` nodes on a line with a log-mean that drifts along it, Poisson-gamma counts drawn by torch
on the device, a design of p hat functions on the line (rows sum to 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def hats(nodes, p):
    """(nodes, p): hat functions with p knots equally spaced over the nodes; one column of ones for p = 1."""
    if p == 1:
        return np.ones((nodes, 1))
    at = np.arange(nodes) * (p - 1) / max(nodes - 1, 1)
    seg = np.minimum(at.astype(np.int64), p - 2)
    D = np.zeros((nodes, p))
    D[np.arange(nodes), seg] = 1.0 - (at - seg)
    D[np.arange(nodes), seg + 1] += at - seg
    return D


def timed(torch, call, reps):
    """Milliseconds per call by device events: the median of ``reps`` after one warm-up call."""
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times)), float(min(times))


def torch_sums(torch, X, s, labels, D, coef, alpha, beta, chunk=1000):
    """U (G, p) and I (G, P2) by torch in binary64, ``chunk`` genes at a time (two matrix products per chunk)."""
    p = D.shape[1]
    j, k = np.triu_indices(p)
    Dl = D[labels]                                                 # (N, p)
    pairs = Dl[:, j] * Dl[:, k]                                    # (N, P2)
    U, I = [], []
    for g0 in range(0, X.shape[1], chunk):
        g1 = min(g0 + chunk, X.shape[1])
        mu = s[:, None] * torch.exp(Dl @ coef[g0:g1].T)
        d = alpha[None, g0:g1] * mu + beta[None, g0:g1]
        U.append((Dl.T @ ((X[:, g0:g1].double() - mu) / d)).T)
        I.append((pairs.T @ (mu / d)).T)
    return torch.cat(U), torch.cat(I)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--nodes", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ps", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    import torch
    from prosstt_amd import fit, markers, regress
    N, G, R = args.cells, args.genes, args.nodes
    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    drift = np.cumsum(rng.normal(0.0, 0.05, size=(R, 1)) * rng.normal(0.0, 1.0, size=(1, G)), axis=0)
    logm = rng.normal(0.5, 1.0, size=(1, G)) + drift
    labels = rng.integers(0, R, size=N)
    sc = rng.lognormal(0.0, 0.4, size=N)
    alpha, beta = np.full(G, 0.2), np.full(G, 2.0)
    X = torch.empty((N, G), dtype=torch.int32, device="cuda")
    means = torch.as_tensor(np.exp(logm)).cuda()
    for lo in range(0, N, 5000):
        hi = min(lo + 5000, N)
        mu = torch.as_tensor(sc[lo:hi, None]).cuda() * means[torch.as_tensor(labels[lo:hi]).cuda()]
        shape = mu / (0.2 * mu + 1.0)                              # variance 0.2 mu^2 + 2 mu
        X[lo:hi] = torch.poisson(torch.distributions.Gamma(shape, shape / mu).sample()).to(torch.int32)
        del mu, shape
    print(json.dumps({"matrix": [N, G], "nodes": R, "device": torch.cuda.get_device_name(0)}), flush=True)

    one = fit._Pass(X, sc, labels.astype(np.int64), np.exp(logm), "regress_bench")
    ms, best = timed(torch, lambda: one(alpha, beta, out="torch"), args.reps)
    print(json.dumps({"what": "fit.loglik, one candidate", "ms": round(ms, 3), "best_ms": round(best, 3)}), flush=True)
    del one

    for p in args.ps:
        D = hats(R, p)
        coef = np.linalg.lstsq(D, logm, rcond=None)[0].T           # (G, p): near the fit
        run = regress._Pass(X, sc, labels.astype(np.int64), D, "regress_bench")
        for split in regress.SPLITS:
            for meat in (False, True):
                ms, best = timed(torch, lambda: run(coef, alpha, beta, meat, "torch", split), args.reps)
                print(json.dumps({"what": "regress.normal_equations", "p": p, "sums": p + p * (p + 1) // 2, "split": split,
                                  "meat": meat, "ms": round(ms, 3), "best_ms": round(best, 3)}), flush=True)
        if args.torch:
            dev = [torch.as_tensor(a).cuda() for a in (sc, labels, D, coef, alpha, beta)]
            ms, best = timed(torch, lambda: torch_sums(torch, X, *dev), max(args.reps // 2, 1))
            got = run(coef, alpha, beta, False, "torch", 0)
            U, _ = torch_sums(torch, X, *dev)
            err = float((U - got.score).abs().max() / got.score.abs().max())
            print(json.dumps({"what": "torch binary64, the same U and I", "p": p, "ms": round(ms, 3), "best_ms": round(best, 3),
                              "max |U - device| / max |U|": err}), flush=True)
            del dev, U, got
        del run
        torch.cuda.empty_cache()

    for p in args.ps[:2]:
        # regress.regression's own steps, timed apart: the setup (uploads, workspace, the count sums by markers.group_moments),
        # the passes with their copies back, and the rest of regression_with, which is the scoring on the host
        D = hats(R, p)
        passes = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run = regress._Pass(X, sc, labels.astype(np.int64), D, "regress_bench")
        totals = np.asarray(markers.group_moments(X, sc, np.zeros(N, dtype=np.int64)).count_sum).sum(axis=0)
        torch.cuda.synchronize()
        setup = time.perf_counter() - t0

        def evaluate(coef, meat):
            t = time.perf_counter()
            out = run(coef, alpha, beta, meat)
            passes.append(time.perf_counter() - t)
            return out

        t0 = time.perf_counter()
        r = regress.regression_with(evaluate, D, totals, float(sc.sum()))
        loop = time.perf_counter() - t0
        print(json.dumps({"what": "regress.regression, step by step", "p": p, "s": round(setup + loop, 3), "setup s": round(setup, 3),
                          "passes": len(passes), "in passes (device and copies) s": round(sum(passes), 3),
                          "scoring on the host s": round(loop - sum(passes), 3),
                          "scoring's share of the loop": round(1 - sum(passes) / loop, 3),
                          "rounds max": int(r.rounds.max()), "rounds mean": round(float(r.rounds.mean()), 2),
                          "converged": int(r.converged.sum()), "no_counts": int(r.no_counts.sum()),
                          "separated": int(r.separated.sum())}), flush=True)
        t0 = time.perf_counter()
        regress.regression(X, sc, labels, D, alpha=alpha, beta=beta)
        print(json.dumps({"what": "regress.regression", "p": p, "s": round(time.perf_counter() - t0, 3)}), flush=True)
        del run

    if args.numpy:
        import regress_model as M
        n, g, p = 5000, 2000, 8
        Xh = X[:n, :g].cpu().numpy()
        D = hats(R, p)
        coef = np.linalg.lstsq(D, logm[:, :g], rcond=None)[0].T
        for ordered in (True, False):
            t0 = time.perf_counter()
            M.normal_equations(Xh, sc[:n], labels[:n], D, coef, alpha[:g], beta[:g], ordered=ordered)
            print(json.dumps({"what": "numpy model, one pass", "matrix": [n, g], "p": p, "device order of the sums": ordered,
                              "s": round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == "__main__":
    main()
