"""Times prosstt_amd.factors on one device: one ``cell_equations`` pass per number of coefficients, per split and per
``genes_per_block``, each beside ``regress.normal_equations`` at the same p on the same matrix with one design row per cell (the
yardstick: the same arithmetic per entry in the other orientation) with the ratio of the two; the same on 2 000 selected genes
(a column view of the matrix); (``--torch``) the same sums by torch in binary64 on the same device; ``glmpca`` end to end with
its rounds, its passes and the host's share; and (``--numpy``) the numpy model of the pass at 5 000 x 2 000.  Medians of
``--reps`` calls by device events.  One JSON line per measurement.

    python tools/factors_bench.py [--cells 50000] [--genes 20000] [--reps 5] [--torch] [--numpy]

The matrix is synthetic: a rank-4 log-bilinear model, Poisson-gamma counts drawn by torch on the device (variance
0.2 mu^2 + 2 mu)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


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


def torch_sums(torch, X, s, L, C, alpha, beta, chunk=5000):
    """U (N, p) and I (N, P2) by torch in binary64, ``chunk`` cells at a time (two matrix products per chunk)."""
    p = L.shape[1]
    j, k = np.triu_indices(p)
    pairs = L[:, j] * L[:, k]                                      # (G, P2)
    U, I = [], []
    for lo in range(0, X.shape[0], chunk):
        hi = min(lo + chunk, X.shape[0])
        mu = s[lo:hi, None] * torch.exp(C[lo:hi] @ L.T)
        d = alpha[None, :] * mu + beta[None, :]
        U.append(((X[lo:hi].double() - mu) / d) @ L)
        I.append((mu / d) @ pairs)
    return torch.cat(U), torch.cat(I)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--selected", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ps", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()
    import torch
    from prosstt_amd import factors, regress
    N, G = args.cells, args.genes
    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    rank = 4
    scores, loads = rng.normal(0.0, 1.0, size=(N, rank)), rng.normal(0.0, 0.3, size=(G, rank))
    base = rng.normal(0.5, 1.0, size=G)
    sc = rng.lognormal(0.0, 0.4, size=N)
    alpha, beta = np.full(G, 0.2), np.full(G, 2.0)
    X = torch.empty((N, G), dtype=torch.int32, device="cuda")
    Ld, bd = torch.as_tensor(loads).cuda(), torch.as_tensor(base).cuda()
    for lo in range(0, N, 5000):
        hi = min(lo + 5000, N)
        mu = torch.as_tensor(sc[lo:hi, None]).cuda() * torch.exp(bd[None, :] + torch.as_tensor(scores[lo:hi]).cuda() @ Ld.T)
        shape = mu / (0.2 * mu + 1.0)                              # variance 0.2 mu^2 + 2 mu
        X[lo:hi] = torch.poisson(torch.distributions.Gamma(shape, shape / mu).sample()).to(torch.int32)
        del mu, shape
    print(json.dumps({"matrix": [N, G], "device": torch.cuda.get_device_name(0), "own genes_per_block": factors.gene_blocks(N, G)[0],
                      "regress row blocks": regress.row_blocks(N, G)[1]}), flush=True)

    def state(p, genes):
        """Loadings (genes, p) and coefficients (N, p) near the truth, padded with small columns beyond the rank."""
        L = np.concatenate([base[:genes, None], loads[:genes], 0.05 * rng.normal(size=(genes, max(p - 1 - rank, 0)))], axis=1)[:, :p]
        C = np.concatenate([np.ones((N, 1)), scores, 0.05 * rng.normal(size=(N, max(p - 1 - rank, 0)))], axis=1)[:, :p]
        return np.ascontiguousarray(L), np.ascontiguousarray(C)

    for genes, view in ((G, X), (min(args.selected, G), X[:, :min(args.selected, G)])):
        cells = factors._CellPass(view, sc, "factors_bench")
        for p in args.ps:
            L, C = state(p, genes)
            a, b = alpha[:genes], beta[:genes]
            own = {}
            for split in regress.SPLITS:
                ms, best = timed(torch, lambda: cells(L, C, a, b, None, "torch", split, 0), args.reps)
                own[split] = ms
                print(json.dumps({"what": "factors.cell_equations", "genes": genes, "p": p, "sums": p + p * (p + 1) // 2, "split": split,
                                  "genes_per_block": 0, "ms": round(ms, 3), "best_ms": round(best, 3)}), flush=True)
            chosen = 16 if p + p * (p + 1) // 2 <= 48 else 32
            for per in sorted({32 * 8, 32 * 32, -(-genes // 32) * 32}):
                ms, best = timed(torch, lambda: cells(L, C, a, b, None, "torch", 0, per), args.reps)
                print(json.dumps({"what": "factors.cell_equations", "genes": genes, "p": p, "split": 0, "genes_per_block": per,
                                  "gene blocks": factors.gene_blocks(N, genes, per)[1], "ms": round(ms, 3),
                                  "best_ms": round(best, 3)}), flush=True)
            # the yardstick: the gene half at the same p, the design one row per cell, the genes' coefficients
            run = regress._Pass(view, sc, np.arange(N), C, "factors_bench")
            ms, best = timed(torch, lambda: run(L, a, b, False, "torch", 0), args.reps)
            print(json.dumps({"what": "regress.normal_equations, one design row per cell", "genes": genes, "p": p, "ms": round(ms, 3),
                              "best_ms": round(best, 3), "cell_equations / normal_equations": round(own[chosen] / ms, 3)}), flush=True)
            del run
            if args.torch and genes == G:
                dev = [torch.as_tensor(v).cuda() for v in (sc, L, C, a, b)]
                ms, best = timed(torch, lambda: torch_sums(torch, view, *dev), max(args.reps // 2, 1))
                got = cells(L, C, a, b, None, "torch", 0, 0)
                U, _ = torch_sums(torch, view, *dev)
                err = float((U - got.score).abs().max() / got.score.abs().max())
                print(json.dumps({"what": "torch binary64, the same U and I", "p": p, "ms": round(ms, 3), "best_ms": round(best, 3),
                                  "max |U - device| / max |U|": err}), flush=True)
                del dev, U, got
            torch.cuda.empty_cache()
        del cells

    # glmpca end to end on the selected genes, its passes timed apart from the host's share (the solves, the copies' waits are
    # in the passes)
    genes = min(args.selected, G)
    view = X[:, :genes]
    passes = {"gene": [], "cell": []}
    real_pass, real_cells = regress._Pass.__call__, factors._CellPass.__call__

    def gene_call(self, *a, **k):
        t = time.perf_counter()
        out = real_pass(self, *a, **k)
        passes["gene"].append(time.perf_counter() - t)
        return out

    def cell_call(self, *a, **k):
        t = time.perf_counter()
        out = real_cells(self, *a, **k)
        passes["cell"].append(time.perf_counter() - t)
        return out

    regress._Pass.__call__, factors._CellPass.__call__ = gene_call, cell_call
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = factors.glmpca(view, sc, args.k, alpha=0.2, beta=2.0, max_rounds=args.rounds)
        total = time.perf_counter() - t0
    finally:
        regress._Pass.__call__, factors._CellPass.__call__ = real_pass, real_cells
    in_passes = sum(passes["gene"]) + sum(passes["cell"])
    print(json.dumps({"what": "factors.glmpca", "matrix": [N, genes], "k": args.k, "rounds": f.rounds, "s": round(total, 3),
                      "gene passes": len(passes["gene"]), "in them s": round(sum(passes["gene"]), 3),
                      "cell passes": len(passes["cell"]), "in them (device and copies) s": round(sum(passes["cell"]), 3),
                      "the host's share (start, solves, rotation)": round(1 - in_passes / total, 3),
                      "objective": [round(float(v), 1) for v in f.objective]}), flush=True)

    if args.numpy:
        import factors_model as M
        n, g, p = min(5000, N), min(2000, G), 8
        Xh = X[:n, :g].cpu().numpy()
        L, C = state(p, g)
        for ordered in (True, False):
            t0 = time.perf_counter()
            M.cell_equations(Xh, sc[:n], L, C[:n], alpha[:g], beta[:g], ordered=ordered)
            print(json.dumps({"what": "numpy model, one pass", "matrix": [n, g], "p": p, "device order of the sums": ordered,
                              "s": round(time.perf_counter() - t0, 3)}), flush=True)


if __name__ == "__main__":
    main()
