"""
Times of the count-model fit (prosstt_amd/fit.py, libprosstt_amd_fit.so) on the device, on the sampled workload C3
(50 000 cells x 20 000 genes) with the true means of its 8-branch tree as ``means``, warm:

  * one ``prosstt_amd_fit_loglik`` pass for C = 1, 3 and 10 candidates (HIP events, the median of --reps), and what that is
    per entry and candidate;
  * the same pass over matrices whose every entry is 0, 5 or 40: what each path of the term costs;
  * ``fit.count_model`` end to end with its rounds (wall time, once);
  * with --torch, the same sums for one candidate by torch's binary64 ``lgamma`` / ``log1p`` / ``log`` over chunks of genes
    on the same device, and how far the two are apart;
  * with --scipy, the numpy model (tests/fit_model.py) under ``scipy.optimize`` (L-BFGS-B per gene) at 2 000 x 200 on the
    host, beside ``fit.count_model`` on the same sub-matrix.

    python tools/fit_bench.py [--cells N] [--genes G] [--reps 3] [--torch] [--scipy]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--no-fit", action="store_true", help="skip the end-to-end count_model")
    args = ap.parse_args()

    import torch
    from prosstt_amd import fit, simulation as sim, workloads
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    rows, means = sim.cell_rows(work.tree, pt, br), fit.simulation_means(work.tree)
    run = fit._Pass(X, sc, fit._codes(rows, N), means, "fit_bench")
    N, G = run.m.N, run.m.G
    print("device: %s; C3: %d cells x %d genes, %d rows of means" % (torch.cuda.get_device_name(0), N, G, means.shape[0]))
    zeros = float((run.m.X == 0).sum().item()) / (float(N) * G)
    above = float((run.m.X > 12).sum().item()) / (float(N) * G)
    print("entries: %.1f %% zeros, %.2f %% above 12 (the Stirling form)" % (100 * zeros, 100 * above))
    alpha = np.clip(np.asarray(work.alpha, dtype=np.float64), 1e-5, None)
    beta = np.clip(np.asarray(work.beta, dtype=np.float64), 1.0 + 1e-5, None)

    def events(fn):
        times = []
        for rep in range(args.reps + 1):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            fn()
            end.record()
            end.synchronize()
            if rep:
                times.append(begin.elapsed_time(end))
        return float(np.median(times)), float(min(times)), float(max(times))

    rng = np.random.default_rng(3)
    for C in (1, 3, 10):
        a = alpha[None, :] * np.exp(rng.uniform(-0.5, 0.5, size=(C, G)))
        b = 1.0 + (beta[None, :] - 1.0) * np.exp(rng.uniform(-0.5, 0.5, size=(C, G)))
        a[0], b[0] = alpha, beta
        ms = events(lambda: run(a, b, out="torch"))
        print("loglik, C = %2d   %9.2f ms (min %.2f, max %.2f)   %.3f ns per entry and candidate"
              % (C, ms[0], ms[1], ms[2], ms[0] * 1e6 / (float(N) * G * C)))

    # what each path of the term costs: matrices of one value (10 000 cells of the same plan), four candidates
    n_part = min(10000, N)
    a4, b4 = np.tile(alpha, (4, 1)), np.tile(beta, (4, 1))
    for value in (0, 5, 40):
        part = fit._Pass(torch.full((n_part, G), value, dtype=torch.int32, device="cuda"), np.asarray(sc)[:n_part],
                         fit._codes(np.asarray(rows)[:n_part], n_part), means, "fit_bench")
        ms = events(lambda: part(a4, b4, out="torch"))
        print("every entry %2d, %d cells, C = 4   %9.2f ms   %.3f ns per entry and candidate"
              % (value, n_part, ms[0], ms[0] * 1e6 / (float(n_part) * G * 4)))

    if not args.no_fit:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = fit.count_model(X, sc, rows, means)
        s = time.perf_counter() - t0
        hp = fit.hyperparameters(f)
        print("count_model end to end   %8.2f s;  rounds: median %d, max %d;  %d of %d genes converged, %d on the box, %d without "
              "counts" % (s, int(np.median(f.rounds)), int(f.rounds.max()), int(f.converged.sum()), G, int(f.at_bound.sum()),
                          int(np.isnan(f.loglik).sum())))
        print("    log alpha: mean %.3f, std %.3f;  log(beta - 1): mean %.3f, std %.3f over %d genes"
              % (hp.log_alpha_mean, hp.log_alpha_std, hp.log_beta_minus_1_mean, hp.log_beta_minus_1_std, hp.n_genes))

    if args.torch:
        D, size, labels, M = run.m.X, run.size, run.labels.to(torch.int64), run.means
        a_d, bm1_d = torch.as_tensor(alpha).cuda(), torch.as_tensor(beta - 1.0).cuda()
        chunk = 512

        def by_torch():
            out = torch.empty(G, dtype=torch.float64, device="cuda")
            for lo in range(0, G, chunk):
                hi = min(G, lo + chunk)
                x = D[:, lo:hi].to(torch.float64)
                mu = size[:, None] * M[labels, lo:hi]
                theta = a_d[lo:hi] * mu + bm1_d[lo:hi]
                r = mu / theta
                l1 = torch.log1p(theta)
                t = torch.lgamma(r + x) - torch.lgamma(r) - r * l1 + x * (torch.log(theta) - l1)
                out[lo:hi] = torch.where(mu > 0, t, torch.zeros_like(t)).sum(dim=0)
            return out

        ms = events(by_torch)
        ours = run(alpha, beta, out="torch").values[0]
        theirs = by_torch()
        apart = float(((ours - theirs).abs() / ours.abs().clamp_min(1.0)).max().item())
        print("the same sums by torch (lgamma, log1p, log in binary64, %d genes at a time)   %9.2f ms (min %.2f, max %.2f); "
              "largest relative difference of a gene's sum %.2g" % (chunk, ms[0], ms[1], ms[2], apart))

    if args.scipy:
        import scipy.optimize
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import fit_model
        n, g = min(2000, N), min(200, G)
        sub = run.m.X[:n, :g].contiguous()
        cells = np.arange(n) if run.m.cell_of_row is None else run.m.cell_of_row[:n]
        sc_s, rows_s = np.asarray(sc, dtype=np.float64)[cells], np.asarray(rows)[cells]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fit.count_model(sub, sc_s, rows_s, means[:, :g])
        ours = time.perf_counter() - t0
        host = sub.cpu().numpy()
        t0 = time.perf_counter()
        best = np.full(g, np.nan)
        for j in range(g):
            if not host[:, j].any():
                continue
            res = scipy.optimize.minimize(
                lambda p: -fit_model.loglik(host[:, [j]], sc_s, rows_s, means[:, [j]], [np.exp(p[0])], [1.0 + np.exp(p[1])])[0][0, 0],
                [np.log(0.1), 0.0], method="L-BFGS-B", bounds=[(-12.0, 4.0)] * 2)
            best[j] = -res.fun
        theirs = time.perf_counter() - t0
        base = fit_model.loglik(host, sc_s, rows_s, means[:, :g], np.full(g, 0.1), np.full(g, 2.0))[1]
        keep = got.converged & np.isfinite(best)
        print("%d x %d: count_model %.2f s; scipy L-BFGS-B on the numpy model %.1f s (%d threads visible); count_model's "
              "likelihood minus scipy's over %d genes: least %.3g, largest %.3g"
              % (n, g, ours, theirs, os.cpu_count() or 1, int(keep.sum()), float((got.loglik - (best - base))[keep].min()),
                 float((got.loglik - (best - base))[keep].max())))


if __name__ == "__main__":
    main()
