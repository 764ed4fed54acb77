"""
Times of binomial thinning (prosstt_amd/thin.py, libprosstt_amd_thin.so) on the device, on the sampled workload C3 (50 000 cells x
20 000 genes), warm, with HIP events, the median of --reps, every pass into outputs allocated once:

  * the part [0, k) at 1/2 (one plane), 1/4 (two), 3/16 (four) and 40 000 / 65 536 (ten) and [1, 65 536) (sixteen planes), each
    without and with the complement (the three-matrix case: 4 GB read, 8 GB written);
  * ``downsample``'s pass with per-cell fractions (the totals' median as the target depth);
  * beside them ``X.clone()`` (the floor of a pass that reads and writes the matrix once), ``hvg.select_genes`` of all columns,
    and ``torch.distributions.Binomial(X, p).sample()`` in chunks of rows on the same device;
  * the share of the entries that are not 0, and of those that take more than one step of 64 trials;
  * with --rank-curve, ``thin.rank_curve`` end to end on --select highly variable genes (wall time);
  * with --numpy, the host route at 5 000 x 2 000: the copy of the matrix and ``numpy.random.Generator.binomial``.

    python tools/thin_bench.py [--cells N] [--genes G] [--reps 5] [--numpy] [--rank-curve] [--select 2000] [--ks 2 5 10]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--rank-curve", action="store_true")
    ap.add_argument("--select", type=int, default=2000)
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 5, 10])
    ap.add_argument("--max-rounds", type=int, default=None)
    args = ap.parse_args()

    import torch
    from prosstt_amd import hvg, summary, thin, simulation as sim, workloads
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    presented = X                                  # cells grouped by their row of the mean tensor: a device.PresentedCounts
    X = X.counts if hasattr(X, "counts") else X    # the passes are timed on the matrix as it lies
    N, G = X.shape
    m = thin._matrix(X, "thin_bench").on_device()

    def events(fn):
        """ms of what ``fn`` enqueues: the median, least and largest of --reps after one warm call."""
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

    print("device: %s; C3: %d cells x %d genes, row stride %d" % (torch.cuda.get_device_name(0), N, G, m.ld))
    nonzero = int(torch.count_nonzero(X).item())
    long = int((X > 64).sum().item())
    print("entries: %.4g, not 0: %.2f %%, more than one step of 64 trials: %d (%.4f %% of all, %.4f %% of those not 0), largest %d"
          % (float(N) * G, 100.0 * nonzero / (float(N) * G), long, 100.0 * long / (float(N) * G), 100.0 * long / max(nonzero, 1),
             int(X.max().item())))
    matrix_bytes = 4.0 * N * G
    Y, R = torch.empty_like(X), torch.empty_like(X)
    vec = thin.plan(N, G, X.data_ptr(), m.ld, Y.data_ptr(), G, R.data_ptr(), G)[0]
    print("instantiation: %s" % ("aligned (16-byte loads and stores)" if vec else "plain"))

    clone = events(lambda: Y.copy_(X))
    print("%-44s %8.3f ms (min %.3f, max %.3f) = %.2f TB/s moved" % ("X.clone() into place (the floor)", *clone,
                                                                    2 * matrix_bytes / (clone[0] * 1e-3) / 1e12))
    everything = np.arange(G)
    gather = events(lambda: hvg.select_genes(X, everything))
    print("%-44s %8.3f ms (min %.3f, max %.3f);  ratio to the clone %.2f" % ("hvg.select_genes of all columns", *gather,
                                                                          gather[0] / clone[0]))

    def run(lo1, lo_n, hi1, hi_n, complement):
        out = thin._enqueue(m, lo1, lo_n, hi1, hi_n, 5, complement, 0, 0, out=(Y, R if complement else None))
        return out[2]

    for name, lo, hi in (("1/2: [0, 32768), 1 plane", 0, 32768), ("1/4: [0, 16384), 2 planes", 0, 16384),
                         ("3/16: [0, 12288), 4 planes", 0, 12288), ("[0, 40000), 10 planes", 0, 40000),
                         ("[1, 65536), 16 planes", 1, 65536)):
        for complement in (False, True):
            t = events(lambda: run(lo, None, hi, None, complement))
            moved = (3 if complement else 2) * matrix_bytes
            print("%-44s %8.3f ms (min %.3f, max %.3f) = %.2f TB/s moved;  ratio to the clone %.2f"
                  % (name + (", with the complement" if complement else ""), *t, moved / (t[0] * 1e-3) / 1e12, t[0] / clone[0]))
    assert int(run(0, None, 32768, None, True).item()) == 0 and bool((Y + R == X).all())

    totals = summary.count_summary(X).cell_total
    target = int(np.median(totals))
    grid = thin.downsample_grid(totals, target)
    t = events(lambda: run(0, None, None, grid, False))
    planes = np.array([16 - ((int(k) & -int(k)).bit_length() - 1) if 0 < k < 65536 else 0 for k in grid])
    print("%-44s %8.3f ms (min %.3f, max %.3f);  ratio to the clone %.2f  (target depth %d; %d of %d cells thinned, %.1f planes "
          "on average over those)" % ("downsample's pass, per-cell fractions", *t, t[0] / clone[0], target, int((grid < 65536).sum()),
                                      N, float(planes[grid < 65536].mean()) if (grid < 65536).any() else 0.0))

    rows = 5000

    def by_torch():
        for at in range(0, N, rows):
            Y[at:at + rows] = torch.distributions.Binomial(X[at:at + rows].to(torch.float32), probs=0.5).sample().to(torch.int32)

    t = events(by_torch)
    print("%-44s %8.3f ms (min %.3f, max %.3f);  ratio to the clone %.2f" % ("torch.distributions.Binomial in chunks of %d" % rows,
                                                                          *t, t[0] / clone[0]))
    del Y, R

    if args.rank_curve:
        hv = hvg.highly_variable_genes(presented, n_top_genes=min(args.select, G))
        Xs = hvg.select_genes(presented, hv.genes)
        alpha, beta = (np.broadcast_to(np.asarray(v, dtype=np.float64), (G,))[hv.genes] for v in (work.alpha, work.beta))
        kwargs = {} if args.max_rounds is None else {"max_rounds": args.max_rounds}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        curve = thin.rank_curve(Xs, sc, args.ks, alpha=alpha, beta=beta, seed=5, **kwargs)
        torch.cuda.synchronize()
        print("rank_curve on %d selected genes, ks = %s%s: %.1f s end to end; held-out Q minus its largest %s, best k = %d"
              % (len(hv.genes), list(curve.ks), "" if args.max_rounds is None else ", at most %d rounds" % args.max_rounds,
                 time.perf_counter() - t0, np.round(curve.heldout - curve.heldout.max(), 1).tolist(), curve.best))

    if args.numpy:
        n_small, g_small = min(5000, N), min(2000, G)
        sub = X[:n_small, :g_small].contiguous()
        small = events(lambda: thin.interval(sub, 0, 32768, seed=5))
        t0 = time.perf_counter()
        host = sub.cpu().numpy()
        t1 = time.perf_counter()
        np.random.default_rng(5).binomial(host, 0.5)
        t2 = time.perf_counter()
        print("%d x %d: thin.interval %.3f ms with its status word; the host route: copy %.1f ms, numpy's binomial %.1f ms"
              % (n_small, g_small, small[0], (t1 - t0) * 1e3, (t2 - t1) * 1e3))


if __name__ == "__main__":
    main()
