"""
Times of the count-matrix summary (prosstt_amd/summary.py, libprosstt_amd_stats.so) on the device:

  * count_summary's kernels alone at C3 and T32 (HIP events around the enqueue, warm, mean of --reps), with the rate at
    which they read the 4-byte counts;
  * sample_density_summary end to end (wall clock to the host result) at C3 and, in chunks, at C5 on one GPU;
  * once, for contrast, sample_density(out="numpy") followed by the reference notebooks' five numpy lines at C3.

    python tools/summary_bench.py [--configs C3,T32] [--c5] [--numpy] [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_time(X, reps):
    import torch
    from prosstt_amd import _native, device
    L = _native.load("stats")
    p = device._ptr
    m = device.CountMatrix(X, "summary_bench").on_device()
    genes = torch.zeros(4, m.G, dtype=torch.int64, device=m.device)          # sum, sumsq (low, high), zeros
    cells = torch.empty(2, m.N, dtype=torch.int64, device=m.device)
    status = torch.zeros(1, dtype=torch.int32, device=m.device)

    def enqueue():                                       # what summary.count_summary enqueues, workspace included
        ws = m.workspace("stats", "prosstt_amd_stats_workspace_bytes")
        _native.check(L.prosstt_amd_stats_count_summary(
            m.stream(), p(m.X), m.N, m.G, m.ld, p(ws), ws.numel(), p(genes[0]), p(genes[1:3]), p(genes[3]), p(cells[0]),
            p(cells[1]), p(status), 0), "stats")

    for _ in range(3):
        enqueue()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        enqueue()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,T32")
    ap.add_argument("--c5", action="store_true", help="sample_density_summary at C5 (1 000 000 x 30 000) in chunks")
    ap.add_argument("--numpy", action="store_true", help="sample_density(out='numpy') + numpy's five lines at C3, once")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from prosstt_amd import simulation as sim, workloads, summary
    torch.cuda.set_device(0)
    for name in [c for c in args.configs.split(",") if c]:
        work = workloads.build(name)
        pt, br, sc, _ = work.plan()
        presented = sim.draw_counts(work.tree, pt, br, sc, work.alpha, work.beta, seed=1, out="torch")
        N, G = presented.shape
        ms = kernel_time(presented.counts, args.reps)
        print("%s count_summary kernels: %d x %d, %.3f ms, %.0f GB/s of counts read (mean of %d, warm)"
              % (name, N, G, ms, N * G * 4 / ms / 1e6, args.reps), flush=True)
        del presented
        torch.cuda.empty_cache()
        if name == "C3":
            for chunk in (None, 10000):
                np.random.seed(work.cfg["seed"] + 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = summary.sample_density_summary(work.tree, N, alpha=work.alpha, beta=work.beta, chunk_cells=chunk)[0]
                t1 = time.perf_counter()
                print("C3 sample_density_summary (chunk_cells=%s): %.1f ms wall, %d counts summed"
                      % (chunk, (t1 - t0) * 1e3, int(s.gene_sum.sum())), flush=True)
            if args.numpy:
                np.random.seed(work.cfg["seed"] + 1)
                t0 = time.perf_counter()
                X = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, out="numpy")[0]
                t1 = time.perf_counter()
                stats = (np.mean(X, axis=0), np.var(X, axis=0), np.sum(X == 0, axis=0), np.sum(X == 0, axis=1),
                         np.sum(X, axis=1))
                t2 = time.perf_counter()
                assert int(stats[4].sum()) == int(s.gene_sum.sum())
                print("C3 sample_density(out='numpy') + numpy's five lines: %.1f ms + %.1f ms wall"
                      % ((t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
                del X, stats
        del work
        torch.cuda.empty_cache()
    if args.c5:
        work = workloads.build("C5")
        N = work.cfg["N"]
        np.random.seed(work.cfg["seed"] + 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = summary.sample_density_summary(work.tree, N, alpha=work.alpha, beta=work.beta)[0]
        t1 = time.perf_counter()
        print("C5 sample_density_summary: %d x %d in chunks of %d cells, %.1f ms wall, peak device memory %.1f GB, "
              "%d counts summed, mean library size %.1f"
              % (s.n_cells, s.n_genes, summary.default_chunk_cells(N, work.tree.G), (t1 - t0) * 1e3,
                 torch.cuda.max_memory_allocated() / 1e9, int(s.gene_sum.sum()), s.cell_total.mean()), flush=True)


if __name__ == "__main__":
    main()
