"""
Times of the PCA passes (prosstt_amd/embed.py, libprosstt_amd_embed.so) on the device:

  * gene_moments, matmul and rmatmul alone at C3 and T32 with l = 64 (HIP events around the bare C calls, warm, mean of
    --reps), with the rate at which they read the 4-byte counts;
  * embed.pca(k=50, n_iter=7) end to end (wall clock to the host result) at C3, from the sampler's PresentedCounts;
  * for contrast, the copy of the same matrix to the host (to_host("numpy32"));
  * with --sklearn, scikit-learn's randomized PCA of log1p(X / s) on that host copy, if scikit-learn is importable.

    python tools/embed_bench.py [--configs C3,T32] [--reps 20] [--l 64] [--sklearn]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_times(op, l, reps):
    """ms per call of each entry point, enqueued back to back without the wrapper's status check."""
    import torch
    from prosstt_amd import _native, device
    L = _native.load("embed")
    p = device._ptr
    N, G = op.shape
    ws = op.matrix.workspace("embed", "prosstt_amd_embed_workspace_bytes", l)
    W = torch.randn(G, l, device=op.device)
    Q = torch.randn(N, l, device=op.device)
    Y = torch.empty(N, l, device=op.device)
    Z = torch.empty(G, l, device=op.device)
    S = torch.empty(2, G, dtype=torch.float64, device=op.device)
    st = op.matrix.stream()
    X, ld, inv, status = p(op.counts), op.ld, p(op.inv_size), p(op.status)
    calls = {
        "gene_moments": lambda: L.prosstt_amd_embed_gene_moments(st, X, N, G, ld, inv, p(ws), ws.numel(), p(S[0]), p(S[1]),
                                                                  status),
        "matmul": lambda: L.prosstt_amd_embed_matmul(st, X, N, G, ld, inv, p(W), l, p(Y), p(ws), ws.numel(), status),
        "rmatmul": lambda: L.prosstt_amd_embed_rmatmul(st, X, N, G, ld, inv, p(Q), l, p(Z), p(ws), ws.numel(), status),
    }
    out = {}
    for name, call in calls.items():
        for _ in range(3):
            _native.check(call(), "embed")
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            _native.check(call(), "embed")
        stop.record()
        stop.synchronize()
        out[name] = start.elapsed_time(stop) / reps
    assert int(op.status.item()) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,T32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--l", type=int, default=64)
    ap.add_argument("--sklearn", action="store_true", help="scikit-learn's randomized PCA on the host copy at C3, once")
    args = ap.parse_args()
    import torch
    from prosstt_amd import simulation as sim, workloads, embed
    torch.cuda.set_device(0)
    for name in [c for c in args.configs.split(",") if c]:
        work = workloads.build(name)
        pt, br, sc, _ = work.plan()
        presented = sim.draw_counts(work.tree, pt, br, sc, work.alpha, work.beta, seed=1, out="torch")
        N, G = presented.shape
        op = embed.LogNormalized(presented, sc)
        for k, ms in kernel_times(op, args.l, args.reps).items():
            print("%s %-12s %d x %d, l = %d: %.3f ms, %.0f GB/s of counts read (mean of %d, warm)"
                  % (name, k, N, G, args.l, ms, N * G * 4 / ms / 1e6, args.reps), flush=True)
        if name == "C3":
            walls = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p = embed.pca(presented, sc, 50)
                walls.append((time.perf_counter() - t0) * 1e3)
            print("C3 pca(k=50, n_iter=7): %s ms wall to the host result (first call, then warm); top sigma %.4g, "
                  "explained variance ratio of 50 components %.4f"
                  % (", ".join("%.1f" % w for w in walls), p.singular_values[0], p.explained_variance_ratio.sum()),
                  flush=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = presented.to_host("numpy32")
            t1 = time.perf_counter()
            print("C3 to_host('numpy32') of the same matrix: %.1f ms wall" % ((t1 - t0) * 1e3), flush=True)
            if args.sklearn:
                try:
                    from sklearn.decomposition import PCA as SkPCA
                except ImportError:
                    print("C3 scikit-learn: not importable, skipped", flush=True)
                else:
                    t0 = time.perf_counter()
                    A = np.log1p(host / sc[:, None].astype(np.float32))
                    t1 = time.perf_counter()
                    SkPCA(50, svd_solver="randomized", random_state=0).fit_transform(A)
                    t2 = time.perf_counter()
                    print("C3 scikit-learn: log1p(X / s) %.0f ms + randomized PCA(50) %.0f ms wall"
                          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
                    del A
            del host
        del presented, op, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
