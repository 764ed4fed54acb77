"""
Times of the t-SNE step (prosstt_amd/tsne.py, libprosstt_amd_tsne.so) on the device, on the tests' noisy-Y cloud
(tests/graph_model.py: tree_points) at --cells x --dim:

  * the affinities of --cells x --neighbours neighbours from neighbors.knn at --perplexity (the bisection kernel alone as a
    bare C call, HIP events around it; and the whole ``tsne.affinities`` call with its sort, wall time with a synchronise):
    the median of --reps;
  * the gradient at the positions after --warm iterations, per ``slabs`` value of --slabs (0: the library's choice), as ONE
    bare C call of --batch iterations: HIP events around it, the median of --reps, as microseconds per iteration, and the
    pair terms per second that makes; beside it the same launches on three cells, which do no work: what of an iteration
    is launch cost;
  * the whole ``tsne.tsne`` call on the panel (kNN, affinities, --iterations iterations, objective, copy to the host): wall
    time, the median of --reps; with --score, the trustworthiness (k = 15) of the result over 500 sampled cells;
  * with --sklearn, scikit-learn's Barnes-Hut TSNE on the same panel on the host, if that package imports.

    python tools/tsne_bench.py [--cells 50000] [--dim 50] [--neighbours 90] [--perplexity 30] [--iterations 1000] [--reps 5]
                               [--slabs 0,1,4,11,32] [--score] [--sklearn]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--neighbours", type=int, default=90)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iterations", type=int, default=1000)
    ap.add_argument("--warm", type=int, default=50)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slabs", default="0,1,4,11,32")
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()

    import torch
    import graph_model
    from prosstt_amd import _native, neighbors, tsne
    from prosstt_amd.device import _ptr
    from umap_bench import sampled_trustworthiness
    L = _native.load("tsne")
    N, d, k = args.cells, args.dim, args.neighbours
    print("device: %s; cloud: tree_points(%d, %d, seed %d), k = %d, perplexity %g"
          % (torch.cuda.get_device_name(0), N, d, N, k, args.perplexity))
    points = graph_model.tree_points(N, d, N)
    panel = torch.from_numpy(points).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def wall(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times)), out

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

    ms, nb = wall(lambda: neighbors.knn(panel, k, out="torch"))
    print("knn(k = %d)           %9.3f ms" % (k, ms))
    cond = torch.empty((N, k), dtype=torch.float64, device="cuda")
    beta = torch.empty(N, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    med, lo, hi = events(lambda: _native.check(L.prosstt_amd_tsne_affinities(
        stream, _ptr(nb.indices), _ptr(nb.sq_distances), N, k, args.perplexity, _ptr(cond), _ptr(beta), _ptr(status)), "tsne"))
    print("conditional affinities %8.3f ms (min %.3f, max %.3f): %d x %d, 65 evaluations of H each" % (med, lo, hi, N, k))
    ms, aff = wall(lambda: tsne.affinities(nb, args.perplexity, out="torch"))
    nnz = aff.indices.numel()
    print("affinities()          %9.3f ms   (the bisection, the emit, torch's sort and prefix sum, the fold); nnz %d (%.1f per row)"
          % (ms, nnz, nnz / N))

    eta = max(N / 12.0 / 4.0, 50.0)
    start = torch.from_numpy(points[:, :2] / points[:, 0].std() * 1e-4).float().cuda()
    Y, update, gains = tsne.optimize(aff, start, 0, args.warm, learning_rate=eta)
    tiny = tsne.Affinities(torch.tensor([0, 2, 4, 6]).cuda(), torch.tensor([1, 2, 0, 2, 0, 1], dtype=torch.int32).cuda(),
                           torch.full((6,), 1.0 / 6, dtype=torch.float64).cuda(), None)

    def iterations_ms(a, first, slabs):
        n = a.indptr.numel() - 1
        need = ctypes.c_uint64(0)
        _native.check(L.prosstt_amd_tsne_workspace_bytes(n, 2, slabs, ctypes.byref(need)), "tsne")
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        y0, y1 = first.clone(), torch.empty_like(first)
        u, g = torch.zeros_like(first), torch.ones_like(first)
        return events(lambda: _native.check(L.prosstt_amd_tsne_iterations(
            stream, _ptr(a.indptr), _ptr(a.indices), _ptr(a.data), n, a.indices.numel(), 2, _ptr(y0), _ptr(y1), _ptr(u), _ptr(g),
            args.warm, args.warm + args.batch, 0, 12.0, 1e-6, slabs, _ptr(ws), ws.numel()), "tsne"))

    B = args.batch
    empty = iterations_ms(tiny, start[:3].contiguous(), 1)
    print("%d iterations that do no work (three cells, three launches each): %.3f ms = %.2f us each (min %.2f, max %.2f)"
          % (B, empty[0], 1e3 * empty[0] / B, 1e3 * empty[1] / B, 1e3 * empty[2] / B))
    for slabs in (int(v) for v in args.slabs.split(",")):
        med, lo, hi = iterations_ms(aff, Y, slabs)
        print("iterations slabs %4d  %9.3f ms for %d = %8.2f us per iteration (min %.2f, max %.2f): %.3g pair terms per second"
              % (slabs, med, B, 1e3 * med / B, 1e3 * lo / B, 1e3 * hi / B, float(N) * N / (1e-3 * med / B)))

    ms, res = wall(lambda: tsne.tsne(panel, perplexity=args.perplexity, n_iter=args.iterations))
    print("tsne(n_iter=%d)     %9.3f ms   (the whole call from the panel, result on the host; KL %.4f, finite: %s, largest |y| %.1f)"
          % (args.iterations, ms, res.kl_divergence, bool(np.all(np.isfinite(res.embedding))), float(np.abs(res.embedding).max())))
    rows = np.random.default_rng(0).choice(N, min(N, 500), replace=False)
    if args.score:
        print("trustworthiness (k = 15, %d sampled cells): start %.4f, layout %.4f"
              % (len(rows), sampled_trustworthiness(points, res.init, 15, rows), sampled_trustworthiness(points, res.embedding, 15, rows)))
    if args.sklearn:
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            print("scikit-learn does not import here: skipped")
        else:
            t0 = time.perf_counter()
            model = TSNE(2, perplexity=args.perplexity, init="pca", method="barnes_hut", random_state=0)
            emb = model.fit_transform(points)
            print("scikit-learn's Barnes-Hut TSNE on the host (%d threads visible): %.1f s; KL %.4f; trustworthiness %.4f"
                  % (os.cpu_count() or 1, time.perf_counter() - t0, model.kl_divergence_, sampled_trustworthiness(points, emb, 15, rows)))


if __name__ == "__main__":
    main()
