"""
Times of the layout step (prosstt_amd/layout.py, libprosstt_amd_layout.so) on the device, on the tests' noisy-Y cloud
(tests/graph_model.py: tree_points) at --cells x --dim with k = 14 neighbours from neighbors.knn:

  * the spectral start (S, the Lanczos run, the scaling on the host): wall time with a synchronise at the end, warm;
  * a whole run of --epochs epochs per lanes_per_row (4, 16, 64 and 0, the library's choice) as ONE bare C call from the
    spectral start: HIP events around it, the median of --reps, as microseconds per epoch, for every negative_sample_rate
    of --rates; beside it the same number of launches of the same kernel on a graph of three cells, which do no work: what
    of an epoch is launch cost;
  * the whole ``layout.umap`` call (graph checks, start, epochs, the copy to the host): wall time, the median of --reps;
  * with --score, the trustworthiness (k = 14) of the start and of the layout over 500 sampled cells;
  * with --numpy, the model of tests/layout_model.py at the same size: seconds per epoch over the first --numpy-epochs;
  * with --umap-learn, umap-learn's own optimiser on the copied graph, if that package imports.

    python tools/umap_bench.py [--cells 50000] [--dim 50] [--epochs 200] [--reps 5] [--rates 5,0] [--score] [--numpy] [--umap-learn]
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


def sampled_trustworthiness(X, Y, k, rows):
    """layout_model.trustworthiness restricted to the sampled ``rows`` (ranks among all cells)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    N = len(X)

    def order_of(Z):
        d = np.sum(Z * Z, axis=1)[None, :] - 2.0 * (Z[rows] @ Z.T)
        d[np.arange(len(rows)), rows] = -np.inf
        return np.argsort(d, axis=1, kind="stable")

    order_x = order_of(X)
    ranks_x = np.empty_like(order_x)
    np.put_along_axis(ranks_x, order_x, np.broadcast_to(np.arange(N), order_x.shape), axis=1)
    near = order_of(Y)[:, 1:k + 1]
    excess = np.maximum(np.take_along_axis(ranks_x, near, axis=1) - k, 0)
    return 1.0 - excess.sum() * 2.0 / (len(rows) * k * (2.0 * N - 3.0 * k - 1.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rates", default="5,0")
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--numpy-epochs", type=int, default=5)
    ap.add_argument("--umap-learn", action="store_true")
    args = ap.parse_args()

    import torch
    import graph_model
    import layout_model
    from prosstt_amd import _native, graph, layout, neighbors
    from prosstt_amd.device import _ptr
    L = _native.load("layout")
    N, d, E, k = args.cells, args.dim, args.epochs, 14
    print("device: %s; cloud: tree_points(%d, %d, seed %d), k = %d" % (torch.cuda.get_device_name(0), N, d, N, k))
    points = graph_model.tree_points(N, d, N)
    g = graph.connectivities(neighbors.knn(torch.from_numpy(points).cuda(), k, out="torch"), out="torch")
    nnz = g.indices.numel()
    p = g.data / g.data.max()
    sampled = int(torch.floor(E * p).sum())
    print("nnz %d (%.1f per row, longest row %d); %d edge samples in %d epochs (%.0f per epoch, x 6 pairs each)"
          % (nnz, nnz / N, int((g.indptr[1:] - g.indptr[:-1]).max()), sampled, E, sampled / E))

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

    ms, (_, vectors) = wall(lambda: layout.spectral_vectors(g, 2, out="torch"))
    start = torch.from_numpy(layout._scale_start(vectors.cpu().numpy(), 0)).cuda()
    print("spectral start     %9.3f ms" % ms)

    a, b = layout.find_ab_params(1.0, 0.5)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    tiny = graph.Connectivities(torch.tensor([0, 2, 4, 6]).cuda(), torch.tensor([1, 2, 0, 2, 0, 1], dtype=torch.int32).cuda(),
                                torch.zeros(6, dtype=torch.float64).cuda(), None, None)

    def run_ms(conn, weights, first, lanes, rate=5):
        """ms of the E epochs as one C call: the median of --reps, events around the call."""
        n = conn.indptr.numel() - 1
        y0, y1 = first.clone(), torch.empty_like(first)
        times = []
        for rep in range(args.reps + 1):
            y0.copy_(first)
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            _native.check(L.prosstt_amd_layout_epochs(stream, _ptr(conn.indptr), _ptr(conn.indices), _ptr(weights), n,
                                                      conn.indices.numel(), 2, _ptr(y0), _ptr(y1), 0, E, E, a, b, 1.0, 1.0,
                                                      rate, 0, lanes), "layout")
            end.record()
            end.synchronize()
            if rep:
                times.append(begin.elapsed_time(end))
        return float(np.median(times)), float(min(times)), float(max(times))

    empty = run_ms(tiny, tiny.data, start[:3].contiguous(), 16)
    print("%d launches that do no work (three cells): %.3f ms = %.2f us each (min %.2f, max %.2f)"
          % (E, empty[0], 1e3 * empty[0] / E, 1e3 * empty[1] / E, 1e3 * empty[2] / E))
    for rate in (int(v) for v in args.rates.split(",")):
        for lanes in (4, 16, 64, 0):
            med, lo, hi = run_ms(g, p, start, lanes, rate)
            print("epochs rate %2d lanes %2d    %9.3f ms for %d epochs = %7.2f us per epoch (min %.2f, max %.2f)"
                  % (rate, lanes, med, E, 1e3 * med / E, 1e3 * lo / E, 1e3 * hi / E))

    ms, lay = wall(lambda: layout.umap(g, n_epochs=E))
    print("umap(n_epochs=%d)  %9.3f ms   (the whole call, result on the host; finite: %s, largest |y| %.1f)"
          % (E, ms, bool(np.all(np.isfinite(lay.embedding))), float(np.abs(lay.embedding).max())))
    if args.score:
        rows = np.random.default_rng(0).choice(N, 500, replace=False)
        print("trustworthiness (k = %d, 500 sampled cells): start %.4f, layout %.4f"
              % (k, sampled_trustworthiness(points, lay.init, k, rows), sampled_trustworthiness(points, lay.embedding, k, rows)))
    if args.numpy:
        W = g.to_csr()
        Y = np.array(lay.init)
        t0 = time.perf_counter()
        for n in range(args.numpy_epochs):
            Y = layout_model.epoch(W, Y, n, E, a, b)[0].astype(np.float32)
        print("numpy model: %.3f s per epoch over the first %d" % ((time.perf_counter() - t0) / args.numpy_epochs, args.numpy_epochs))
    if args.umap_learn:
        try:
            from umap.umap_ import simplicial_set_embedding
        except ImportError:
            print("umap-learn does not import here: skipped")
        else:
            t0 = time.perf_counter()
            simplicial_set_embedding(points, g.to_csr(), 2, 1.0, a, b, 1.0, 5, E, "spectral", np.random.RandomState(0),
                                     "euclidean", {}, False, {}, False)
            print("umap-learn's simplicial_set_embedding: %.1f s" % (time.perf_counter() - t0))


if __name__ == "__main__":
    main()
