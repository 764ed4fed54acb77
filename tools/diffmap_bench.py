"""
Times of the graph step (prosstt_amd/graph.py, libprosstt_amd_graph.so) on the device, on the tests' noisy-Y cloud
(tests/graph_model.py: tree_points) at --cells x --dim with k = 14, 100 and 700 neighbours from neighbors.knn:

  * connectivities (memberships, the keyed entries, torch's sort and prefix sum, the fold) and the normalisation into T:
    HIP events around the calls, warm, mean of --reps;
  * one product y = T x per lanes_per_row (4, 16, 64 and 0, the library's choice): events around --spmv-reps bare C calls,
    beside the bytes a product must move (12 per stored entry, 8 per gathered x, 8 per row of y and of indptr) at 8 TB/s;
  * diffmap(n_comps=15) on the finished connectivities, warm: wall time with a synchronise at the end (it includes the
    host's eigh of the tridiagonal matrix every 16 steps), and the Lanczos steps taken;
  * with --scipy, the host route on the copied graph: the normalisation in scipy CSR arithmetic and
    scipy.sparse.linalg.eigsh(T, k=15, which="LM"), and the largest difference between the two sets of eigenvalues.

    python tools/diffmap_bench.py [--cells 50000] [--dim 50] [--ks 14,100,700] [--reps 5] [--spmv-reps 200] [--scipy]
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


def event_ms(fn, reps):
    """ms per call of fn, warm: HIP events around ``reps`` calls."""
    import torch
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def wall_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--dim", type=int, default=50)
    ap.add_argument("--ks", default="14,100,700")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spmv-reps", type=int, default=200)
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()

    import torch
    import graph_model
    from prosstt_amd import _native, graph, neighbors
    from prosstt_amd.device import _ptr
    L = _native.load("graph")
    N, d = args.cells, args.dim
    print("device: %s; cloud: tree_points(%d, %d, seed %d)" % (torch.cuda.get_device_name(0), N, d, N))
    P = torch.from_numpy(graph_model.tree_points(N, d, N)).cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in (int(v) for v in args.ks.split(",")):
        nb = neighbors.knn(P, k, out="torch")
        g = graph.connectivities(nb, out="torch")
        t = graph.transitions(g)
        nnz = g.indices.numel()
        longest = int((g.indptr[1:] - g.indptr[:-1]).max())
        print("k = %d: nnz %d (%.1f per row, longest row %d)" % (k, nnz, nnz / N, longest))
        print("  connectivities   %9.3f ms" % event_ms(lambda: graph.connectivities(nb, out="torch"), args.reps))
        print("  normalisation    %9.3f ms" % event_ms(lambda: graph.transitions(g), args.reps))
        x = torch.from_numpy(np.random.default_rng(k).standard_normal(N)).cuda()
        y = torch.empty_like(x)
        floor_us = (12.0 * nnz + 8.0 * nnz + 16.0 * N) / 8e12 * 1e6
        for lanes in (4, 16, 64, 0):
            def product():
                _native.check(L.prosstt_amd_graph_spmv(stream, _ptr(t.indptr), _ptr(t.indices), _ptr(t.data), N, nnz,
                                                       _ptr(x), _ptr(y), lanes), "graph")
            us = 1e3 * event_ms(product, args.spmv_reps)
            print("  spmv lanes %2d    %9.2f us   (%.1f GB/s of entries; the bytes at 8 TB/s: %.2f us)"
                  % (lanes, us, 12.0 * nnz / us / 1e3, floor_us))
        ms, dm = wall_ms(lambda: graph.diffmap(g, 15, out="torch"), max(1, args.reps // 2))
        print("  diffmap(15)      %9.3f ms   (%d Lanczos steps, largest residual estimate %.2g)"
              % (ms, dm.steps, dm.residuals.max()))
        if args.scipy:
            import scipy.sparse.linalg as sla
            W = g.to_csr()
            t0 = time.perf_counter()
            T, _, _ = graph_model.transitions(W)
            t1 = time.perf_counter()
            values = sla.eigsh(T, k=15, which="LM", return_eigenvectors=True)[0]
            t2 = time.perf_counter()
            order = np.argsort(-values)
            print("  host: scipy normalisation %.1f ms, eigsh(k=15, LM) %.1f ms; eigenvalues differ by at most %.2g"
                  % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, np.abs(values[order] - dm.eigenvalues.cpu().numpy()).max()))
        del nb, g, t, dm
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
