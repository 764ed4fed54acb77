"""
Times of the clustering step (prosstt_amd/cluster.py, libprosstt_amd_cluster.so) on the device, on the tests' noisy-Y cloud
(tests/graph_model.py: tree_points) at --cells x --dim with k = 14 neighbours from neighbors.knn:

  * the quantisation (one bare C call): HIP events around it, the median of --reps;
  * one sweep per path that holds the level-0 graph, and path 0, from c_i = i and from the communities of the first level
    (few communities, many lanes sharing one), beside the same launch on a graph of three nodes, which does no work: what of
    a sweep is launch cost;
  * the totals for both community arrays;
  * the aggregation of level 0 (emit, torch's sort and prefix sum, fold, the bins of the next level): wall time;
  * ``cluster.louvain`` end to end (graph checks, every level, the labels on the host): wall time, its levels and rounds,
    and what a round costs on average (two sweeps, two totals, one copy of the two int64 arrays and the decision on the
    host);
  * with --networkx, ``networkx.community.louvain_communities`` (seed 0) on the copied graph of --networkx-cells cells, its
    seconds and both Q values at that size.

    python tools/cluster_bench.py [--cells 50000] [--dim 50] [--reps 5] [--networkx] [--networkx-cells 20000]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--networkx", action="store_true")
    ap.add_argument("--networkx-cells", type=int, default=20000)
    args = ap.parse_args()

    import torch
    import graph_model
    from prosstt_amd import _native, cluster, graph, neighbors
    from prosstt_amd.device import _ptr
    L = _native.load("cluster")
    N, d, k = args.cells, args.dim, 14
    print("device: %s; cloud: tree_points(%d, %d, seed %d), k = %d" % (torch.cuda.get_device_name(0), N, d, N, k))

    def connectivities(n):
        points = graph_model.tree_points(n, d, n)
        return graph.connectivities(neighbors.knn(torch.from_numpy(points).cuda(), k, out="torch"), out="torch")

    g = connectivities(N)
    nnz = g.indices.numel()
    lengths = (g.indptr[1:] - g.indptr[:-1])
    print("nnz %d (%.1f per row, longest row %d)" % (nnz, nnz / N, int(lengths.max())))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def events(fn):
        """ms of what ``fn`` enqueues: the median, min and max of --reps, events around it, after one warm call."""
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

    flags = torch.zeros(2, dtype=torch.int32, device="cuda")
    u = torch.empty(nnz, dtype=torch.int64, device="cuda")
    kk = torch.empty(N, dtype=torch.int64, device="cuda")
    ms = events(lambda: _native.check(L.prosstt_amd_cluster_quantize(stream, _ptr(g.indptr), _ptr(g.indices), _ptr(g.data), N, nnz,
                                                                    _ptr(u), _ptr(kk), _ptr(flags)), "cluster"))
    print("quantize           %9.3f ms (min %.3f, max %.3f)" % ms)
    level = cluster.quantize(g)
    print("rows of at most 16 / 64 / 512 entries: %d / %d / %d of %d" % (level.bins + (N,)))

    tiny = cluster.LevelGraph.from_csr(np.array([0, 2, 4, 6]), np.array([1, 2, 0, 2, 0, 1], dtype=np.int32),
                                       np.full(6, 1 << 32, dtype=np.int64))

    def sweep_call(lv, c, tot, path):
        c_new = torch.empty_like(c)
        return lambda: _native.check(L.prosstt_amd_cluster_sweep(stream, _ptr(lv.indptr), _ptr(lv.indices), _ptr(lv.u), _ptr(lv.k),
                                                                 lv.n, lv.indices.numel(), _ptr(lv.rows), *lv.bins, _ptr(c),
                                                                 _ptr(tot), lv.M2, 1.0, 0, path, _ptr(c_new), _ptr(flags[1:]),
                                                                 _ptr(flags)), "cluster")

    c3 = torch.arange(3, dtype=torch.int32, device="cuda")
    for path in cluster.PATHS:
        ms = events(sweep_call(tiny, c3, tiny.k, path))
        print("a sweep that does no work (three nodes), path %d: %7.2f us (min %.2f, max %.2f)" % ((path,) + tuple(1e3 * v for v in ms)))

    longest = int(lengths.max())
    own = torch.arange(N, dtype=torch.int32, device="cuda")
    first_level, _, _ = cluster._run_level(L, level, 1.0, 1e-7, 1000, 0)
    for name, c in (("c_i = i", own), ("the first level's communities (%d)" % int(torch.unique(first_level).numel()), first_level)):
        tot, inn = cluster.totals(level, c)
        for path in cluster.PATHS:
            if path in (1, 2, 3) and longest > cluster.PATH_ROWS[path - 1]:
                print("sweep path %d from %s: refused, the longest row has %d entries" % (path, name, longest))
                continue
            ms = events(sweep_call(level, c, tot, path))
            print("sweep path %d from %-40s %9.3f ms (min %.3f, max %.3f)" % ((path, name) + ms))
        both = torch.empty((2, N), dtype=torch.int64, device="cuda")
        ms = events(lambda: _native.check(L.prosstt_amd_cluster_totals(stream, _ptr(level.indptr), _ptr(level.indices), _ptr(level.u),
                                                                      _ptr(level.k), N, nnz, _ptr(c), _ptr(both[0]), _ptr(both[1]),
                                                                      _ptr(flags)), "cluster"))
        print("totals from %-47s %9.3f ms (min %.3f, max %.3f)" % ((name,) + ms))
    torch.cuda.synchronize()
    assert int(flags[0].item()) == 0

    ms, (nxt, _) = wall(lambda: cluster.aggregate(level, first_level))
    print("aggregate level 0  %9.3f ms wall (%d -> %d nodes, %d -> %d entries, longest row %d)"
          % (ms, N, nxt.n, nnz, nxt.indices.numel(), int((nxt.indptr[1:] - nxt.indptr[:-1]).max())))

    ms, res = wall(lambda: cluster.louvain(g))
    rounds = sum(r for _, _, r, _ in res.levels)
    print("louvain()          %9.3f ms wall, Q = %.4f, %d clusters (largest %d, smallest %d)"
          % (ms, res.modularity, len(res.sizes), int(res.sizes[0]), int(res.sizes[-1])))
    print("  levels (nodes -> communities, accepted rounds): %s" % ", ".join("%d -> %d (%d)" % lv[:3] for lv in res.levels))
    print("  %d accepted rounds and %d refused ones: %.3f ms per round run, everything else included"
          % (rounds, len(res.levels), ms / (rounds + len(res.levels))))
    ms0, _ = wall(lambda: cluster._run_level(L, level, 1.0, 1e-7, 1000, 0))
    r0 = res.levels[0][2]
    print("  level 0 alone     %9.3f ms wall for %d + 1 rounds = %.3f ms per round (two sweeps, two totals, one copy of 2 x %d "
          "int64 and the host's fsum)" % (ms0, r0, ms0 / (r0 + 1), N))

    if args.networkx:
        import networkx as nx
        n = min(args.networkx_cells, N)
        gs = g if n == N else connectivities(n)
        W = gs.to_csr()
        t0 = time.perf_counter()
        ours = cluster.louvain(gs)
        t_ours = time.perf_counter() - t0
        G = nx.from_scipy_sparse_array(W)
        t0 = time.perf_counter()
        parts = nx.community.louvain_communities(G, seed=0)
        t_nx = time.perf_counter() - t0
        print("at %d cells: louvain() %.3f s, Q = %.4f, %d clusters; networkx louvain_communities(seed=0) %.1f s, Q = %.4f, %d clusters"
              % (n, t_ours, ours.modularity, len(ours.sizes), t_nx, nx.community.modularity(G, parts), len(parts)))


if __name__ == "__main__":
    main()
