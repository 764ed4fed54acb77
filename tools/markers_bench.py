"""
Times of the marker-gene step (prosstt_amd/markers.py, libprosstt_amd_markers.so) on the device, on a sampled workload
(--workload: C3 is 50 000 cells x 20 000 genes with K = 8, 32 and 256 random balanced labels; T32 is the same size on a tree of
32 branches, grouped by its branches):

  * the grouped pass as a bare C call beside ``prosstt_amd_embed_gene_moments`` on the same matrix in the same process: HIP
    events around each, warm, the median of --reps.  The moments kernel is the yardstick: it reads the same bytes with the same
    layout and forms the same entries;
  * ``rank_genes_groups`` end to end (labels on the host in, the ranking on the host out): wall time, the median of --reps;
  * with --scipy, the host route at 5 000 x 2 000: the copy of the matrix, ``log1p(X / s)`` and ``scipy.stats.ttest_ind`` per
    group against the rest.

    python tools/markers_bench.py [--workload C3] [--cells N] [--genes G] [--groups 8,32,256] [--reps 5] [--scipy]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="C3", choices=["C3", "T32"])
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--groups", default="8,32,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, embed, markers, simulation as sim, workloads
    from prosstt_amd.device import _ptr
    L, E = _native.load("markers"), _native.load("embed")
    work = workloads.build(args.workload, G=args.genes)
    N = args.cells or workloads.CONFIGS[args.workload]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    op = embed.LogNormalized(X, sc)
    N, G = op.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("device: %s; workload %s: %d cells x %d genes, %d branches, row stride %d"
          % (torch.cuda.get_device_name(0), args.workload, N, G, len(np.unique(br)), op.ld))

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

    ws = op._workspace(1)
    S = torch.empty(2, G, dtype=torch.float64, device="cuda")
    yard = events(lambda: _native.check(E.prosstt_amd_embed_gene_moments(
        stream, _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(ws), ws.numel(), _ptr(S[0]), _ptr(S[1]), _ptr(op.status)),
        "embed"))
    print("embed gene_moments           %8.4f ms (min %.4f, max %.4f): %.2f TB/s of counts" % (yard + (4e-9 * N * G / yard[0],)))

    rng = np.random.default_rng(7)
    cases = [("%d branches" % len(np.unique(br)), np.unique(br, return_inverse=True)[1])] if args.workload == "T32" else []
    cases += [("K = %d random" % k, rng.permutation(np.arange(N) % k)) for k in (int(v) for v in args.groups.split(","))]
    for name, labels in cases:
        groups, codes = markers.encode_labels(labels, N)
        K = len(groups)
        key = torch.as_tensor(markers.codes_in_row_order(codes, op.matrix.cell_of_row)).cuda()
        rows = torch.sort(key, stable=True).indices.to(torch.int32)
        start = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
        start[1:] = torch.cumsum(torch.bincount(key, minlength=K), 0)
        need = ctypes.c_uint64(0)
        _native.check(L.prosstt_amd_markers_workspace_bytes(N, G, K, 0, ctypes.byref(need)), "markers")
        mws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        ints = torch.empty((2, K, G), dtype=torch.int64, device="cuda")
        sums = torch.empty((2, K, G), dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        med, lo, hi = events(lambda: _native.check(L.prosstt_amd_markers_group_moments(
            stream, _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(rows), N, _ptr(start), K, 0, _ptr(mws), mws.numel(),
            _ptr(ints[0]), _ptr(ints[1]), _ptr(sums[0]), _ptr(sums[1]), _ptr(status)), "markers"))
        assert int(status.item()) == 0
        apart = [float(((sums[i].sum(0) - S[i]).abs() / S[i].clamp_min(1e-300)).max()) for i in (0, 1)]
        print("grouped pass, %-16s %8.4f ms (min %.4f, max %.4f) = %.2f x gene_moments; workspace %.0f MB; sum_k S1, S2 against "
              "embed's, relative: %.3g, %.3g" % (name, med, lo, hi, med / yard[0], need.value / 1e6, apart[0], apart[1]))
        ms, res = wall(lambda: markers.rank_genes_groups(X, sc, labels))
        print("rank_genes_groups, %-12s %7.2f ms end to end (labels on the host in, %d x %d ranking on the host out)"
              % (name, ms, K, G))
    del mws, ints, sums

    if args.scipy:
        import scipy.stats
        n, g, k = 5000, 2000, 8
        sub = op.counts[:n, :g].contiguous()
        s = np.asarray(sc, dtype=np.float64)[op.matrix.cell_of_row[:n] if op.matrix.cell_of_row is not None else slice(0, n)]
        labels = rng.permutation(np.arange(n) % k)
        ms, _ = wall(lambda: markers.rank_genes_groups(sub, s, labels))
        t0 = time.perf_counter()
        host = sub.cpu().numpy()
        t1 = time.perf_counter()
        A = np.log1p(host / s[:, None])
        t2 = time.perf_counter()
        for group in range(k):
            scipy.stats.ttest_ind(A[labels == group], A[labels != group], equal_var=False, axis=0)
        t3 = time.perf_counter()
        print("%d x %d, K = %d: rank_genes_groups %.2f ms; the host route: copy %.1f ms, log1p %.1f ms, ttest_ind per group %.1f "
              "ms (%d threads visible)" % (n, g, k, ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, os.cpu_count() or 1))


if __name__ == "__main__":
    main()
