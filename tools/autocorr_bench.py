"""
Times of the autocorrelation step (prosstt_amd/autocorr.py, libprosstt_amd_autocorr.so) on the device, on the sampled workload
C3 (50 000 cells x 20 000 genes; the graph: connectivities of the 14 nearest neighbours in the PCA scores), warm, with HIP
events, the median of --reps:

  * ``prosstt_amd_autocorr_gene_sums`` as a bare C call: both gene tiles, three values of rows_per_block, the matrix in the
    PRESENTED row order (cells of a branch together: a block's neighbours lie in nearby rows) beside the same matrix with
    its rows in PLAN order (neighbours anywhere), and on --select chosen genes; nnz G 4 bytes over the time is the gather
    rate;
  * ``prosstt_amd_autocorr_smooth`` alone (the same gather, less arithmetic, one store per entry);
  * the kernels on their own from a ``rocprofv3 --kernel-trace --stats`` run of --one-call in a child process;
  * the same sums by the torch route on the same device: float32 A formed per chunk of --chunk genes, ``torch.sparse.mm`` with
    the graph as a float32 CSR tensor, elementwise products and column sums (float32 throughout, where the library's sums
    are binary64);
  * ``autocorr.autocorrelation`` end to end (the statistics on the host out; wall time);
  * with --scipy, the host route at 5 000 x 2 000: the copy of the matrix, ``log1p(X / s)``, scipy CSR @ dense and the sums.

    python tools/autocorr_bench.py [--cells N] [--genes G] [--select 2000] [--chunk 2000] [--reps 3] [--no-kernels] [--scipy]
"""
import argparse
import csv
import ctypes
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("autocorr_sums_kernel", "autocorr_finish_kernel", "autocorr_smooth_kernel")


def kernel_times(args):
    """{kernel: (launches, average ns)} of --one-call under rocprofv3, in a child process of its own."""
    out = tempfile.mkdtemp(prefix="autocorr_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--one-call", "--reps", str(args.reps)]
        for name in ("cells", "genes"):
            if getattr(args, name):
                cmd += ["--" + name, str(getattr(args, name))]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        found = {}
        for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for kernel in KERNELS:
                    if kernel in row["Name"]:
                        calls, total = found.get(kernel, (0, 0.0))
                        found[kernel] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]))
        return {k: (c, t / c) for k, (c, t) in found.items()}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--select", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="skip the rocprofv3 child run")
    ap.add_argument("--one-call", action="store_true", help="the two bare calls alone, warm + --reps times (what the child runs)")
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, autocorr, device, embed, graph, hvg, neighbors, simulation as sim, workloads
    from prosstt_amd.device import _ptr
    L = _native.load("autocorr")
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    assert isinstance(X, device.PresentedCounts)
    op = embed.LogNormalized(X, sc)
    N, G = op.shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    t0 = time.perf_counter()
    nb = neighbors.knn(embed.pca(X, sc).scores, 14, out="torch")
    g = graph.connectivities(nb, out="torch")
    torch.cuda.synchronize()
    graph_ms = (time.perf_counter() - t0) * 1e3
    nnz = g.indices.numel()
    mean = op.gene_moments()[0] / N
    mu = torch.as_tensor(mean).cuda()
    # (the columns relabelled to matrix rows, cell_of_row): what autocorr.graph_sums passes for a presented matrix
    perms = (torch.as_tensor(X.row_of_cell.astype(np.int32)).cuda()[g.indices.to(torch.int64)],
             torch.as_tensor(X.cell_of_row.astype(np.int32)).cuda())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def workspace(n, genes, rpb):
        need = ctypes.c_uint64(0)
        _native.check(L.prosstt_amd_autocorr_workspace_bytes(n, genes, rpb, ctypes.byref(need)), "autocorr")
        return torch.empty(int(need.value), dtype=torch.uint8, device="cuda")

    def sums_call(D, ld, inv, perm, genes, mean_t, rpb, tile, out):
        ws = workspace(N, genes, rpb)
        return lambda: _native.check(L.prosstt_amd_autocorr_gene_sums(
            stream, _ptr(D), N, genes, ld, _ptr(inv), _ptr(perm[1]), _ptr(g.indptr), _ptr(perm[0]), _ptr(g.data),
            nnz, _ptr(mean_t), rpb, tile, _ptr(ws), ws.numel(), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3]),
            _ptr(status)), "autocorr")

    def smooth_call(D, ld, inv, perm, genes, tile, panel):
        return lambda: _native.check(L.prosstt_amd_autocorr_smooth(
            stream, _ptr(D), N, genes, ld, _ptr(inv), _ptr(perm[1]), _ptr(g.indptr), _ptr(perm[0]), _ptr(g.data),
            nnz, 1, tile, _ptr(panel), genes, _ptr(status)), "autocorr")

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

    def report(name, t, genes):
        print("%-58s %9.2f ms (min %.2f, max %.2f): %.2f TB/s gathered" % (name, t[0], t[1], t[2], 4e-9 * nnz * genes / t[0]))

    sums = torch.empty((4, G), dtype=torch.float64, device="cuda")
    panel = torch.empty((N, G), dtype=torch.float32, device="cuda")
    if args.one_call:
        events(sums_call(op.counts, op.ld, op.inv_size, perms, G, mu, 0, 0, sums))
        events(smooth_call(op.counts, op.ld, op.inv_size, perms, G, 0, panel))
        assert int(status.item()) == 0
        return

    print("device: %s; C3: %d cells x %d genes, row stride %d; graph: %d entries (%.1f per cell), pca + knn + connectivities %.0f ms"
          % (torch.cuda.get_device_name(0), N, G, op.ld, nnz, nnz / N, graph_ms))
    rows = X.row_of_cell[g.indices.cpu().numpy().astype(np.int64)]
    own = np.repeat(X.row_of_cell, np.diff(g.indptr.cpu().numpy()))
    print("median |row of a neighbour - row of its cell|: presented order %d, plan order %d"
          % (np.median(np.abs(rows - own)), np.median(np.abs(g.indices.cpu().numpy() - np.repeat(np.arange(N), np.diff(g.indptr.cpu().numpy()))))))

    for tile in (256, 64):
        report("gene_sums, presented rows, gene_tile %d" % tile,
               events(sums_call(op.counts, op.ld, op.inv_size, perms, G, mu, 0, tile, sums)), G)
    keep = sums.clone()
    for rpb in (64, 196, 512):
        report("gene_sums, presented rows, gene_tile 256, rows_per_block %d" % rpb,
               events(sums_call(op.counts, op.ld, op.inv_size, perms, G, mu, rpb, 256, sums)), G)
    plan = X.in_plan_order()
    inv_plan = torch.as_tensor(embed._inverse_sizes(sc, N)).cuda()
    for tile in (256, 64):
        report("gene_sums, rows in plan order, gene_tile %d" % tile,
               events(sums_call(plan, G, inv_plan, (g.indices, None), G, mu, 0, tile, sums)), G)
    apart = float(((sums - keep).abs() / keep[2].abs().clamp_min(1e-300)).max())
    print("    largest difference of a sum between the two row orders, relative to the gene's m2: %.3g" % apart)
    for tile in (256, 64):
        report("smooth, presented rows, gene_tile %d" % tile, events(smooth_call(op.counts, op.ld, op.inv_size, perms, G, tile, panel)), G)
    report("smooth, rows in plan order, gene_tile 256", events(smooth_call(plan, G, inv_plan, (g.indices, None), G, 256, panel)), G)
    assert int(status.item()) == 0

    n_sel = min(args.select, G)
    idx = np.sort(np.random.default_rng(7).choice(G, size=n_sel, replace=False))
    Xs = hvg.select_genes(X, idx)
    mu_s = torch.as_tensor(mean[idx]).cuda()
    sums_s = torch.empty((4, n_sel), dtype=torch.float64, device="cuda")
    for tile in (64, 256):
        report("gene_sums on %d selected genes, gene_tile %d" % (n_sel, tile),
               events(sums_call(Xs.counts, n_sel, op.inv_size, perms, n_sel, mu_s, 0, tile, sums_s)), n_sel)
    print("    the same bits as those genes of the full call: %s" % bool(torch.equal(sums_s.view(torch.int64), keep[:, torch.as_tensor(idx).cuda()].view(torch.int64))))

    if not args.no_kernels:
        try:
            times = kernel_times(args)
        except (OSError, subprocess.SubprocessError) as e:
            print("the rocprofv3 run failed: %s" % e)
            times = {}
        for kernel in KERNELS:
            if kernel not in times:
                print("%-28s not found in the trace" % kernel)
                continue
            calls, ns = times[kernel]
            rate = "" if "finish" in kernel else ": %.2f TB/s gathered" % (4.0 * nnz * G / ns / 1e3)
            print("%-28s %10.3f ms per launch, %d launches under rocprofv3%s" % (kernel, ns / 1e6, calls, rate))

    # the torch route: float32 A per chunk of genes, torch.sparse.mm, elementwise sums
    try:
        Wt = torch.sparse_csr_tensor(g.indptr, g.indices.to(torch.int64), g.data.to(torch.float32), size=(N, N))
        r = torch.zeros(N, dtype=torch.float32, device="cuda").index_add_(
            0, torch.repeat_interleave(torch.arange(N, device="cuda"), g.indptr[1:] - g.indptr[:-1]), g.data.to(torch.float32))
        c = torch.zeros(N, dtype=torch.float32, device="cuda").index_add_(0, g.indices.to(torch.int64), g.data.to(torch.float32))
        rc = (r + c)[:, None]
        mu32 = mu.to(torch.float32)
        got = torch.empty((4, G), dtype=torch.float32, device="cuda")

        def torch_route():
            for c0 in range(0, G, args.chunk):
                c1 = min(G, c0 + args.chunk)
                A = torch.log1p(plan[:, c0:c1].to(torch.float32) * inv_plan[:, None])
                Z = A - mu32[None, c0:c1]
                M = torch.sparse.mm(Wt, Z)
                cross = (Z * M).sum(0)
                zz = Z * Z
                got[0, c0:c1] = cross
                got[1, c0:c1] = (rc * zz).sum(0) - 2.0 * cross
                got[2, c0:c1] = zz.sum(0)
                got[3, c0:c1] = (zz * zz).sum(0)

        t = events(torch_route)
        sums_call(plan, G, inv_plan, (g.indices, None), G, mu, 0, 0, sums)()
        live = sums[2] > 0
        moran = lambda s: (s[0] / s[2])[live]                        # noqa: E731
        print("%-58s %9.2f ms (min %.2f, max %.2f); largest difference of cross / m2 from the library's: %.3g"
              % ("the torch route (float32, chunks of %d genes, sparse.mm)" % args.chunk, t[0], t[1], t[2],
                 float((moran(got.to(torch.float64)) - moran(sums)).abs().max())))
        del Wt, got
    except (RuntimeError, NotImplementedError) as e:
        print("the torch route failed: %s" % (str(e).splitlines()[0],))
    del plan, panel

    ms, res = wall(lambda: autocorr.autocorrelation(X, sc, g))
    print("autocorrelation end to end %9.1f ms (graph on the device in, statistics on the host out); %d genes with adjusted p < 0.01; "
          "I of the first ten in order: %s" % (ms, int(np.sum(res.pvals_adj < 0.01)), np.round(res.morans_i[res.order[:10]], 3)))

    if args.scipy:
        import scipy.sparse as sparse
        n, k = min(5000, N), min(2000, G)
        cells = np.sort(X.cell_of_row[:n])
        sub = op.counts[torch.as_tensor(X.row_of_cell[cells]).cuda()][:, :k].contiguous()      # n cells in plan order
        s = np.asarray(sc, dtype=np.float64)[cells]
        small = graph.connectivities(neighbors.knn(embed.pca(sub, s).scores, 14))
        ms, got = wall(lambda: autocorr.graph_sums(sub, s, small))
        W = sparse.csr_matrix((small.data, small.indices, small.indptr), shape=(n, n))
        t0 = time.perf_counter()
        host = sub.cpu().numpy()
        t1 = time.perf_counter()
        A = np.log1p(host / s[:, None])
        t2 = time.perf_counter()
        Z = A - A.mean(0)
        M = W @ Z
        cross, m2 = (Z * M).sum(0), (Z * Z).sum(0)
        margins = np.asarray(W.sum(1)).ravel() + np.asarray(W.sum(0)).ravel()
        sq = (margins[:, None] * Z * Z).sum(0) - 2 * cross
        t3 = time.perf_counter()
        live = got.m2 > 0
        print("%d x %d, %d entries: graph_sums %.2f ms; the host route: copy %.1f ms, log1p %.1f ms, scipy CSR @ dense and the sums "
              "%.1f ms (%d threads visible); largest differences of cross / m2 and sqdiff / m2: %.2g, %.2g"
              % (n, k, W.nnz, ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, os.cpu_count() or 1,
                 np.abs(cross / m2 - got.cross / got.m2)[live].max(), np.abs(sq / m2 - got.sqdiff / got.m2)[live].max()))


if __name__ == "__main__":
    main()
