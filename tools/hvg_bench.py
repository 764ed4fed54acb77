"""
Times of the highly-variable-gene step (prosstt_amd/hvg.py, libprosstt_amd_hvg.so) on the device, on the sampled workload C3
(50 000 cells x 20 000 genes), warm, with HIP events, the median of --reps, each new pass beside its yardstick in the same
process:

  * ``prosstt_amd_hvg_clipped_sums`` (thresholds of the matrix's own seurat_v3 fit) beside
    ``prosstt_amd_stats_count_summary`` on the same matrix: the same bytes read;
  * ``prosstt_amd_hvg_normalized_moments`` beside ``prosstt_amd_embed_gene_moments``;
  * ``prosstt_amd_hvg_gather_columns`` of --select sorted columns beside ``torch.index_select(X, 1, idx)``;
  * ``hvg.highly_variable_genes`` of both flavours end to end (the mask on the host out; wall time), and the share of the
    seurat_v3 call that is the local regression;
  * ``embed.pca`` on the selected genes beside all of them (wall time);
  * with --numpy, the host route of seurat_v3 at 5 000 x 2 000: the copy of the matrix, mean and variance, the same
    regression, ``np.minimum(X, clip)`` and its two sums.

    python tools/hvg_bench.py [--cells N] [--genes G] [--select 2000] [--reps 5] [--numpy]
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
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--select", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, embed, hvg, summary, simulation as sim, workloads
    from prosstt_amd.device import _ptr
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    op = embed.LogNormalized(X, sc)
    N, G = op.shape
    n_sel = min(args.select, G)
    D, ld = op.counts, op.ld
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lh, Ls, Le = _native.load("hvg"), _native.load("stats"), _native.load("embed")

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

    def beside(name, new, yard_name, yard, nbytes):
        a, b = events(new), events(yard)
        a2, b2 = events(new), events(yard)                      # interleaved: both twice, the better median of each
        a, b = min(a, a2), min(b, b2)
        print("%-34s %8.3f ms (min %.3f, max %.3f) = %.2f TB/s;  %-28s %8.3f ms (min %.3f, max %.3f);  ratio %.2f"
              % (name, a[0], a[1], a[2], nbytes / (a[0] * 1e-3) / 1e12, yard_name, b[0], b[1], b[2], a[0] / b[0]))

    def workspace(lib, symbol, *sizes):
        need = ctypes.c_uint64(0)
        _native.check(getattr(_native.load(lib), symbol)(*sizes, ctypes.byref(need)), lib)
        return torch.empty(int(need.value), dtype=torch.uint8, device="cuda")

    print("device: %s; C3: %d cells x %d genes, row stride %d" % (torch.cuda.get_device_name(0), N, G, ld))
    matrix_bytes = 4.0 * N * G
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    i64 = dict(dtype=torch.int64, device="cuda")

    # the clipped pass beside count_summary
    cs = summary.count_summary(X)
    fit = hvg.seurat_v3_fit(cs, device=D.device)
    thr = torch.as_tensor(fit.thresholds.astype(np.int32)).cuda()
    ws_h = workspace("hvg", "prosstt_amd_hvg_workspace_bytes", N, G)
    ws_s = workspace("stats", "prosstt_amd_stats_workspace_bytes", N, G)
    n_over, sum_le, sumsq_le = torch.empty(G, **i64), torch.empty(G, **i64), torch.empty(2 * G, **i64)
    gs, gq, gz, ct, cz = (torch.empty(G, **i64), torch.empty(2 * G, **i64), torch.empty(G, **i64), torch.empty(N, **i64),
                          torch.empty(N, **i64))
    beside("clipped_sums",
           lambda: _native.check(Lh.prosstt_amd_hvg_clipped_sums(stream, _ptr(D), N, G, ld, _ptr(thr), _ptr(ws_h), ws_h.numel(),
                                                                 _ptr(n_over), _ptr(sum_le), _ptr(sumsq_le), _ptr(status)), "hvg"),
           "count_summary",
           lambda: _native.check(Ls.prosstt_amd_stats_count_summary(stream, _ptr(D), N, G, ld, _ptr(ws_s), ws_s.numel(), _ptr(gs),
                                                                    _ptr(gq), _ptr(gz), _ptr(ct), _ptr(cz), _ptr(status), 0), "stats"),
           matrix_bytes)
    print("    entries over their gene's threshold: %d of %.3g" % (int(n_over.sum().item()), float(N) * G))

    # normalized_moments beside embed's gene_moments
    ws_e = workspace("embed", "prosstt_amd_embed_workspace_bytes", N, G, 1)
    S = torch.empty(2, G, dtype=torch.float64, device="cuda")
    beside("normalized_moments",
           lambda: _native.check(Lh.prosstt_amd_hvg_normalized_moments(stream, _ptr(D), N, G, ld, _ptr(op.inv_size), _ptr(ws_h),
                                                                       ws_h.numel(), _ptr(S[0]), _ptr(S[1]), _ptr(status)), "hvg"),
           "embed gene_moments",
           lambda: _native.check(Le.prosstt_amd_embed_gene_moments(stream, _ptr(D), N, G, ld, _ptr(op.inv_size), _ptr(ws_e),
                                                                   ws_e.numel(), _ptr(S[0]), _ptr(S[1]), _ptr(status)), "embed"),
           matrix_bytes)

    # the gather beside torch.index_select
    rng = np.random.default_rng(7)
    idx = np.sort(rng.choice(G, size=n_sel, replace=False))
    cols32, cols64 = torch.as_tensor(idx.astype(np.int32)).cuda(), torch.as_tensor(idx).cuda()
    Y = torch.empty((N, n_sel), dtype=torch.int32, device="cuda")
    Y2 = torch.empty((N, n_sel), dtype=torch.int32, device="cuda")
    beside("gather_columns, %d sorted" % n_sel,
           lambda: _native.check(Lh.prosstt_amd_hvg_gather_columns(stream, _ptr(D), N, G, ld, _ptr(cols32), n_sel, _ptr(Y), n_sel,
                                                                   _ptr(status)), "hvg"),
           "torch.index_select(X, 1, idx)", lambda: torch.index_select(D, 1, cols64, out=Y2), 4.0 * N * n_sel)
    assert torch.equal(Y, Y2) and int(status.item()) == 0

    # both flavours end to end
    ms3, hv3 = wall(lambda: hvg.highly_variable_genes(X, n_top_genes=n_sel))
    t0 = time.perf_counter()
    hvg.seurat_v3_fit(cs, device=D.device)
    fit_ms = (time.perf_counter() - t0) * 1e3
    print("highly_variable_genes, seurat_v3   %8.1f ms end to end (of it the fit with its regression over %d genes: %.1f ms)"
          % (ms3, int((hv3.variances > 0).sum()), fit_ms))
    ms, hvs = wall(lambda: hvg.highly_variable_genes(X, sc, n_sel, "seurat"))
    print("highly_variable_genes, seurat      %8.1f ms end to end; %d genes in both selections" %
          (ms, int((hv3.highly_variable & hvs.highly_variable).sum())))

    # the PCA on the selected genes beside all of them
    Xs = hvg.select_genes(X, hv3.genes)
    ms_sel, _ = wall(lambda: embed.pca(Xs, sc))
    ms_all, _ = wall(lambda: embed.pca(X, sc))
    print("embed.pca on %d selected genes     %8.1f ms;  on all %d genes %8.1f ms" % (n_sel, ms_sel, G, ms_all))

    if args.numpy:
        n_small, g_small = min(5000, N), min(2000, G)
        sub = D[:n_small, :g_small].contiguous()
        ms, got = wall(lambda: hvg.highly_variable_genes(sub, n_top_genes=max(1, g_small // 10)))
        t0 = time.perf_counter()
        host = sub.cpu().numpy().astype(np.float64)
        t1 = time.perf_counter()
        mean, var = host.mean(axis=0), host.var(axis=0, ddof=1)
        t2 = time.perf_counter()
        v = var > 0
        reg_std = np.ones(g_small)
        reg_std[v] = np.sqrt(10.0 ** hvg.loess_fit(np.log10(mean[v]), np.log10(var[v])))
        clip = reg_std * np.sqrt(n_small) + mean
        t3 = time.perf_counter()
        C = np.minimum(host, clip[None, :])
        sum_c, sq_c = C.sum(axis=0), (C * C).sum(axis=0)
        vn = (n_small * mean ** 2 + sq_c - 2.0 * sum_c * mean) / ((n_small - 1) * reg_std ** 2)
        t4 = time.perf_counter()
        vn[~v] = 0.0
        apart = float(np.abs(vn - got.variances_norm).max())
        print("%d x %d: highly_variable_genes %.1f ms; the host route: copy %.1f ms, mean and variance %.1f ms, the regression "
              "%.1f ms, np.minimum and its sums %.1f ms (%d threads visible); largest difference of a score %.2g"
              % (n_small, g_small, ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t4 - t3) * 1e3, os.cpu_count() or 1,
                 apart))


if __name__ == "__main__":
    main()
