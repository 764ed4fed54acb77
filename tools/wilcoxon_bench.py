"""
Times of the Wilcoxon marker-gene step (prosstt_amd/ranks.py, libprosstt_amd_ranks.so) on the device, on the sampled workload
C3 (50 000 cells x 20 000 genes) with K = 8 random balanced labels:

  * ``prosstt_amd_ranks_rank_sums`` as a bare C call: HIP events around it, warm, the median of --reps;
  * its kernels each on their own -- the emit, one sort pass, the fold -- from a ``rocprofv3 --kernel-trace --stats`` run of
    this file as a child process (--one-call: the same call and nothing else), averaged per launch and added up per call,
    with the bytes each moves per entry (emit 4 in + 6 out, a sort pass 4 + 6 in and 6 out, the fold 2 x 6 in);
  * ``torch.sort(dim=1, stable=True)`` of one chunk of keys of the same shape (genes_per_pass x cells int32, the bit patterns
    of torch's own log1p(x / s): the same distribution, not the same bits), beside the four sort passes of that chunk: the
    yardstick for the hand-written passes;
  * ``ranks.rank_sums`` and ``markers.rank_genes_groups(method="wilcoxon")`` end to end (labels on the host in, the integers or
    the ranking on the host out): wall time, the median of --reps;
  * with --scipy, the host route at 5 000 x 2 000: the copy of the matrix, ``log1p(X / s)``, ``scipy.stats.rankdata`` per gene
    and the rank sums per group.

    python tools/wilcoxon_bench.py [--cells N] [--genes G] [--groups 8] [--reps 3] [--no-kernels] [--scipy]
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

KERNELS = ("ranks_emit_kernel", "ranks_sort_kernel", "ranks_fold_kernel")
BYTES_PER_ENTRY = {"ranks_emit_kernel": 4 + 6, "ranks_sort_kernel": 4 + 6 + 6, "ranks_fold_kernel": 12}


def kernel_times(args):
    """{kernel: (launches, average ns)} of --one-call under rocprofv3, in a child process of its own."""
    out = tempfile.mkdtemp(prefix="wilcoxon_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
               os.path.abspath(__file__), "--one-call", "--groups", str(args.groups), "--reps", str(args.reps)]
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
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-kernels", action="store_true", help="skip the rocprofv3 child run")
    ap.add_argument("--one-call", action="store_true", help="the bare call alone, warm + --reps times (what the child runs)")
    ap.add_argument("--scipy", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, embed, markers, ranks, simulation as sim, workloads
    from prosstt_amd.device import _ptr
    L = _native.load("ranks")
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch")
    op = embed.LogNormalized(X, sc)
    N, G = op.shape
    K = args.groups
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    labels = rng.permutation(np.arange(N) % K)
    groups, codes = markers.encode_labels(labels, N)
    n, rows, start = markers._row_list(codes, K, op.matrix.cell_of_row, op.device)
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_ranks_workspace_bytes(N, G, 0, ctypes.byref(need)), "ranks")
    gpp = min(G, ((1 << 30) - 1024) // (12 * N))                 # the header's rule for genes_per_pass = 0
    chunks = -(-G // gpp)
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    Q = torch.empty((K, G), dtype=torch.int64, device="cuda")
    T = torch.empty(G, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def bare():
        _native.check(L.prosstt_amd_ranks_rank_sums(stream, _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(rows), N, _ptr(start),
                                                    K, -1, 0, _ptr(ws), ws.numel(), _ptr(Q), _ptr(T), _ptr(status)), "ranks")

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

    if args.one_call:
        events(bare)
        assert int(status.item()) == 0
        return

    print("device: %s; C3: %d cells x %d genes, K = %d, row stride %d; workspace %.0f MB for %d genes per pass (%d chunks)"
          % (torch.cuda.get_device_name(0), N, G, K, op.ld, need.value / 1e6, gpp, chunks))
    med, lo, hi = events(bare)
    assert int(status.item()) == 0
    entries = float(N) * G
    print("rank_sums, bare call         %9.2f ms (min %.2f, max %.2f): %.2f ns per gene, %.3g entries/s"
          % (med, lo, hi, med * 1e6 / G, entries / (med * 1e-3)))
    total_q = int(Q.sum().item())
    assert total_q == G * N * N, (total_q, G * N * N)            # every pair of cells counted once per gene

    if not args.no_kernels:
        per_call = {"ranks_emit_kernel": chunks, "ranks_sort_kernel": 4 * chunks, "ranks_fold_kernel": chunks}
        try:
            times = kernel_times(args)
        except (OSError, subprocess.SubprocessError) as e:
            print("the rocprofv3 run failed: %s" % e)
            times = {}
        for kernel in KERNELS:
            if kernel not in times:
                print("%-28s not found in the trace" % kernel)
                continue
            launches, avg = times[kernel]
            whole = avg * per_call[kernel] * 1e-6
            print("%-28s %9.3f ms per launch (%d launches traced), %8.2f ms per call = %.2f TB/s at %d bytes per entry"
                  % (kernel, avg * 1e-6, launches, whole, BYTES_PER_ENTRY[kernel] * entries * (4 if "sort" in kernel else 1)
                     / (whole * 1e-3) / 1e12, BYTES_PER_ENTRY[kernel]))
        if "ranks_sort_kernel" in times:
            print("the four sort passes of one whole chunk of %d genes (the call's sort time x %d / %d): %.2f ms"
                  % (gpp, gpp, G, 4 * chunks * times["ranks_sort_kernel"][1] * 1e-6 * gpp / G))

    # the yardstick: torch's stable sort of one chunk of keys (values and indices out, as torch.sort always gives both)
    inv = op.inv_size.to(torch.float32)
    keys = torch.log1p(op.counts[:, :gpp].to(torch.float32) * inv[:, None]).t().contiguous().view(torch.int32)
    med, lo, hi = events(lambda: torch.sort(keys, dim=1, stable=True))
    print("torch.sort(dim=1, stable) of one chunk, %d x %d int32: %.2f ms (min %.2f, max %.2f); x %d chunks = %.1f ms"
          % (gpp, N, med, lo, hi, chunks, med * chunks))

    ms, rs = wall(lambda: ranks.rank_sums(X, sc, labels))
    print("ranks.rank_sums end to end   %9.2f ms (labels on the host in, %d x %d integers on the host out)" % (ms, K, G))
    ms, res = wall(lambda: markers.rank_genes_groups(X, sc, labels, method="wilcoxon"))
    print("rank_genes_groups, wilcoxon  %9.2f ms end to end (labels on the host in, %d x %d ranking on the host out)" % (ms, K, G))
    ms, _ = wall(lambda: markers.rank_genes_groups(X, sc, labels))
    print("rank_genes_groups, t-test    %9.2f ms end to end, for comparison" % ms)

    if args.scipy:
        import scipy.stats
        n_small, g_small, k = min(5000, N), min(2000, G), 8
        sub = op.counts[:n_small, :g_small].contiguous()
        s = np.asarray(sc, dtype=np.float64)[op.matrix.cell_of_row[:n_small] if op.matrix.cell_of_row is not None else slice(0, n_small)]
        small = rng.permutation(np.arange(n_small) % k)
        ms, got = wall(lambda: ranks.rank_sums(sub, s, small))
        t0 = time.perf_counter()
        host = sub.cpu().numpy()
        t1 = time.perf_counter()
        A = np.log1p(host / s[:, None]).astype(np.float32)
        t2 = time.perf_counter()
        sums = np.empty((k, g_small))
        for j in range(g_small):
            r = scipy.stats.rankdata(A[:, j])
            sums[:, j] = np.bincount(small, weights=r, minlength=k)
        t3 = time.perf_counter()
        # (numpy's float32 log1p is not the device's entry to the bit: a tie here may not be one there; the sums agree closely)
        apart = float(np.abs((got.q + got.n[:, None]) / 2.0 - sums).max())
        print("%d x %d, K = %d: ranks.rank_sums %.2f ms; the host route: copy %.1f ms, log1p %.1f ms, rankdata per gene %.1f ms "
              "(%d threads visible); largest difference of a rank sum %.1f" % (n_small, g_small, k, ms, (t1 - t0) * 1e3,
                                                                            (t2 - t1) * 1e3, (t3 - t2) * 1e3, os.cpu_count() or 1, apart))


if __name__ == "__main__":
    main()
