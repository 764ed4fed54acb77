"""
Times of the expression trends (prosstt_amd/trends.py, libprosstt_amd_trends.so) on the device, on the sampled workload C3
(50 000 cells x 20 000 genes) with the nodes of its own tree, warm:

  * ``node_sums`` (the native call alone, HIP events, the median of --reps) for ``kernel="nearest"`` and for the tricube
    bandwidths 2, 5 and 10: entries per node, ms, and the bytes of gathered row segments (entries x genes x 4) per second;
    with --sweep, the same for several ``entries_per_block`` beside the library's rule;
  * ``markers.group_moments`` on the same labels (the hard bins: one read of the matrix, float sums as well);
  * with --torch, ``torch.sparse.mm`` of the weights in binary64 with chunks of genes converted to binary64 (S1 only; not
    exact above 2^53);
  * ``expression_trends`` end to end (wall time, once: weights on the host, the pass, the divisions);
  * with --host, the numpy model of the sums (tests/trends_model.py) and scipy's int64 sparse product at 5 000 x 2 000.

    python tools/trends_bench.py [--cells N] [--genes G] [--reps 3] [--sweep] [--torch] [--host]
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, device, markers, simulation as sim, trends, workloads
    from prosstt_amd.device import _ptr
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch", order="plan")
    N, G = X.shape
    print("device: %s; C3: %d cells x %d genes" % (torch.cuda.get_device_name(0), N, G))

    def events(fn):
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

    L = _native.load("trends")
    m = device.CountMatrix(X, "trends_bench").on_device()

    def native(w, epb):
        """The native call alone on device arrays prepared once."""
        R, nnz = w.n_nodes, len(w.indices)
        arrays = [torch.as_tensor(a).cuda() for a in (w.indptr, w.indices, w.weights)]
        ws = device.workspace("trends", "prosstt_amd_trends_workspace_bytes", m.device, R, G, nnz, epb)
        s1 = torch.empty((R, G), dtype=torch.int64, device="cuda")
        s2 = torch.empty((R, G, 2), dtype=torch.int64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")

        def call():
            _native.check(L.prosstt_amd_trends_node_sums(
                m.stream(), _ptr(m.X), N, G, m.ld, _ptr(arrays[0]), _ptr(arrays[1]), _ptr(arrays[2]), R, nnz, epb, _ptr(ws),
                ws.numel(), _ptr(s1), _ptr(s2), _ptr(status)), "trends")
        ms = events(call)
        assert int(status.item()) == 0
        return ms, ws.numel()

    cases = [("nearest", None)] + [("tricube", h) for h in (2.0, 5.0, 10.0)]
    weights = {}
    for kernel, h in cases:
        t0 = time.perf_counter()
        w = trends.node_weights(work.tree, pt, br, h or 3.0, kernel=kernel)
        built = time.perf_counter() - t0
        weights[kernel, h] = w
        nnz, R = len(w.indices), w.n_nodes
        per = np.diff(w.indptr)
        for epb in ((0, 256, 1024, 4096) if args.sweep else (0,)):
            ms, ws_bytes = native(w, epb)
            print("node_sums %-8s h = %-4s entries_per_block %-5d  %d nodes, %9d entries (per node: median %d, max %d)   %8.2f ms "
                  "(min %.2f, max %.2f)   %.2f TB/s of row segments;  workspace %.1f MB;  weights on the host %.2f s"
                  % (kernel, h, epb, R, nnz, int(np.median(per)), int(per.max()), ms[0], ms[1], ms[2],
                     nnz * G * 4 / (ms[0] * 1e-3) / 1e12, ws_bytes / 1e6, built))

    labels = weights["nearest", None].labels
    if labels.max() < markers.MAX_GROUPS:
        ms = events(lambda: markers.group_moments(X, sc, labels, out="torch"))
        print("markers.group_moments on the same labels (whole call)   %8.2f ms (min %.2f, max %.2f)" % ms)
        ms = events(lambda: trends.node_sums(X, weights["nearest", None], out="torch"))
        print("trends.node_sums, kernel nearest (whole call)           %8.2f ms (min %.2f, max %.2f)" % ms)

    if args.torch:
        for key in (("nearest", None), ("tricube", 5.0)):
            w = weights[key]
            W = torch.sparse_csr_tensor(torch.as_tensor(w.indptr).cuda(), torch.as_tensor(w.indices.astype(np.int64)).cuda(),
                                        torch.as_tensor(w.weights.astype(np.float64)).cuda(), size=(w.n_nodes, N))
            chunk = 2048

            def by_torch():
                out = torch.empty((w.n_nodes, G), dtype=torch.float64, device="cuda")
                for lo in range(0, G, chunk):
                    out[:, lo:lo + chunk] = torch.sparse.mm(W, X[:, lo:lo + chunk].to(torch.float64))
                return out

            ms = events(by_torch)
            ours = trends.node_sums(X, w, out="torch").s1
            same = bool((by_torch() == ours.to(torch.float64)).all().item())
            print("S1 by torch.sparse.mm in binary64, %s h = %s, %d genes at a time   %8.2f ms (min %.2f, max %.2f); equal to the "
                  "integers: %s" % (key[0], key[1], chunk, ms[0], ms[1], ms[2], same))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr = trends.expression_trends(X, sc, work.tree, pt, br, bandwidth=5.0)
    print("expression_trends end to end, h = 5   %.2f s;  %d empty nodes, effective cells per node: median %.0f"
          % (time.perf_counter() - t0, len(tr.empty), float(np.median(tr.effective_cells))))

    if args.host:
        import scipy.sparse as sparse
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import trends_model as tm
        n, g = min(5000, N), min(2000, G)
        host = X[:n, :g].cpu().numpy()
        w = trends.node_weights(work.tree, np.asarray(pt)[:n], np.asarray(br)[:n], 5.0)
        t0 = time.perf_counter()
        S1, _ = tm.node_sums(host, w.indptr, w.indices, w.weights)
        model = time.perf_counter() - t0
        Q = sparse.csr_matrix((w.weights.astype(np.int64), w.indices, w.indptr), shape=(w.n_nodes, n))
        t0 = time.perf_counter()
        H = host.astype(np.int64)
        P1, P2 = Q @ H, Q @ (H * H)
        by_scipy = time.perf_counter() - t0
        view = X[:n, :g]
        ms = events(lambda: trends.node_sums(view, w, out="torch"))
        assert np.array_equal(tm.as_int64(S1), P1)
        print("%d x %d, h = 5, %d entries: the numpy model %.2f s; scipy int64 CSR products (S1 and a 64-bit S2) %.2f s "
              "(%d threads visible); node_sums on the device %.2f ms" % (n, g, len(w.indices), model, by_scipy, os.cpu_count() or 1,
                                                                         ms[0]))


if __name__ == "__main__":
    main()
