"""
Times of the mapping of cells onto the tree (prosstt_amd/mapping.py, libprosstt_amd_mapping.so) on the device, on the sampled
workload C3 (50 000 cells x 20 000 genes) with the nodes of its own tree, warm; on all genes and on 2 000 genes chosen by
``hvg.highly_variable_genes`` / ``hvg.select_genes``:

  * the native call (pass and finish kernel, HIP events, the median of --reps), the same call on the first 32 genes alone
    (the finish kernel, the epilogue's stores and a pass of one step: what is not the product), and from their difference
    the rate of the product as a share of 155 TF of f32 MFMA;
  * a sweep of ``genes_per_chain`` over 64 / 256 / 1 024 and of the node tile over 1 .. 4;
  * ``map_cells`` end to end (wall time: the panel on the host, the pass, the posteriors);
  * with --torch, the same scores by torch on the same device: chunks of ``X.float() @ P.T`` in float32, then the binary64
    bias, argmax and logsumexp; and how far its scores are from the library's;
  * with --host, the numpy model (tests/mapping_model.py) at 5 000 x 2 000.

    python tools/mapping_bench.py [--cells N] [--genes G] [--reps 3] [--torch] [--host]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()

    import torch
    from prosstt_amd import _native, device, fit, hvg, mapping, simulation as sim, workloads
    from prosstt_amd.device import _ptr
    work = workloads.build("C3", G=args.genes)
    N = args.cells or workloads.CONFIGS["C3"]["N"]
    np.random.seed(1)
    X, pt, br, sc = sim.sample_density(work.tree, N, alpha=work.alpha, beta=work.beta, seed=5, out="torch", order="plan")
    N, G = X.shape
    sc = np.asarray(sc, dtype=np.float64)
    truth = sim.cell_rows(work.tree, pt, br)
    means = fit.simulation_means(work.tree)
    table = mapping.node_table(work.tree)
    R, B = means.shape[0], len(table.names)
    print("device: %s; C3: %d cells x %d genes, %d nodes in %d branches" % (torch.cuda.get_device_name(0), N, G, R, B))

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

    L = _native.load("mapping")

    def native(view, panel, exposure, chain, tile):
        """The native call alone on device arrays prepared once: (median, min, max) ms."""
        m = device.CountMatrix(view, "mapping_bench").on_device()
        P = torch.as_tensor(np.ascontiguousarray(panel)).cuda()
        s_d, m_d, c_d, o_d = (torch.as_tensor(a).cuda() for a in (sc, exposure, np.zeros(R), table.offsets))
        ws = m.workspace("mapping", "prosstt_amd_mapping_workspace_bytes", R, B)
        best = torch.empty(m.N, dtype=torch.int32, device="cuda")
        outs = [torch.empty(m.N, dtype=torch.float64, device="cuda") for _ in range(2)]
        branch_lse = torch.empty((m.N, B), dtype=torch.float64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")

        def call():
            _native.check(L.prosstt_amd_mapping_node_scores_tiled(
                m.stream(), _ptr(m.X), m.N, m.G, m.ld, _ptr(s_d), _ptr(P), P.stride(0), R, _ptr(m_d), _ptr(c_d), _ptr(o_d), B,
                chain, tile, _ptr(ws), ws.numel(), _ptr(best), _ptr(outs[0]), _ptr(outs[1]), _ptr(branch_lse), None,
                _ptr(status)), "mapping")
        ms = events(call)
        assert int(status.item()) == 0
        return ms

    selected = hvg.highly_variable_genes(X, sc, n_top_genes=min(2000, G)).genes
    Xs = hvg.select_genes(X, selected)
    for name, view, mu in (("%d selected genes" % Xs.shape[1], Xs, means[:, selected]), ("all %d genes" % G, X, means)):
        g = view.shape[1]
        panel, exposure = mapping.poisson_panel(mu)
        whole = native(view, panel, exposure, 256, 0)
        rest = native(view[:, :32], np.ascontiguousarray(panel[:, :32]), exposure, 256, 0)
        flops = 2.0 * N * R * g
        product = max(whole[0] - rest[0], 1e-6)
        print("%-20s native call %8.2f ms (min %.2f, max %.2f); on 32 genes alone (finish, stores, one step) %6.2f ms; the "
              "product %8.2f ms = %.1f TF, %.1f %% of %g TF" % (name, whole[0], whole[1], whole[2], rest[0], product,
                                                               flops / product / 1e9, 100 * flops / product / 1e9 / PEAK_TF,
                                                               PEAK_TF))
        for chain in (64, 256, 1024):
            print("    genes_per_chain %-5d  %8.2f ms (min %.2f, max %.2f)" % ((chain,) + native(view, panel, exposure, chain, 0)))
        for tile in (1, 2, 3, 4):
            print("    node_tile %-5d        %8.2f ms (min %.2f, max %.2f)" % ((tile,) + native(view, panel, exposure, 256, tile)))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = mapping.node_scores(view, sc, panel, exposure, None, table.offsets, scores=args.torch, out="torch")
        torch.cuda.synchronize()
        wrapped = time.perf_counter() - t0
        node = got.best.cpu().numpy()
        print("    node_scores through the wrapper %.3f s; %.1f %% of the cells on their true node, %.1f %% on their true branch"
              % (wrapped, 100 * np.mean(node == truth), 100 * np.mean(table.branch_code[node] == table.branch_code[truth])))
        if args.torch:
            P = torch.as_tensor(panel).cuda()
            m_d, s_d = torch.as_tensor(exposure).cuda(), torch.as_tensor(sc).cuda()
            chunk = 8192

            def by_torch():
                S = torch.empty((N, R), dtype=torch.float64, device="cuda")
                for lo in range(0, N, chunk):
                    D = view[lo:lo + chunk].float() @ P.T
                    S[lo:lo + chunk] = D.double() - s_d[lo:lo + chunk, None] * m_d[None, :]
                return S, S.argmax(dim=1), torch.logsumexp(S, dim=1)

            ms = events(by_torch)
            S, arg, _ = by_torch()
            print("    by torch, %d cells at a time: float32 matmul, binary64 bias, argmax, logsumexp %8.2f ms (min %.2f, max "
                  "%.2f); largest |S - ours| %.3g, %d of %d cells with another node"
                  % (chunk, ms[0], ms[1], ms[2], float((S - got.scores).abs().max()), int((arg != got.best).sum()), N))
            del S, got

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = mapping.map_cells(X, sc, work.tree)
    print("map_cells end to end on all genes %.2f s; mean posterior of the best node %.3f" % (time.perf_counter() - t0,
                                                                                              float(m.posterior.mean())))

    if args.host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import mapping_model as mm
        n, g = min(5000, N), min(2000, G)
        host = X[:n, :g].cpu().numpy()
        panel, exposure = mapping.poisson_panel(means[:, :g])
        t0 = time.perf_counter()
        S = mm.scores(host, sc[:n], panel, exposure)
        arg, total = np.argmax(S, axis=1), mm.lse(S)
        model = time.perf_counter() - t0
        view = X[:n, :g]
        ms = events(lambda: mapping.node_scores(view, sc[:n], panel, exposure, out="torch"))
        got = mapping.node_scores(view, sc[:n], panel, exposure)
        print("%d x %d x %d nodes: the numpy model (binary64 matmul, argmax, log-sum-exp) %.2f s (%d threads visible); "
              "node_scores on the device %.2f ms; %d cells with another node, largest |lse - model| %.3g"
              % (n, g, R, model, os.cpu_count() or 1, ms[0], int((got.best != arg).sum()), float(np.abs(got.lse - total).max())))


if __name__ == "__main__":
    main()
