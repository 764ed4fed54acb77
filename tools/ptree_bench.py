"""
Times of the principal-tree passes (prosstt_amd/ptree.py, libprosstt_amd_ptree.so) on the device, warm, on Gaussian cells
around a Y of three branches: 50 000 cells x 50 and x 15 coordinates, 400 nodes.

  * one soft pass and one hard pass of the native call (HIP events, the median of --reps warm calls, with min and max), beside
    the same number of bare launches of an empty torch operation on the same stream (what a launch costs);
  * the project pass on the spanning tree's edges;
  * ``principal_tree`` end to end (wall time) with the host's share per iteration: Prim's tree, the solve and the copies back;
  * ``kmeans(k = 400)``;
  * with --torch, the same sums by torch on the same device in binary64 (``torch.cdist``, softmax, ``R.T @ Y``);
  * with --numpy, the numpy model (tests/ptree_model.py) of one soft pass at 5 000 cells x 50.

    python tools/ptree_bench.py [--cells N] [--nodes R] [--reps 3] [--torch] [--numpy]
"""
import argparse
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
    ap.add_argument("--nodes", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()

    import torch
    import ptree_model as pm
    from prosstt_amd import _native, device, ptree
    from prosstt_amd.device import _ptr
    N, R = args.cells, args.nodes
    print("device: %s; %d cells, %d nodes" % (torch.cuda.get_device_name(0), N, R))
    L = _native.load("ptree")

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

    for d in (50, 15):
        host, _, _ = pm.three_branches(N, d, 1, noise=0.3)
        Y = torch.from_numpy(host).cuda()
        C_host = pm.initial_centres(host, R, 0)
        C = torch.from_numpy(C_host).cuda()
        sigma = float(np.mean(ptree.assign(Y, C, 0.0).sq_distance.astype(np.float64)))
        edges = ptree.spanning_tree(C_host)
        dev = Y.device
        best = torch.empty(N, dtype=torch.int32, device=dev)
        d2min = torch.empty(N, dtype=torch.float32, device=dev)
        free = torch.empty(N, dtype=torch.float64, device=dev)
        gamma = torch.empty(R, dtype=torch.float64, device=dev)
        sums = torch.empty((R, d), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = device.workspace("ptree", "prosstt_amd_ptree_workspace_bytes", dev, N, d, R, 1)
        e_d = torch.from_numpy(edges).cuda()
        edge = torch.empty(N, dtype=torch.int32, device=dev)
        t_d, q_d = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(2))

        def native(s):
            _native.check(L.prosstt_amd_ptree_assign(device.current_stream(dev), _ptr(Y), N, d, d, _ptr(C), R, d, s, _ptr(ws),
                                                     ws.numel(), _ptr(best), _ptr(d2min), _ptr(free), _ptr(gamma), _ptr(sums),
                                                     None, _ptr(status)), "ptree")

        def native_project():
            _native.check(L.prosstt_amd_ptree_project(device.current_stream(dev), _ptr(Y), N, d, d, _ptr(C), R, d, _ptr(e_d),
                                                      len(edges), _ptr(edge), _ptr(t_d), _ptr(q_d), _ptr(status)), "ptree")

        def bare(count):
            for _ in range(count):
                status.add_(0)

        print("d = %d, sigma = %.4g" % (d, sigma))
        print("  soft pass (4 kernels)  %8.3f ms (min %.3f, max %.3f)" % events(lambda: native(sigma)))
        print("  hard pass (4 kernels)  %8.3f ms (min %.3f, max %.3f)" % events(lambda: native(0.0)))
        print("  project, %d edges     %8.3f ms (min %.3f, max %.3f)" % ((len(edges),) + events(native_project)))
        print("  4 bare launches        %8.3f ms (min %.3f, max %.3f)" % events(lambda: bare(4)))
        assert int(status.item()) == 0

        host_time = {"prim": 0.0, "solve": 0.0, "pass and copies": 0.0}
        original = (ptree.spanning_tree, ptree.centre_step, ptree.assign)

        def timed(name, fn):
            def call(*a, **k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn(*a, **k)
                host_time[name] += time.perf_counter() - t0
                return out
            return call
        ptree.spanning_tree, ptree.centre_step, ptree.assign = (timed("prim", original[0]), timed("solve", original[1]),
                                                                 timed("pass and copies", original[2]))
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit = ptree.principal_tree(Y, R, init="cells", sigma=sigma, n_iter=10, tol=0.0)
            total = time.perf_counter() - t0
        finally:
            ptree.spanning_tree, ptree.centre_step, ptree.assign = original
        passes = len(fit.energy)
        print("  principal_tree, %d centre steps: %.3f s; per iteration Prim's tree %.1f ms, the solve %.1f ms, the pass with its "
              "copies back %.1f ms" % (fit.n_iter, total, 1e3 * host_time["prim"] / passes,
                                       1e3 * host_time["solve"] / max(fit.n_iter, 1), 1e3 * host_time["pass and copies"] / passes))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        km = ptree.kmeans(Y, R, n_iter=10)
        print("  kmeans(k = %d), %d updates: %.3f s" % (R, km.n_iter, time.perf_counter() - t0))

        if args.torch:
            Y64, C64 = Y.double(), C.double()

            def by_torch():
                D = torch.cdist(Y64, C64) ** 2
                r = torch.softmax(-D / sigma, dim=1)
                return r.sum(dim=0), r.T @ Y64, r

            ms = events(by_torch)
            g, s, r = by_torch()
            ours = ptree.assign(Y, C, sigma, out="torch")
            print("  by torch in binary64 (cdist, softmax, R.T @ Y) %8.3f ms (min %.3f, max %.3f); largest |gamma - ours| %.3g, "
                  "|sums - ours| %.3g" % (ms + (float((g - ours.gamma).abs().max()), float((s - ours.sums).abs().max()))))
            del r

    if args.numpy:
        host, _, _ = pm.three_branches(5000, 50, 1, noise=0.3)
        C_host = pm.initial_centres(host, R, 0)
        sigma = float(np.mean(pm.assign(host, C_host, 0.0, False).sq_distance.astype(np.float64)))
        t0 = time.perf_counter()
        pm.assign(host, C_host, sigma)
        model = time.perf_counter() - t0
        Y = torch.from_numpy(host).cuda()
        ms = events(lambda: ptree.assign(Y, C_host, sigma, out="torch"))
        print("5 000 x 50 x %d nodes: the numpy model of one soft pass %.2f s (%d threads visible); ptree.assign on the device "
              "%.2f ms" % (R, model, os.cpu_count() or 1, ms[0]))


if __name__ == "__main__":
    main()
