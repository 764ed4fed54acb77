"""
Times of the diffusion-pseudotime step (prosstt_amd/dpt.py, libprosstt_amd_dpt.so) on the device, on the tests' noisy-Y cloud
(tests/graph_model.py: tree_points) at --cells x --dim with --neighbours neighbours, from the diffusion map that
``graph.diffmap`` gives for ``neighbors.knn``'s graph; the root is the far end of arm 0:

  * a launch of the row kernel (one source, then four), as a bare C call: HIP events around it, warm, the median of --reps;
  * the concordance call (three rotations in one launch, the ranks of the real branching) per ``slabs`` value of --slabs (0:
    the library's choice), as a bare C call: HIP events, warm, the median of --reps, and the pairs per second that makes;
    beside it the same launches on three cells, which do no work: what of the call is launch cost;
  * the whole ``dpt.dpt(n_branchings=1)`` call on the device's diffusion map with the result on the host: wall time, the
    median of --reps; and what it found, against the generator's truth;
  * with --numpy, the time the numpy model (tests/dpt_model.py) takes for the sums of ONE rotation on the host.

    python tools/dpt_bench.py [--cells 50000] [--dim 50] [--neighbours 14] [--reps 5] [--slabs 1,4,0,32] [--numpy]
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
    ap.add_argument("--neighbours", type=int, default=14)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slabs", default="1,4,0,32")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()

    import torch
    import scipy.stats
    import dpt_model
    import graph_model
    from prosstt_amd import _native, dpt, graph, neighbors
    from prosstt_amd.device import _ptr
    L = _native.load("dpt")
    N, d, k = args.cells, args.dim, args.neighbours
    print("device: %s; cloud: tree_points(%d, %d, seed %d), k = %d" % (torch.cuda.get_device_name(0), N, d, N, k))
    points = graph_model.tree_points(N, d, N)
    arm, pos = dpt_model.tree_truth(N, d, N)
    root = int(np.argmax(np.where(arm == 0, pos, -1.0)))
    truth = np.where(arm == 0, pos[root] - pos, pos[root] + pos)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

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

    t0 = time.perf_counter()
    nb = neighbors.knn(torch.from_numpy(points).cuda(), k, out="torch")
    dm = graph.diffmap(nb, out="torch")
    torch.cuda.synchronize()
    print("knn and diffmap (cold)  %9.1f ms; %d Lanczos steps, eigenvalues %s"
          % ((time.perf_counter() - t0) * 1e3, dm.steps, np.array2string(dm.eigenvalues.cpu().numpy()[:4], precision=5)))

    n_dcs = min(10, dm.eigenvectors.shape[1])
    psi, w = dpt._device_map(dm, n_dcs)
    for count in (1, 4):
        sources = torch.arange(count, dtype=torch.int64, device="cuda") * (N // 4) + root % (N // 4)
        out = torch.empty((count, N), dtype=torch.float64, device="cuda")
        med, lo, hi = events(lambda: _native.check(L.prosstt_amd_dpt_rows(
            stream, _ptr(psi), psi.shape[1], _ptr(w), N, n_dcs, _ptr(sources), count, _ptr(out)), "dpt"))
        print("rows, %d source(s)       %9.4f ms (min %.4f, max %.4f): n_dcs = %d" % (count, med, lo, hi, n_dcs))

    ms, (res, stages) = wall(lambda: dpt.dpt(dm, root, n_branchings=1, _stages=True))
    ru, rv = stages["ru"].contiguous(), stages["rv"].contiguous()

    def concordance_ms(u, v, slabs):
        batch, n = u.shape
        need = ctypes.c_uint64(0)
        _native.check(L.prosstt_amd_dpt_workspace_bytes(n, batch, slabs, ctypes.byref(need)), "dpt")
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        lower = torch.empty((batch, n), dtype=torch.int64, device="cuda")
        upper = torch.empty_like(lower)
        return events(lambda: _native.check(L.prosstt_amd_dpt_concordance(
            stream, _ptr(u), _ptr(v), n, batch, slabs, _ptr(ws), ws.numel(), _ptr(lower), _ptr(upper)), "dpt")), lower, upper

    tiny = torch.tensor([[0, 1, 2]] * 3, dtype=torch.int32, device="cuda")
    empty, _, _ = concordance_ms(tiny, tiny, 1)
    print("a concordance call that does no work (three cells, two launches): %.4f ms (min %.4f, max %.4f)" % empty)
    first = None
    for slabs in (int(v) for v in args.slabs.split(",")):
        (med, lo, hi), lower, upper = concordance_ms(ru, rv, slabs)
        first = (lower.clone(), upper.clone()) if first is None else first
        same = bool((lower == first[0]).all() & (upper == first[1]).all())
        print("concordance slabs %4d  %9.4f ms (min %.4f, max %.4f) for 3 x %d^2 pairs: %.3g pairs per second; equal to the first: %s"
              % (slabs, med, lo, hi, N, 3.0 * N * N / (1e-3 * med), same))

    print("dpt(n_branchings=1)    %9.3f ms   (the whole call from the diffusion map, result on the host)" % ms)
    tip_arms, sizes, share, agreement = dpt_model.structure(dict(tips=res.tips, groups=res.groups), arm)
    print("   tips %s in arms %s, splits %s, groups %s, share with a group %.4f, agreement with the true arm %.4f, tau of the "
          "pseudotime %.4f" % (res.tips, tip_arms, res.splits, sizes, share, agreement,
                              scipy.stats.kendalltau(res.pseudotime, truth).statistic))
    ms0, _ = wall(lambda: dpt.dpt(dm, root))
    print("dpt(n_branchings=0)    %9.3f ms" % ms0)

    if args.numpy:
        u, v = ru[:1].cpu().numpy(), rv[:1].cpu().numpy()
        t0 = time.perf_counter()
        lower, upper = dpt_model.concordance(u, v, block=256)
        seconds = time.perf_counter() - t0
        same = np.array_equal(lower[0], first[0][0].cpu().numpy()) and np.array_equal(upper[0], first[1][0].cpu().numpy())
        print("the numpy model, ONE rotation on the host (%d threads visible): %.1f s; equal to the device: %s"
              % (os.cpu_count() or 1, seconds, same))


if __name__ == "__main__":
    main()
