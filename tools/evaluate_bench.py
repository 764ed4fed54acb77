"""
Times of the trajectory scores (prosstt_amd/evaluate.py, libprosstt_amd_evaluate.so) on the device, at --cells cells of the
density plan of the 8-branch tree (C3) and the 32-branch tree (T32) of prosstt_amd/workloads.py.  The found trajectory is the
truth with noise (a quarter of the cells on a wrong branch, the pseudotime jittered by --jitter steps), on the true tree as
the second tree: the times do not depend on what the answer is.

  * each pass (pair counts, pair moments) per ``tiles_per_block`` of --tiles (0: the library's choice), as a bare C call on
    sorted device arrays: HIP events around the three launches, warm, the median of --reps, and the pairs per second that
    makes; beside it the same call on two cells, which does no work: what of the call is launch cost;
  * ``evaluate.trajectory`` on a ``ptree.LineageFit`` end to end (labels, ordering, distances; host arrays in, floats out):
    wall time, the median of --reps;
  * with --scipy, ``scipy.stats.kendalltau`` on the host, over all cells and per comparable class pair (the union of the two
    classes, which also holds the pairs inside either).  It sorts and counts inversions, O(N log N), where the pass counts all
    N^2 / 2 pairs: it is the faster way to ONE tau; the pass gives every class pair's four sums at once, exactly;
  * with --torch, the five distance sums over all pairs by torch on the same device, in chunks of --chunk rows (int64
    broadcasting, one (chunk, N) tensor per intermediate), not binned by class;
  * with --numpy, the numpy model (tests/evaluate_model.py) at --model-cells cells on the host.

    python tools/evaluate_bench.py [--cells 50000] [--reps 5] [--tiles 1,2,4,8,16,64,0] [--scipy] [--torch] [--numpy]
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


def workload_tree(name):
    """The topology of a configuration of prosstt_amd/workloads.py as a ``Tree`` without genes."""
    from prosstt_amd import workloads
    from prosstt_amd.tree import Tree
    cfg = workloads.CONFIGS[name]
    np.random.seed(cfg["seed"])
    topology, labels = workloads.topology_of(cfg)
    return Tree(topology=topology, time={b: cfg["T"] for b in labels}, num_branches=len(labels),
                branch_points=len({p for p, _ in topology}), modules=0, G=4), cfg


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", default="1,2,4,8,16,64,0")
    ap.add_argument("--jitter", type=float, default=4.0)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--model-cells", type=int, default=5000)
    ap.add_argument("--trees", default="C3,T32")
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--torch", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    args = ap.parse_args()

    import torch
    import evaluate_model as em
    from prosstt_amd import _native, evaluate, ptree, simulation as sim
    from prosstt_amd.device import _ptr
    from prosstt_amd.trends import _Nodes
    L = _native.load("evaluate")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    print("device: %s" % torch.cuda.get_device_name(0))

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

    def passes(h, a, b, h2, c2, offsets, J, J2, K, K2, tiles):
        """((ms of the counts), (ms of the moments), counts, words) of bare calls on sorted device arrays."""
        n = h.numel()
        need = ctypes.c_uint64(0)
        _native.check(L.prosstt_amd_evaluate_workspace_bytes(n, K, tiles, ctypes.byref(need)), "evaluate")
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        counts = torch.empty((K, K, 4), dtype=torch.int64, device="cuda")
        words = torch.empty((K, K, 5, 2), dtype=torch.int64, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        tc = events(lambda: _native.check(L.prosstt_amd_evaluate_pair_counts(
            stream, _ptr(a), _ptr(b), _ptr(offsets), n, K, tiles, _ptr(ws), ws.numel(), _ptr(counts), _ptr(status)), "evaluate"))
        tm = events(lambda: _native.check(L.prosstt_amd_evaluate_pair_moments(
            stream, _ptr(h), _ptr(h2), _ptr(c2), _ptr(offsets), _ptr(J), _ptr(J2), n, K, K2, tiles, _ptr(ws), ws.numel(),
            _ptr(words), _ptr(status)), "evaluate"))
        assert int(status.item()) == 0
        return tc, tm, counts, words, int(need.value)

    for name in args.trees.split(","):
        tree, cfg = workload_tree(name)
        np.random.seed(cfg["seed"] + 1)
        pt, br = sim._density_plan(tree, args.cells)
        pt, br = np.asarray(pt), np.asarray(br)
        N = len(pt)
        nodes = _Nodes(tree)
        K = len(nodes.names)
        rng = np.random.default_rng(cfg["seed"])
        codes = nodes.codes(br)
        wrong = rng.random(N) < 0.25
        found_codes = np.where(wrong, rng.integers(0, K, N), codes)
        found_br = np.array(nodes.names)[found_codes]
        position = np.clip(pt + rng.normal(0.0, args.jitter, N), nodes.first[found_codes], nodes.last[found_codes])
        lf = ptree.LineageFit(tree, found_br, np.rint(position).astype(np.int64), position, np.zeros(N, dtype=np.int32),
                              np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64))
        print("\n%s: %d branches, %d cells, %d pairs; sizes of the classes %d .. %d"
              % (name, K, N, N * (N - 1) // 2, np.bincount(codes, minlength=K).min(), np.bincount(codes, minlength=K).max()))

        ticks = 16
        h, _, J = evaluate._depths(nodes, pt, br, ticks, "the true tree")
        h2, _, J2 = evaluate._depths(nodes, position, found_br, ticks, "the second tree")
        order, offsets = em.by_class(codes, K)
        a = np.unique(pt, return_inverse=True)[1]
        b = np.unique(position, return_inverse=True)[1]
        dev = [torch.from_numpy(np.ascontiguousarray(v[order]).astype(np.int32)).cuda() for v in (h, a, b, h2, found_codes)]
        d_off, d_J, d_J2 = torch.from_numpy(offsets).cuda(), torch.from_numpy(J).cuda(), torch.from_numpy(J2).cuda()

        two = [torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(5)]
        tc, tm, _, _, _ = passes(*two, torch.tensor([0, 2], device="cuda"), d_J[:1, :1].contiguous(), d_J2[:1, :1].contiguous(), 1, 1, 0)
        print("a call that does no work (two cells, three launches): counts %.4f ms (min %.4f, max %.4f), moments %.4f ms "
              "(min %.4f, max %.4f)" % (tc + tm))
        first = None
        for tiles in (int(v) for v in args.tiles.split(",")):
            tc, tm, counts, words, need = passes(*dev, d_off, d_J, d_J2, K, K, tiles)
            first = (counts.clone(), words.clone()) if first is None else first
            same = bool((counts == first[0]).all() & (words == first[1]).all())
            chosen = tiles or em.default_tiles(N, K)
            print("tiles_per_block %4d%s  counts %8.4f ms (min %.4f, max %.4f) %.3g pairs/s;  moments %8.4f ms (min %.4f, max "
                  "%.4f) %.3g pairs/s;  workspace %.1f MB;  equal to the first: %s"
                  % (tiles, " (= %d)" % chosen if not tiles else "", tc[0], tc[1], tc[2], 0.5 * N * N / (1e-3 * tc[0]), tm[0],
                     tm[1], tm[2], 0.5 * N * N / (1e-3 * tm[0]), need / 1e6, same))

        ms, ev = wall(lambda: evaluate.trajectory(tree, pt, br, lf))
        print("trajectory(LineageFit)  %9.3f ms end to end: accuracy %.4f, ARI %.4f, NMI %.4f; gamma all %.4f, comparable %.4f, "
              "within %.4f; tau-b all %.4f; Spearman %.4f; distance correlation %.4f"
              % (ms, ev.labels.accuracy, ev.labels.ari, ev.labels.nmi, ev.ordering.overall.gamma, ev.ordering.comparable.gamma,
                 ev.ordering.within.gamma, ev.ordering.overall.tau_b, ev.ordering.spearman, ev.distances.pearson()))

        if args.scipy:
            import scipy.stats
            t0 = time.perf_counter()
            tau = scipy.stats.kendalltau(pt, position).statistic
            whole = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            n_pairs = 0
            for p in range(K):
                for q in range(p, K):
                    if ev.ordering.comparable_mask[p, q]:
                        sel = (codes == p) | (codes == q)
                        if sel.sum() > 1:
                            scipy.stats.kendalltau(pt[sel], position[sel])
                            n_pairs += 1
            per_pair = (time.perf_counter() - t0) * 1e3
            print("scipy.stats.kendalltau on the host, O(N log N): all cells %.1f ms (tau-b %.6f, ours %.6f); %d comparable class "
                  "pairs one after the other %.1f ms" % (whole, tau, ev.ordering.overall.tau_b, n_pairs, per_pair))

        if args.torch:
            dh, _, _, dh2, dc2 = (v.to(torch.int64) for v in dev)
            dc = torch.repeat_interleave(torch.arange(K, device="cuda"), torch.from_numpy(np.diff(offsets)).cuda())
            J64, J264 = d_J.to(torch.int64).reshape(-1), d_J2.to(torch.int64).reshape(-1)

            def chunks():
                sums = torch.zeros(5, dtype=torch.int64, device="cuda")
                for r0 in range(0, N, args.chunk):
                    r1 = min(N, r0 + args.chunk)
                    upper = torch.arange(N, device="cuda")[None, :] > torch.arange(r0, r1, device="cuda")[:, None]
                    d = dh[r0:r1, None] + dh[None, :] - 2 * torch.minimum(torch.minimum(dh[r0:r1, None], dh[None, :]),
                                                                           J64[dc[r0:r1, None] * K + dc[None, :]])
                    e = dh2[r0:r1, None] + dh2[None, :] - 2 * torch.minimum(torch.minimum(dh2[r0:r1, None], dh2[None, :]),
                                                                             J264[dc2[r0:r1, None] * K + dc2[None, :]])
                    d, e = d * upper, e * upper
                    sums += torch.stack([d.sum(), e.sum(), (d * d).sum(), (e * e).sum(), (d * e).sum()])
                return sums
            ms, sums = wall(chunks)
            ours = [sum(t.ravel().tolist()) for t in (ev.distances.d, ev.distances.d2, ev.distances.dd, ev.distances.d2d2,
                                                      ev.distances.dd2)]
            print("torch, the five sums in chunks of %d rows on the device: %.1f ms; equal to the pass (mod 2^64): %s"
                  % (args.chunk, ms, [int(v) % (1 << 64) for v in sums.cpu()] == [v % (1 << 64) for v in ours]))

        if args.numpy:
            n = min(args.model_cells, N)
            keep = np.sort(rng.choice(N, n, replace=False))
            o, off = em.by_class(codes[keep], K)
            t0 = time.perf_counter()
            em.pair_counts(a[keep][o], b[keep][o], off)
            t1 = time.perf_counter()
            em.pair_moments(h[keep][o], off, J, h2[keep][o], found_codes[keep][o], J2)
            t2 = time.perf_counter()
            print("the numpy model at %d cells on the host (%d threads visible): counts %.2f s, moments %.2f s"
                  % (n, os.cpu_count() or 1, t1 - t0, t2 - t1))


if __name__ == "__main__":
    main()
