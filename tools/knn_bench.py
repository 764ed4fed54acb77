"""
Times of the exact neighbour search (prosstt_amd/neighbors.py, libprosstt_amd_knn.so) on the device:

  * knn at C3's and T32's cell counts on a fixed-seed random float32 panel with d = 50 and on embed.pca's scores of the
    sampled matrix, k = 14, 100 and 700: HIP events around the bare C call, warm, mean of --reps, for every --chunk-rows
    (0: the library's choice; a chunk whose slab is far above 256 MiB shows what the last-level cache is worth to the
    selection's re-reads);
  * beside it, on the same device, what a user would write without the library: torch.cdist(P[lo:hi], P).topk(k + 1,
    largest=False) chunked by the same rows, self dropped; and the share of rows whose index list differs from the
    library's (cdist takes the Gram form, which is why it is not the definition);
  * with --sklearn, sklearn.neighbors.NearestNeighbors(algorithm="brute") on the host, on the first panel, if importable.

The split of a call over its two kernels comes from the same run under a kernel trace (in a run of its own):

    rocprofv3 --kernel-trace --stats -d out -- python tools/knn_bench.py --configs C3 --panels random --reps 3

    python tools/knn_bench.py [--configs C3,T32] [--panels random,pca] [--ks 14,100,700] [--chunk-rows 0] [--reps 5] [--sklearn]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def device_panel(host):
    """The f32 device panel of a host array as neighbors.knn stages it: rows padded to 16 bytes (the 16-byte load path)."""
    import torch
    N, d = host.shape
    wide = torch.empty((N, -(-d // 4) * 4), dtype=torch.float32, device="cuda")
    wide[:, :d].copy_(torch.as_tensor(np.ascontiguousarray(host, dtype=np.float32)))
    return wide[:, :d]


def library_ms(P, k, chunk, reps):
    """(ms per bare C call, warm; indices; rows per chunk) of the search over the f32 device panel P."""
    import torch
    from prosstt_amd import _native, device
    L = _native.load("knn")
    p = device._ptr
    N, d = P.shape
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_knn_workspace_bytes(N, d, k, chunk, ctypes.byref(need)), "knn")
    ws = torch.empty(need.value, dtype=torch.uint8, device=P.device)
    index = torch.empty((N, k), dtype=torch.int32, device=P.device)
    sqdist = torch.empty((N, k), dtype=torch.float32, device=P.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _native.check(L.prosstt_amd_knn_search(st, p(P), N, d, P.stride(0), k, chunk, p(index), p(sqdist), p(ws),
                                               ws.numel()), "knn")
    call()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    stop.synchronize()
    rows = chunk if chunk else need.value // (4 * (-(-N // 64) * 64)) // 64 * 64
    return start.elapsed_time(stop) / reps, index, min(rows, N) if rows else N


def cdist_ms(P, k, rows, reps):
    """(ms per pass, warm; indices) of torch.cdist + topk in chunks of ``rows`` queries, self dropped."""
    import torch
    N = P.shape[0]
    out = torch.empty((N, k), dtype=torch.int64, device=P.device)

    def run():
        for lo in range(0, N, rows):
            out[lo:lo + rows] = torch.cdist(P[lo:lo + rows], P).topk(k + 1, largest=False).indices[:, 1:]
    run()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        run()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3,T32")
    ap.add_argument("--panels", default="random,pca")
    ap.add_argument("--ks", default="14,100,700")
    ap.add_argument("--chunk-rows", default="0", help="comma-separated chunk_rows values; 0: the library's choice")
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true", help="scikit-learn's brute-force neighbours on the host, on the first panel")
    args = ap.parse_args()
    import torch
    from prosstt_amd import simulation as sim, workloads, embed
    torch.cuda.set_device(0)
    ks = [int(v) for v in args.ks.split(",") if v]
    chunks = [int(v) for v in args.chunk_rows.split(",") if v]
    kinds = [v for v in args.panels.split(",") if v]
    done_random = set()
    for name in [c for c in args.configs.split(",") if c]:
        work = workloads.build(name)
        N = work.cfg["N"]
        panels = []
        if "random" in kinds and N not in done_random:             # (C3 and T32 have the same cell count: once)
            done_random.add(N)
            rng = np.random.default_rng(20261018)
            panels.append(("random", device_panel(rng.standard_normal((N, args.d)))))
        if "pca" in kinds:
            pt, br, sc, _ = work.plan()
            presented = sim.draw_counts(work.tree, pt, br, sc, work.alpha, work.beta, seed=1, out="torch")
            scores = embed.pca(presented, sc, args.d).scores
            del presented
            torch.cuda.empty_cache()
            panels.append(("pca scores", device_panel(scores)))
        for what, P in panels:
            for k in ks:
                rows = None
                for chunk in chunks:
                    ms, index, rows_used = library_ms(P, k, chunk, args.reps)
                    rows = rows_used if rows is None else rows
                    print("%s %-10s %d x %d, k = %3d, chunk_rows = %d (%d rows, slab %.0f MiB): knn %.2f ms per call "
                          "(mean of %d, warm)" % (name, what, N, P.shape[1], k, chunk, rows_used,
                                                  rows_used * N * 4 / 2 ** 20, ms, args.reps), flush=True)
                    if chunk == chunks[0]:
                        first = index.clone()
                    else:
                        assert torch.equal(first, index), "the result depends on chunk_rows"
                ms, other = cdist_ms(P.contiguous(), k, rows, max(1, args.reps // 2))
                differ = float((other != first.long()).any(dim=1).float().mean())
                print("%s %-10s %d x %d, k = %3d: torch.cdist + topk in chunks of %d rows %.2f ms; %.2f %% of its rows "
                      "differ from the library's index lists" % (name, what, N, P.shape[1], k, rows, ms, 100 * differ),
                      flush=True)
                del other
            if args.sklearn and what == panels[0][0] and name == args.configs.split(",")[0]:     # once
                try:
                    from sklearn.neighbors import NearestNeighbors
                except ImportError:
                    print("%s %s scikit-learn: not importable, skipped" % (name, what), flush=True)
                else:
                    host = P.cpu().numpy()
                    t0 = time.perf_counter()
                    NearestNeighbors(n_neighbors=ks[0] + 1, algorithm="brute").fit(host).kneighbors(host)
                    print("%s %-10s scikit-learn NearestNeighbors(brute), k = %d on the host: %.0f ms wall"
                          % (name, what, ks[0], (time.perf_counter() - t0) * 1e3), flush=True)
            del P
        del work, panels
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
