"""-m gpu: the fold of sorted keyed entries into a CSR matrix (prosstt_amd/csrc/sorted_runs.h) through its two entry points,
prosstt_amd_graph_symmetrize_fold and prosstt_amd_tsne_symmetrize_fold, against the model below: runs longer than two and
empty rows, which a kNN list never produces, and one real symmetrisation over several blocks and on another stream.
indptr and indices are compared exactly and data bit for bit; the outputs are allocated under tests/stale.py's bytes, so an
entry the fold leaves unwritten shows.  Only well-formed inputs: the guards on a bad pos or perm are not provoked."""
import ctypes

import numpy as np
import pytest

import stale

pytestmark = pytest.mark.gpu

# what the two libraries do with a run: (combine(w, b), finish(w, N)), in Python floats, which are binary64 and do not fuse
RULES = {"graph": (lambda w, b: (w + b) - w * b, lambda w, N: w),
         "tsne": (lambda w, b: w + b, lambda w, N: w / (2.0 * N))}


def model(sorted_keys, perm, vals, N, rule):
    """(indptr, indices, data) of the fold: the sorted keys walked in order, a run's values combined from the left."""
    combine, finish = RULES[rule]
    count, indices, data = [0] * N, [], []
    for p, key in enumerate(sorted_keys):
        b = float(vals[perm[p]])
        if p > 0 and sorted_keys[p - 1] == key:
            data[-1] = combine(data[-1], b)
            continue
        count[key >> 32] += 1
        indices.append(key & 0xFFFFFFFF)
        data.append(b)
    indptr = np.concatenate(([0], np.cumsum(count))).astype(np.int64)
    return indptr, np.array(indices, dtype=np.int32), np.array([finish(w, N) for w in data], dtype=np.float64)


def fold(rule, sorted_keys, perm, pos, vals, N, k, nnz, byte):
    """The entry point of library ``rule`` on the current stream: host arrays in, (indptr, indices, data) out."""
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load(rule)
    need = ctypes.c_uint64(0)
    _native.check(_native.load("graph").prosstt_amd_graph_workspace_bytes(N, k, ctypes.byref(need)), "graph")
    half = need.value // 2
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    ws[half:half + 8 * len(vals)].view(torch.float64).copy_(torch.from_numpy(vals))     # the values lie behind the keys
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda() for a in (sorted_keys, perm, pos)]
    with stale.poisoned(byte) as poison:
        indptr = torch.empty(N + 1, dtype=torch.int64, device="cuda")
        indices = torch.empty(nnz, dtype=torch.int32, device="cuda")
        data = torch.empty(nnz, dtype=torch.float64, device="cuda")
    assert poison.fills == 3
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    entry = getattr(L, "prosstt_amd_%s_symmetrize_fold" % rule)
    _native.check(entry(stream, _ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), N, k, nnz, _ptr(ws), ws.numel(), _ptr(indptr),
                        _ptr(indices), _ptr(data)), rule)
    torch.cuda.current_stream().synchronize()
    return indptr.cpu().numpy(), indices.cpu().numpy(), data.cpu().numpy()


def assert_same(got, want):
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2].view(np.int64), want[2].view(np.int64))


def pos_of(sorted_keys):
    head = np.ones(len(sorted_keys), dtype=np.int64)
    head[1:] = sorted_keys[1:] != sorted_keys[:-1]
    return np.cumsum(head)


@pytest.mark.parametrize("rule", sorted(RULES))
def test_long_runs_and_empty_rows(rule):
    N, k = 5, 2
    # (row, column, length of the run): rows 0, 1 and 3; row 2 lies between two heads and row 4 behind the last run
    runs = [(0, 1, 4), (0, 2, 1), (0, 3, 2), (0, 4, 1), (1, 0, 3), (1, 2, 1), (1, 3, 1), (1, 4, 2), (3, 0, 1), (3, 1, 2),
            (3, 2, 1), (3, 4, 1)]
    sorted_keys = np.array([(r << 32) | c for r, c, n in runs for _ in range(n)], dtype=np.int64)
    M, nnz = 2 * N * k, len(runs)
    assert len(sorted_keys) == M and nnz == 12 and N * k <= nnz <= 2 * N * k
    assert {n for _, _, n in runs} == {1, 2, 3, 4} and np.all(np.diff(sorted_keys) >= 0)
    rng = np.random.default_rng(5)
    perm = rng.permutation(M).astype(np.int64)
    vals = rng.uniform(0.0, 1.0, M)
    assert np.all((vals > 0) & (vals < 1))
    want = model(sorted_keys.tolist(), perm.tolist(), vals, N, rule)
    np.testing.assert_array_equal(want[0], [0, 4, 8, 8, 12, 12])
    for byte in stale.BYTES:
        assert_same(fold(rule, sorted_keys, perm, pos_of(sorted_keys), vals, N, k, nnz, byte), want)


def test_a_real_symmetrisation_on_two_streams():
    import torch
    from prosstt_amd import _native, device, graph
    from prosstt_amd.device import _ptr
    N, k = 300, 7
    rng = np.random.default_rng(300)
    # k distinct neighbours of every cell, none the cell itself
    idx = np.stack([rng.permutation(N - 1)[:k] for _ in range(N)])
    idx = (idx + (idx >= np.arange(N)[:, None])).astype(np.int32)
    a = rng.uniform(0.0, 1.0, (N, k))
    L = _native.load("graph")
    ws = device.workspace("graph", "prosstt_amd_graph_workspace_bytes", torch.device("cuda", torch.cuda.current_device()), N, k)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx_d, a_d = torch.from_numpy(idx).cuda(), torch.from_numpy(a).cuda()
    _native.check(L.prosstt_amd_graph_symmetrize_emit(stream, _ptr(idx_d), _ptr(a_d), N, k, _ptr(ws), ws.numel()), "graph")
    M = 2 * N * k
    assert M == 4200 and -(-M // 256) == 17                        # 17 blocks of the fold
    sorted_keys, perm, pos, nnz = graph._sorted_runs(ws[:8 * M].view(torch.int64))
    vals = ws[ws.numel() // 2:][:8 * M].view(torch.float64).cpu().numpy()
    host = [t.cpu().numpy() for t in (sorted_keys, perm, pos)]
    np.testing.assert_array_equal(host[2], pos_of(host[0]))
    assert N * k < nnz < 2 * N * k                                # runs of one entry and runs of two
    for rule in sorted(RULES):
        want = model(host[0].tolist(), host[1].tolist(), vals, N, rule)
        assert_same(fold(rule, *host, vals, N, k, nnz, 0xFF), want)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert_same(fold(rule, *host, vals, N, k, nnz, 0x7F), want)
