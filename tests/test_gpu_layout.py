"""-m gpu: prosstt_amd.layout (libprosstt_amd_layout.so) against the binary64 model of tests/layout_model.py: one epoch at a
time on every kernel path, the hash bit for bit, repeats and another stream, the spectral vectors against dense eigh, whole
runs by their trustworthiness, refusals through the ABI.

One epoch.  The device and the model get the same binary32 positions, which come from the model's own run (rate 5, seed 0,
the spectral start; the uniform random start on the hub cloud, which is too large for dense eigh): Y^n of the run of E
epochs.  Two stand-ins keep the model's runs within seconds: on the hub cloud, epoch 499 of 500 reads the Y^49 of the run
of 50 instead of a Y^499, and every negative_sample_rate reads the positions of the rate 5 run.  The epoch that is checked
is always the stated one (its schedule, its alpha and its hash).  Trajectories are not compared: on the CPU, binary32 and
binary64 runs differ by 5e-3 after 3 epochs and by more than 5 after 5.

The bound, per coordinate: |device - model| <= 2^-22 |y_old| + (2^-15 + L 2^-24) alpha_n S, with S = sum |term| and L the
number of terms of the row.  It is derived, not tuned: the relative error of a term from delta, d2, powf and the coefficient
stays under 2^-17 and is doubled; the worst-case binary32 summation of L terms is added, and so is the final rounding.
Measured on an MI355X: the largest error over all cases was 0.233 of the bound (the final rounding of
y alone is 0.25 of it)."""
import ctypes
import functools

import numpy as np
import pytest

import graph_model
import layout_model

pytestmark = pytest.mark.gpu

LANES = (4, 16, 64, 0)
EPOCH_SEED = 2024


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()               # (a copy: the shared model arrays are read-only)


def _neighbors(case):
    from prosstt_amd import neighbors
    return neighbors.Neighbors(_cuda(case["idx"]), _cuda(case["d2"]))


def _conn_of(W):
    """The device ``Connectivities`` of a scipy CSR matrix: the model's own bits."""
    from prosstt_amd import graph
    return graph.Connectivities(_cuda(W.indptr.astype(np.int64)), _cuda(W.indices.astype(np.int32)), _cuda(W.data), None, None)


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(W as scipy CSR, the device Connectivities of the same bits) of a named test graph."""
    if name != "hubs":
        W = graph_model.case(*name)["W"]
        return W, _conn_of(W)
    # the 20 000 x 14 test cloud in 50 dimensions, neighbours from the device's own search: its hubs make rows far longer
    # than any group of lanes
    from prosstt_amd import graph, neighbors
    P = graph_model.tree_points(20000, 50, 20014)
    g = graph.connectivities(neighbors.knn(_cuda(P), 14, out="torch"), out="torch")
    W = g.to_csr()
    per_row = np.diff(W.indptr)
    assert per_row.max() > 4 * 64 and per_row.min() >= 14
    return W, g


@functools.lru_cache(maxsize=None)
def _snapshots(name, c, E):
    """{n: Y^n} of the model's run of E epochs (rate 5, seed 0) for the epochs the tests read."""
    W, _ = _graph(name)
    N = W.shape[0]
    if name == "hubs":
        Y = np.random.default_rng(0).uniform(-10, 10, (N, c)).astype(np.float32)
    else:
        Y = layout_model.spectral_start(W, c, 0)
    wanted = (0, 1, 7, E - 1)
    if name == "hubs" and E == 500:
        early = _snapshots(name, c, 50)
        return {0: early[0], 1: early[1], 7: early[7], 499: early[49]}
    out = {}
    for n in range(E):
        if n in wanted:
            out[n] = Y
            Y.setflags(write=False)
        if n == E - 1:
            break
        Y = layout_model.epoch(W, Y, n, E)[0].astype(np.float32)
    return out


def _check_epoch(conn, W, Y, n, E, r, worst, **kw):
    """One epoch on every path against the model; the model's ``Epoch``."""
    from prosstt_amd import layout
    a, b = layout_model.A, layout_model.B
    want = layout_model.epoch(W, Y, n, E, a, b, rate=r, seed=EPOCH_SEED, **kw)
    alpha = float(np.float32(kw.get("alpha0", 1.0) * (1.0 - n / E)))
    bound = 2.0 ** -22 * np.abs(Y.astype(np.float64)) + (2.0 ** -15 + want.L[:, None] * 2.0 ** -24) * alpha * want.S
    Yd = _cuda(Y)
    for lanes in LANES:
        got = layout.optimize(conn, Yd, n, n + 1, n_epochs=E, a=a, b=b, negative_sample_rate=r, seed=EPOCH_SEED,
                              lanes_per_row=lanes, gamma=kw.get("gamma", 1.0), alpha=kw.get("alpha0", 1.0))
        assert got.dtype.is_floating_point and tuple(got.shape) == Y.shape and got.data_ptr() != Yd.data_ptr()
        err = np.abs(got.cpu().numpy().astype(np.float64) - want.Y)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        worst[0] = max(worst[0], float(ratio.max()))
        assert np.all(err <= bound), (lanes, n, E, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
    return want


@pytest.mark.parametrize("r", [0, 5, 31])
@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("name", [(65, 63), (1000, 14), (1000, 100), "hubs"], ids=str)
def test_one_epoch_against_the_model(name, c, r):
    W, conn = _graph(name)
    N = W.shape[0]
    worst, own, moved = [0.0], 0, 0.0
    for E in (50, 500):
        shots = _snapshots(name, c, E)
        for n in (0, 1, 7, E - 1):
            want = _check_epoch(conn, W, shots[n], n, E, r, worst)
            own += want.own
            moved = max(moved, float(np.abs(want.Y - shots[n]).max()))
            assert want.L.max() > 0
        # positions with duplicated rows: the upper half of the cells on one point, so that edges and negative samples
        # meet the d2 = 0 branches
        Y = np.array(shots[7])
        Y[N // 2:] = Y[3]
        want = _check_epoch(conn, W, Y, 7, E, r, worst)
        assert want.coincident > 0 and (r == 0 or want.coincident > want.L.sum() // 8)
    # other constants of the curve and of the step, once
    _check_epoch(conn, W, shots[1], 1, 500, r, worst, gamma=2.5, alpha0=0.37)
    print("%s c = %d rate %d: largest error / bound %.3g; largest move of the model %.3g; samples on their own row %d"
          % (name, c, r, worst[0], moved, own))
    assert moved > 1e-3                                           # (an epoch that moved nothing would check nothing)
    if name == (65, 63) and r > 0:
        assert own > 0                                            # rows of 64 in 65 cells: k = i occurs


def test_negatives_bit_for_bit():
    from prosstt_amd import layout
    r, count = 31, 16
    for seed in (0, 12345, (1 << 64) - 1):
        for epoch in (0, 4095):
            for N in (3, 65, (1 << 31) - 1):
                for e_begin in (0, (1 << 27) - 8, (1 << 32) - 8, 1 << 35):
                    got = layout._negatives(seed, epoch, e_begin, count, r, N).cpu().numpy()
                    e = (np.arange(count, dtype=np.uint64) + np.uint64(e_begin))[:, None]
                    want = layout_model.negatives(seed, epoch, e, np.arange(r)[None, :], N)
                    assert got.dtype == np.int32 and got.shape == (count, r)
                    np.testing.assert_array_equal(got.astype(np.int64), want)
    assert tuple(layout._negatives(1, 0, 5, 0, 31, 65).shape) == (0, 31) and tuple(layout._negatives(1, 0, 5, 4, 0, 65).shape) == (4, 0)
    # more than one block, and a rate that does not divide the block
    got = layout._negatives(9, 17, 1000, 5000, 5, 1000).cpu().numpy()
    want = layout_model.negatives(9, 17, (np.arange(5000) + 1000)[:, None], np.arange(5)[None, :], 1000)
    np.testing.assert_array_equal(got.astype(np.int64), want)


def test_bits_repeat_on_any_stream_and_across_calls():
    import torch
    from prosstt_amd import layout
    for name, c in (((1000, 14), 2), ((1000, 100), 3)):
        W, conn = _graph(name)
        Y = _cuda(_snapshots(name, c, 50)[0])
        kw = dict(n_epochs=50, a=layout_model.A, b=layout_model.B, seed=3)
        for lanes in LANES:
            first = layout.optimize(conn, Y, 0, 3, lanes_per_row=lanes, **kw)
            assert torch.equal(first, layout.optimize(conn, Y, 0, 3, lanes_per_row=lanes, **kw))
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                third = layout.optimize(conn, Y, 0, 3, lanes_per_row=lanes, **kw)
            st.synchronize()
            assert torch.equal(first, third)
            # the ping-pong: an odd and an even number of epochs in one call against one-epoch calls
            step = Y
            for n in range(4):
                step = layout.optimize(conn, step, n, n + 1, lanes_per_row=lanes, **kw)
                if n == 2:
                    assert torch.equal(step, first)
            assert torch.equal(step, layout.optimize(conn, Y, 0, 4, lanes_per_row=lanes, **kw))
            assert torch.equal(Y, layout.optimize(conn, Y, 2, 2, lanes_per_row=lanes, **kw))      # an empty range
            assert not torch.equal(first, layout.optimize(conn, Y, 0, 3, lanes_per_row=lanes, **dict(kw, seed=4)))
        assert torch.equal(Y.cpu(), torch.from_numpy(np.array(_snapshots(name, c, 50)[0])))      # the input is left alone


@pytest.mark.parametrize("N,k", [(300, 5), (1000, 14)])
def test_spectral_vectors_against_dense_eigh(N, k):
    from prosstt_amd import layout
    case = graph_model.case(N, k)
    want_values, want_vectors = layout_model.spectral_vectors(case["W"], 3)
    for source in (_neighbors(case), _conn_of(case["W"])):
        for c in (2, 3):
            values, vectors = layout.spectral_vectors(source, c)
            assert values.shape == (c,) and vectors.shape == (N, c) and vectors.dtype == np.float64
            print("(%d, %d) c = %d: largest eigenvalue error %.3g" % (N, k, c, np.abs(values - want_values[:c]).max()))
            assert np.all(np.abs(values - want_values[:c]) <= 1e-12)
            assert np.all(np.abs(np.linalg.norm(vectors, axis=0) - 1) <= 1e-14)
            first = np.argmax(np.abs(vectors), axis=0)
            assert np.all(vectors[first, np.arange(c)] > 0)
            # spans, not columns: eigenvalues 2 and 3 of these Y-shaped clouds are 5e-5 and 2.7e-4 apart, the fourth 4e-3 away
            Q, _ = np.linalg.qr(want_vectors[:, :2])
            U, _ = np.linalg.qr(vectors[:, :2])
            sine = np.linalg.norm(U - Q @ (Q.T @ U), 2)
            print("   sine of the largest principal angle of components 1 .. 2: %.3g" % sine)
            assert sine <= 1e-6
    v, x = layout.spectral_vectors(_neighbors(case), 2, out="torch")
    assert v.is_cuda and x.is_cuda and np.array_equal(x.cpu().numpy(), layout.spectral_vectors(_neighbors(case), 2)[1])


@pytest.mark.parametrize("source", ["spectral", "random", "device neighbours"])
def test_whole_runs_by_trustworthiness(source):
    import torch
    from prosstt_amd import layout, neighbors
    N, k, E = 1000, 14, 200
    case = graph_model.case(N, k)
    init = "random" if source == "random" else "spectral"
    if source == "device neighbours":
        nb = neighbors.knn(_cuda(case["P"]), k, out="torch")
    else:
        nb = _neighbors(case)
    start, model = layout_model.reference_run(N, k, E, init)
    lay = layout.umap(nb, n_epochs=E, init=init)
    assert isinstance(lay.embedding, np.ndarray) and lay.embedding.dtype == np.float32 and lay.embedding.shape == (N, 2)
    assert lay.n_epochs == E and abs(lay.a - layout_model.A) <= 1e-6 and abs(lay.b - layout_model.B) <= 1e-6
    assert np.all(np.isfinite(lay.embedding))
    again = layout.umap(nb, n_epochs=E, init=init, out="torch")
    assert again.embedding.is_cuda and again.init.is_cuda
    np.testing.assert_array_equal(again.embedding.cpu().numpy(), lay.embedding)
    np.testing.assert_array_equal(again.init.cpu().numpy(), lay.init)
    if init == "random":
        np.testing.assert_array_equal(lay.init, start)
    else:
        assert np.abs(lay.init - start).max() <= 1e-3             # the device's eigenvectors against dense eigh's
    scores = [layout_model.trustworthiness(case["P"], Y, k) for Y in (lay.init, lay.embedding, model)]
    print("%s: trustworthiness of the start %.4f, of the device's layout %.4f, of the model's %.4f" % ((source,) + tuple(scores)))
    assert scores[1] >= scores[2] - 0.005
    assert scores[0] < scores[2] - 0.03                           # a layout that did not move fails
    # a start handed over as positions is the same run
    given = layout.umap(nb, n_epochs=E, init=torch.from_numpy(np.array(lay.init)).cuda())
    np.testing.assert_array_equal(given.embedding, lay.embedding)
    if source == "spectral":
        three = layout.umap(nb, 3, n_epochs=20, seed=5, negative_sample_rate=2, lanes_per_row=64)
        assert three.embedding.shape == (N, 3) and np.all(np.isfinite(three.embedding)) and three.n_epochs == 20


def test_refusals_through_the_abi():
    import torch
    from prosstt_amd import _native, graph, layout
    from prosstt_amd.device import _ptr
    W, conn = _graph((65, 63))
    N, nnz = 65, W.nnz
    Y = _cuda(_snapshots((65, 63), 2, 50)[0])
    # values are checked on the device, by torch
    for value in (float("nan"), float("inf"), -1e-300):
        bad = conn.data.clone()
        bad[17] = value
        with pytest.raises(ValueError, match="finite and >= 0"):
            layout.umap(conn._replace(data=bad), init="random")
        with pytest.raises(ValueError, match="finite and >= 0"):
            layout.optimize(conn._replace(data=bad), Y, 0, 1, n_epochs=5, a=1.0, b=1.0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        layout.umap(conn._replace(data=torch.zeros_like(conn.data)), init="random")
    for field, bad in (("indptr", conn.indptr + 1), ("indices", conn.indices + 1), ("indices", conn.indices - 1)):
        with pytest.raises(ValueError, match="not those of a CSR matrix"):
            layout.umap(conn._replace(**{field: bad}), init="random")
    # everything else is refused by the library before anything is enqueued
    L = _native.load("layout")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = conn.data / conn.data.max()
    y1 = torch.full((N, 2), -7.0, dtype=torch.float32, device="cuda")
    before = Y.clone()

    def epochs(**kw):
        a = dict(N=N, nnz=nnz, c=2, y0=Y, y1=y1, begin=0, end=1, E=50, a=1.0, b=1.0, gamma=1.0, alpha=1.0, r=5, lanes=0)
        a.update(kw)
        return L.prosstt_amd_layout_epochs(stream, _ptr(conn.indptr), _ptr(conn.indices), _ptr(p), a["N"], a["nnz"], a["c"],
                                           _ptr(a["y0"]), _ptr(a["y1"]), a["begin"], a["end"], a["E"], a["a"], a["b"], a["gamma"],
                                           a["alpha"], a["r"], 7, a["lanes"])

    refusals = [(dict(N=2), "N < 2"), (dict(N=1 << 31), "N < 2"), (dict(nnz=-1), "nnz"), (dict(nnz=N * N), "nnz"),
                (dict(c=1), "c = 2 or 3"), (dict(c=4), "c = 2 or 3"), (dict(E=0), "n_epochs"), (dict(E=4097), "n_epochs"),
                (dict(begin=-1), "epoch_begin"), (dict(begin=2, end=1), "epoch_begin"), (dict(end=51), "epoch_begin"),
                (dict(r=-1), "negative_sample_rate"), (dict(r=32), "negative_sample_rate"), (dict(a=0.0), "finite a"),
                (dict(b=float("nan")), "finite a"), (dict(gamma=-1.0), "finite a"), (dict(alpha=float("inf")), "finite a"),
                (dict(y1=Y), "alias")]
    refusals += [(dict(lanes=lanes), "lanes_per_row") for lanes in (1, 8, 32, 128, -4)]
    for kw, text in refusals:
        with pytest.raises(_native.NativeError, match=text):
            _native.check(epochs(**kw), "layout")
    out = torch.full((4, 31), -7, dtype=torch.int32, device="cuda")
    for args, text in (((0, 4096, 0, 4, 31, 65), "epoch"), ((0, -1, 0, 4, 31, 65), "epoch"), ((0, 0, 0, 4, 32, 65), "rate"),
                       ((0, 0, 0, 4, -1, 65), "rate"), ((0, 0, 0, 4, 31, 2), "N < 2"), ((0, 0, 0, 4, 31, 1 << 31), "N < 2"),
                       ((0, 0, -1, 4, 31, 65), "e_begin"), ((0, 0, 0, -1, 31, 65), "count")):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_layout_negatives(stream, *args, _ptr(out)), "layout")
    torch.cuda.synchronize()
    assert bool((y1 == -7.0).all()) and bool((out == -7).all()) and torch.equal(Y, before)      # nothing was enqueued
    _native.check(epochs(), "layout")                                # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool((y1 != -7.0).all()) and torch.equal(Y, before)
