"""-m gpu: prosstt_amd.tsne (libprosstt_amd_tsne.so) against the binary64 model of tests/tsne_model.py: the conditional
affinities row by row, the joint affinities bit for bit, the gradient on every slab count, the update rule bit for bit,
repeats and another stream, whole runs by their trustworthiness, refusals through the ABI.

The gradient.  The device and the model get the same binary32 positions, which come from the model's own run (the pca
start, the automatic learning rate): Y^n for n = 0, 1, 7, 249 and 250, each with the exaggeration of its iteration, and the
Y^7 with the upper half of the cells moved onto one point.  Later iterations are not used: at iteration 499 of the 300-cell
case 27 % of the gradient's coordinates lie below the error bound, at these five at most 0.1 % do (counted with the model
on the CPU).  Trajectories are not compared.

The bound, per coordinate, T = 256 the tile of the repulsion, L the row's entries, S_A = sum |attraction terms|, S_R = sum
|q^2 delta|:
    |device - model| <= 4 [x (2^-18 + L 2^-23) S_A + (2 (T + 32) 2^-24 + 2^-20) S_R / Z] + 2^-21 (x S_A + S_R / Z)
It is derived, not tuned.  A term of the attraction carries the roundings of delta, d2, w, the reciprocal (1 ulp), the cast
of P and two products, under 2^-20 relative, taken as 2^-19 and doubled; a lane's chain and the shuffle tree add at most L
2^-24 S_A, doubled.  A term of the repulsion carries twice the error of q and three roundings, under 2^-20 S_R; a tile's
binary32 chain adds at most T 2^-24 S_R, and Z's own relative error, (T + 8) 2^-24 by the same argument, divides it: 2 (T +
32) 2^-24 covers both.  The factor 4 is the gradient's; the last term is the cast of R / Z, the product with x and the
subtraction, 2^-24 each, times 4.  |Z - model| <= 2 (T + 8) 2^-24 Z.  Measured on an MI355X: the largest
error over all cases was 0.0675 of the gradient's bound and 0.0255 of Z's."""
import ctypes
import functools

import numpy as np
import pytest

import graph_model
import knn_model
import layout_model
import tsne_model

pytestmark = pytest.mark.gpu

T = tsne_model.TILE
SLABS = (1, 2, 3, 0)
CASES = [(65, 63, 20.0), (300, 90, 30.0), (1000, 14, 4.0)]
SHOTS = (0, 1, 7, 249, 250)


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()               # (a copy: the shared model arrays are read-only)


def _neighbors(idx, d2):
    from prosstt_amd import neighbors
    return neighbors.Neighbors(_cuda(idx), _cuda(d2))


@functools.lru_cache(maxsize=None)
def _aff(case):
    """The device ``Affinities`` of the model's P: the model's own bits."""
    from prosstt_amd import tsne
    cs = tsne_model.case(*case)
    P = cs["P"]
    return tsne.Affinities(_cuda(P.indptr.astype(np.int64)), _cuda(P.indices.astype(np.int32)), _cuda(P.data), _cuda(cs["beta"]))


def _conditional(idx, d2, perplexity):
    """(cond, beta, status word) of the raw entry: host arrays and an int."""
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    L = _native.load("tsne")
    N, k = idx.shape
    idx, d2 = _cuda(idx), _cuda(d2)
    cond = torch.empty((N, k), dtype=torch.float64, device="cuda")
    beta = torch.empty(N, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(L.prosstt_amd_tsne_affinities(stream, _ptr(idx), _ptr(d2), N, k, perplexity, _ptr(cond), _ptr(beta),
                                                _ptr(status)), "tsne")
    return cond.cpu().numpy(), beta.cpu().numpy(), int(status.item())


def _duplicates():
    P = knn_model.KINDS["duplicates"](300, 10, 314)
    return knn_model.model(P, 14)


# ---------------------------------------------------------------------------------------------------------- affinities

@pytest.mark.parametrize("case", CASES + [(1100, 1024, 300.0)], ids=str)
def test_conditional_affinities_against_the_model(case):
    N, k, perplexity = case
    cs = tsne_model.case(*case)
    cond, beta, status = _conditional(cs["idx"], cs["d2"], perplexity)
    assert status == 0
    assert np.all(np.abs(cond.sum(axis=1) - 1.0) <= k * 2.0 ** -52)
    H = tsne_model.row_entropy(cs["d2"], cond)
    print("%s: largest |H(device row) - log perplexity| %.3g" % (case, np.abs(H - np.log(perplexity)).max()))
    assert np.all(np.abs(H - np.log(perplexity)) <= 1e-11)
    d2 = cs["d2"].astype(np.float64)
    g = d2 - d2.min(axis=1)[:, None]
    p, b = cs["cond"], cs["beta"]
    var = (p * g * g).sum(axis=1) - (p * g).sum(axis=1) ** 2
    bound = 4e-12 * g.max(axis=1) / (b * var) + 1e-14
    err = np.abs(cond - p).max(axis=1)
    print("   largest |p - model| / bound %.3g; largest relative beta difference %.3g"
          % ((err / bound).max(), (np.abs(beta - b) / b).max()))
    assert np.all(err <= bound)


def test_degenerate_rows_and_status_bits():
    import torch
    from prosstt_amd import tsne
    idx, d2 = _duplicates()
    assert np.all(d2 == 0)                                       # every row is degenerate
    cond, beta, status = _conditional(idx, d2, 4.0)
    assert status == 0 and np.all(cond == 1.0 / 14) and np.all(beta == 2.0 ** 64)
    model_cond, model_beta = tsne_model.conditional(d2, 4.0)
    assert np.array_equal(cond, model_cond) and np.array_equal(beta, model_beta)
    # rows wider than one slot of the 16 a lane keeps: twelve points a hundred times each.  k = 70: all zero over two
    # slots, uniform rows; k = 130: 99 zeros, more than the perplexity, so beta runs to 2^64 and the rest of the row is 0
    for k in (70, 130):
        wide = graph_model.case(1200, k, 3, "copies100")
        assert np.all(wide["d2"][:, :min(k, 99)] == 0) and np.all(wide["d2"][:, 99:] > 0)
        cond, beta, status = _conditional(wide["idx"], wide["d2"], 20.0)
        model_cond, model_beta = tsne_model.conditional(wide["d2"], 20.0)
        assert np.all(model_beta == 2.0 ** 64)
        if k == 70:
            assert np.all(model_cond == 1.0 / 70)
        else:
            assert np.all(model_cond[:, :99] == 1.0 / 99) and np.all(model_cond[:, 99:] == 0)
        assert status == 0 and np.array_equal(cond, model_cond) and np.array_equal(beta, model_beta)
    # every status bit by its bad value; the good rows are as before
    cs = tsne_model.case(65, 63, 20.0)
    good = _conditional(cs["idx"], cs["d2"], 20.0)[0]
    seen = 0
    for field, value, bit, text in (("idx", 65, tsne.BAD_INDEX, "outside"), ("idx", -1, tsne.BAD_INDEX, "outside"),
                                    ("idx", 1 << 30, tsne.BAD_INDEX, "outside"), ("idx", 7, tsne.BAD_SELF, "own neighbour"),
                                    ("d2", -1.0, tsne.BAD_DISTANCE, "squared distance"),
                                    ("d2", np.inf, tsne.BAD_DISTANCE, "squared distance"),
                                    ("d2", np.nan, tsne.BAD_DISTANCE, "squared distance")):
        idx, d2 = np.array(cs["idx"]), np.array(cs["d2"])
        (idx if field == "idx" else d2)[7, 62] = value
        cond, _, status = _conditional(idx, d2, 20.0)
        assert status == bit, (field, value, status)
        assert np.array_equal(np.delete(cond, 7, axis=0), np.delete(good, 7, axis=0)) and np.all(np.isfinite(cond))
        with pytest.raises(ValueError, match=text):
            tsne.affinities(_neighbors(idx, d2), 20.0)
        seen |= status
    idx, d2 = np.array(cs["idx"]), np.array(cs["d2"])
    idx[0, 0], idx[64, 62], d2[30, 1] = 99, 64, -0.5
    assert _conditional(idx, d2, 20.0)[2] == seen == tsne.BAD_INDEX | tsne.BAD_SELF | tsne.BAD_DISTANCE
    assert torch.cuda.is_available()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_joint_affinities_bit_for_bit(case):
    from prosstt_amd import tsne
    N, k, perplexity = case
    cs = tsne_model.case(*case)
    cond, beta, _ = _conditional(cs["idx"], cs["d2"], perplexity)
    want = tsne_model.joint(cs["idx"], cond)                     # the model's fold of the device's own rows
    for out in ("torch", "scipy"):
        nb = _neighbors(cs["idx"], cs["d2"]) if out == "torch" else (np.array(cs["idx"]), np.array(cs["d2"]))
        aff = tsne.affinities(nb, perplexity, out=out)
        assert (aff.indptr.is_cuda and aff.data.is_cuda) if out == "torch" else isinstance(aff.data, np.ndarray)
        got = aff.to_csr()
        for arr, bits in ((aff.indptr, "int64"), (aff.indices, "int32"), (aff.data, "float64"), (aff.beta, "float64")):
            assert str(arr.dtype).replace("torch.", "") == bits
        np.testing.assert_array_equal(got.indptr, want.indptr)
        np.testing.assert_array_equal(got.indices, want.indices)
        np.testing.assert_array_equal(got.data, want.data)
        np.testing.assert_array_equal(got.indptr, cs["P"].indptr)
        np.testing.assert_array_equal(got.indices, cs["P"].indices)
        assert (got != got.T).nnz == 0 and got.diagonal().max() == 0.0
        assert abs(got.sum() - 1.0) <= 1e-12
        beta_host = aff.beta.cpu().numpy() if out == "torch" else aff.beta
        np.testing.assert_array_equal(beta_host, beta)


# ------------------------------------------------------------------------------------------------------------ gradient

def _check_gradient(case, Y, x, worst):
    from prosstt_amd import tsne
    P = tsne_model.case(*case)["P"]
    want = tsne_model.gradient(P, Y, x, sums=True)
    L = want.L[:, None]
    bound = (4.0 * (x * (2.0 ** -18 + L * 2.0 ** -23) * want.S_A + (2.0 * (T + 32) * 2.0 ** -24 + 2.0 ** -20) * want.S_R / want.Z)
             + 2.0 ** -21 * (x * want.S_A + want.S_R / want.Z))
    Yd = _cuda(Y)
    for slabs in SLABS:
        grad, Z, sums = tsne.gradient(_aff(case), Yd, exaggeration=x, slabs=slabs, _sums=True)
        assert grad.dtype.is_floating_point and tuple(grad.shape) == Y.shape and isinstance(Z, float)
        err = np.abs(grad.cpu().numpy().astype(np.float64) - want.grad)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        worst[0] = max(worst[0], float(ratio.max()))
        worst[1] = max(worst[1], abs(Z - want.Z) / (2.0 * (T + 8) * 2.0 ** -24 * want.Z))
        assert np.all(err <= bound), (slabs, x, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
        assert abs(Z - want.Z) <= 2.0 * (T + 8) * 2.0 ** -24 * want.Z, (slabs, Z, want.Z)
        assert np.all(np.abs(sums.cpu().numpy() - want.S_R) <= 2.0 * (T + 32) * 2.0 ** -24 * want.S_R + 1e-300)
        plain, Z2 = tsne.gradient(_aff(case), Yd, exaggeration=x, slabs=slabs)      # the production path: no sums
        assert Z2 == Z and np.array_equal(plain.cpu().numpy(), grad.cpu().numpy())
    return want


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gradient_against_the_model(case, c):
    N = case[0]
    _, _, shots = tsne_model.reference_run(*case, 251, "pca", c, SHOTS)
    worst, moved = [0.0, 0.0], 0.0
    for n in SHOTS:
        x, _ = tsne_model.schedule(n, 250, 12.0)
        want = _check_gradient(case, shots[n][0], x, worst)
        moved = max(moved, float(np.abs(want.grad).max()))
    Y = np.array(shots[7][0])
    Y[N // 2:] = Y[3]                                             # half the rows on one point: delta = 0, q = 1
    _check_gradient(case, Y, 12.0, worst)
    _check_gradient(case, shots[1][0], 3.7, worst)                # another exaggeration, once
    print("%s c = %d: largest error / bound %.3g (gradient), %.3g (Z); largest gradient entry %.3g"
          % (case, c, worst[0], worst[1], moved))
    assert moved > 0
    if N == 65:                                                   # one tile: slabs 2 and 3 leave slabs empty
        assert -(-N // T) == 1


@pytest.mark.parametrize("c", [2, 3])
def test_update_rule_bit_for_bit(c):
    from prosstt_amd import tsne
    case = (300, 90, 30.0)
    N = case[0]
    eta = tsne_model.auto_learning_rate(N)
    _, _, shots = tsne_model.reference_run(*case, 251, "pca", c, SHOTS)
    rng = np.random.default_rng(c)
    for n in (7, 249, 250):                                       # both sides of the exploration
        x, mu = tsne_model.schedule(n, 250, 12.0)
        states = [shots[n]]
        Y, update, gains = (np.array(a) for a in shots[n])
        gains[:N // 2] = np.float32(0.01)                         # at the floor: 0.8 of it is raised back, + 0.2 is not
        gains[N // 2:3 * N // 4] = np.float32(0.0125)
        update[N // 4:3 * N // 4] = 0.0                           # update grad = 0 is not < 0
        update[-5:] = rng.standard_normal((5, c)).astype(np.float32) * 1e-30      # products that underflow
        states.append((Y, update, gains))
        for Y, update, gains in states:
            for slabs in (0, 3):
                grad = tsne.gradient(_aff(case), _cuda(Y), exaggeration=x, slabs=slabs)[0].cpu().numpy()
                want = tsne_model.step(Y, update, gains, grad, mu, eta)
                got = tsne.optimize(_aff(case), _cuda(Y), n, n + 1, update=_cuda(update), gains=_cuda(gains), exploration=250,
                                    early_exaggeration=12.0, learning_rate=eta, slabs=slabs)
                for name, g, w in zip(("Y", "update", "gains"), got, want):
                    assert g.dtype.is_floating_point and g.is_cuda
                    np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32), err_msg="%s at %d" % (name, n))
        floor = want[2]
        assert (floor == np.float32(0.01)).any() and (want[1] == 0).sum() < want[1].size


def test_bits_repeat_on_any_stream_and_across_calls():
    import torch
    from prosstt_amd import tsne
    for case, c in (((300, 90, 30.0), 2), ((1000, 14, 4.0), 3)):
        start = tsne_model.reference_run(*case, 251, "pca", c, SHOTS)[0]
        Y = _cuda(start)
        kw = dict(learning_rate=tsne_model.auto_learning_rate(case[0]), exploration=2)
        for slabs in (1, 3, 0):
            first = tsne.optimize(_aff(case), Y, 0, 3, slabs=slabs, **kw)
            again = tsne.optimize(_aff(case), Y, 0, 3, slabs=slabs, **kw)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                third = tsne.optimize(_aff(case), Y, 0, 3, slabs=slabs, **kw)
                g3 = tsne.gradient(_aff(case), Y, slabs=slabs)
            st.synchronize()
            g1 = tsne.gradient(_aff(case), Y, slabs=slabs)
            assert g1[1] == g3[1] and torch.equal(g1[0], g3[0])
            for a, b, d in zip(first, again, third):
                assert torch.equal(a, b) and torch.equal(a, d)
            # the ping-pong: an odd and an even number of iterations in one call against one-iteration calls
            step = (Y, None, None)
            for n in range(4):
                step = tsne.optimize(_aff(case), step[0], n, n + 1, update=step[1], gains=step[2], slabs=slabs, **kw)
                if n == 2:
                    assert all(torch.equal(a, b) for a, b in zip(step, first))
            four = tsne.optimize(_aff(case), Y, 0, 4, slabs=slabs, **kw)
            assert all(torch.equal(a, b) for a, b in zip(step, four))
            empty = tsne.optimize(_aff(case), Y, 2, 2, slabs=slabs, **kw)               # an empty range
            assert torch.equal(empty[0], Y) and empty[0].data_ptr() != Y.data_ptr()
            assert bool((empty[1] == 0).all()) and bool((empty[2] == 1).all())
            assert not torch.equal(first[0], Y)
        assert torch.equal(Y.cpu(), torch.from_numpy(np.array(start)))                  # the input is left alone


# ----------------------------------------------------------------------------------------------------------- whole runs

@pytest.mark.parametrize("source", ["panel", "model neighbours", "random"])
def test_whole_runs_by_trustworthiness(source):
    import torch
    from prosstt_amd import tsne
    case = (300, 90, 30.0)
    N, k, perplexity = case
    cs = tsne_model.case(*case)
    panel = cs["P_panel"]
    init = "random" if source == "random" else "pca"
    start, model, _ = tsne_model.reference_run(N, k, perplexity, 500, init)
    if source == "panel":
        X, kw = np.array(panel), dict(init="pca")
    elif source == "model neighbours":
        X, kw = _neighbors(cs["idx"], cs["d2"]), dict(init=np.array(start))
    else:
        X, kw = _neighbors(cs["idx"], cs["d2"]), dict(init="random")
    res = tsne.tsne(X, perplexity=perplexity, n_iter=500, **kw)
    assert isinstance(res.embedding, np.ndarray) and res.embedding.dtype == np.float32 and res.embedding.shape == (N, 2)
    assert res.n_iter == 500 and res.learning_rate == tsne_model.auto_learning_rate(N) == 50.0
    assert np.all(np.isfinite(res.embedding))
    np.testing.assert_array_equal(res.init, start)
    scores = [layout_model.trustworthiness(panel, Y, 15) for Y in (res.init, res.embedding, model)]
    want_kl = tsne_model.gradient(cs["P"], res.embedding).kl
    print("%s: trustworthiness of the start %.4f, of the device's layout %.4f, of the model's %.4f; KL %.6f, the model's at "
          "the same positions %.6f" % ((source,) + tuple(scores) + (res.kl_divergence, want_kl)))
    assert scores[1] >= scores[2] - 0.005
    assert scores[0] < scores[2] - 0.03                           # a layout that did not move fails
    assert abs(res.kl_divergence - want_kl) <= 1e-5 * abs(want_kl)
    Xd = _cuda(panel) if source == "panel" else X
    again = tsne.tsne(Xd, perplexity=perplexity, n_iter=500, out="torch", **kw)
    assert again.embedding.is_cuda and again.init.is_cuda and again.kl_divergence == res.kl_divergence
    np.testing.assert_array_equal(again.embedding.cpu().numpy(), res.embedding)
    # a start handed over as positions, and the affinities handed over, are the same run
    aff = tsne.affinities(_neighbors(cs["idx"], cs["d2"]), perplexity, out="torch")
    if source != "panel":
        given = tsne.tsne(aff, n_iter=500, init=torch.from_numpy(np.array(res.init)).cuda())
        np.testing.assert_array_equal(given.embedding, res.embedding)
    if source == "panel":
        three = tsne.tsne(Xd, 3, perplexity=perplexity, n_iter=20, exploration=10, learning_rate=200.0, slabs=2)
        assert three.embedding.shape == (N, 3) and np.all(np.isfinite(three.embedding)) and three.n_iter == 20
        assert three.learning_rate == 200.0 and np.isfinite(three.kl_divergence)
        none = tsne.tsne(Xd, perplexity=perplexity, n_iter=0)
        np.testing.assert_array_equal(none.embedding, none.init)


# ------------------------------------------------------------------------------------------------------------- refusals

def test_refusals_through_the_abi():
    import torch
    from prosstt_amd import _native, tsne
    from prosstt_amd.device import _ptr
    case = (65, 63, 20.0)
    cs = tsne_model.case(*case)
    aff = _aff(case)
    N, k, nnz = 65, 63, cs["P"].nnz
    L = _native.load("tsne")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Y = _cuda(tsne_model.pca_start(cs["P_panel"], 2))
    before = Y.clone()
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_tsne_workspace_bytes(N, 2, 0, ctypes.byref(need)), "tsne")
    ws = torch.zeros(need.value + 16, dtype=torch.uint8, device="cuda")
    f32 = lambda fill: torch.full((N, 2), fill, dtype=torch.float32, device="cuda")      # noqa: E731
    grad, y1, update, gains = f32(-7.0), f32(-7.0), f32(-7.0), f32(-7.0)
    z = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    rows = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")

    def raises(code, text):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(code, "tsne")

    for args, text in (((2, 2, 0), "N < 2"), ((1 << 31, 2, 0), "N < 2"), ((N, 1, 0), "c = 2 or 3"), ((N, 4, 0), "c = 2 or 3"),
                       ((N, 2, -1), "slabs"), ((N, 2, 1025), "slabs")):
        raises(L.prosstt_amd_tsne_workspace_bytes(*args, ctypes.byref(need)), text)
    raises(L.prosstt_amd_tsne_workspace_bytes(N, 2, 0, None), "NULL")
    # the workspace grows with the slabs
    sizes = []
    for slabs in (1, 2, 1024):
        _native.check(L.prosstt_amd_tsne_workspace_bytes(N, 3, slabs, ctypes.byref(need)), "tsne")
        sizes.append(need.value)
    assert sizes[0] < sizes[1] < sizes[2]

    def gradient(**kw):
        a = dict(N=N, nnz=nnz, c=2, y=Y, x=1.0, slabs=0, ws=_ptr(ws), bytes=ws.numel() - 16, grad=grad, z=z, indptr=aff.indptr)
        a.update(kw)
        return L.prosstt_amd_tsne_gradient(stream, _ptr(a["indptr"]), _ptr(aff.indices), _ptr(aff.data), a["N"], a["nnz"],
                                           a["c"], _ptr(a["y"]), a["x"], a["slabs"], a["ws"], a["bytes"], _ptr(a["grad"]),
                                           _ptr(a["z"]), None)

    def iterations(**kw):
        a = dict(N=N, nnz=nnz, c=2, y0=Y, y1=y1, update=update, gains=gains, begin=0, end=1, exploration=250, early=12.0,
                 eta=50.0, slabs=0, ws=_ptr(ws), bytes=ws.numel() - 16)
        a.update(kw)
        return L.prosstt_amd_tsne_iterations(stream, _ptr(aff.indptr), _ptr(aff.indices), _ptr(aff.data), a["N"], a["nnz"],
                                             a["c"], _ptr(a["y0"]), _ptr(a["y1"]), _ptr(a["update"]), _ptr(a["gains"]),
                                             a["begin"], a["end"], a["exploration"], a["early"], a["eta"], a["slabs"], a["ws"],
                                             a["bytes"])

    shared = [(dict(N=2), "N < 2"), (dict(N=1 << 31), "N < 2"), (dict(nnz=-1), "nnz"), (dict(nnz=N * N), "nnz"),
              (dict(c=1), "c = 2 or 3"), (dict(c=4), "c = 2 or 3"), (dict(slabs=-1), "slabs"), (dict(slabs=1025), "slabs"),
              (dict(ws=None), "NULL"), (dict(ws=ctypes.c_void_p(ws.data_ptr() + 8)), "16-byte aligned"),
              (dict(bytes=1024), "workspace of 1024 bytes"), (dict(slabs=64), "workspace of")]
    for kw, text in shared + [(dict(x=0.0), "exaggeration"), (dict(x=float("nan")), "exaggeration"), (dict(x=float("inf")), "exaggeration"),
                              (dict(grad=Y), "alias"), (dict(z=None), "NULL"), (dict(indptr=None), "NULL")]:
        raises(gradient(**kw), text)
    for kw, text in shared + [(dict(begin=-1), "it_begin"), (dict(begin=2, end=1), "it_begin"), (dict(exploration=-1), "exploration"),
                              (dict(early=0.0), "early_exaggeration"), (dict(eta=float("nan")), "learning_rate"),
                              (dict(eta=-1.0), "learning_rate"), (dict(y1=Y), "alias"), (dict(update=Y), "alias"),
                              (dict(gains=y1), "alias"), (dict(gains=update), "alias"), (dict(update=None), "NULL")]:
        raises(iterations(**kw), text)
    for kw, text in ((dict(N=2), "N < 2"), (dict(nnz=-1), "nnz"), (dict(c=5), "c = 2 or 3"), (dict(rows=None), "NULL")):
        a = dict(dict(N=N, nnz=nnz, c=2, rows=rows), **kw)
        raises(L.prosstt_amd_tsne_objective(stream, _ptr(aff.indptr), _ptr(aff.indices), _ptr(aff.data), a["N"], a["nnz"], a["c"],
                                            _ptr(Y), _ptr(a["rows"])), text)
    # affinities and the fold
    idx, d2 = _cuda(cs["idx"]), _cuda(cs["d2"])
    cond = torch.full((N, k), -7.0, dtype=torch.float64, device="cuda")
    beta = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for kw, text in ((dict(N=2), "N < 2"), (dict(N=1 << 31), "N < 2"), (dict(k=1), "k <= min"), (dict(k=65), "k <= min"),
                     (dict(N=5000, k=1025), "k <= min"), (dict(p=1.0), "perplexity"), (dict(p=63.0), "perplexity"),
                     (dict(p=float("nan")), "perplexity"), (dict(cond=None), "NULL")):
        a = dict(dict(N=N, k=k, p=20.0, cond=cond), **kw)
        raises(L.prosstt_amd_tsne_affinities(stream, _ptr(idx), _ptr(d2), a["N"], a["k"], a["p"], _ptr(a["cond"]), _ptr(beta),
                                             _ptr(status)), text)
    M = 2 * N * k
    keys = torch.zeros(M, dtype=torch.int64, device="cuda")
    gws = torch.zeros(2 * 8 * M + 1024, dtype=torch.uint8, device="cuda")
    indptr = torch.full((N + 1,), -7, dtype=torch.int64, device="cuda")
    indices = torch.full((M,), -7, dtype=torch.int32, device="cuda")
    data = torch.full((M,), -7.0, dtype=torch.float64, device="cuda")
    for kw, text in ((dict(N=2), "N < 2"), (dict(k=1), "k <= min"), (dict(nnz=N * k - 1), "nnz"), (dict(nnz=M + 1), "nnz"),
                     (dict(ws=None), "NULL"), (dict(ws=ctypes.c_void_p(gws.data_ptr() + 4)), "16-byte aligned"),
                     (dict(bytes=64), "workspace of 64 bytes")):
        a = dict(dict(N=N, k=k, nnz=M, ws=_ptr(gws), bytes=gws.numel()), **kw)
        raises(L.prosstt_amd_tsne_symmetrize_fold(stream, _ptr(keys), _ptr(keys), _ptr(keys), a["N"], a["k"], a["nnz"], a["ws"],
                                                  a["bytes"], _ptr(indptr), _ptr(indices), _ptr(data)), text)
    torch.cuda.synchronize()
    for t in (grad, y1, update, gains, z, rows, cond, beta, data):                       # nothing was enqueued
        assert bool((t == -7.0).all())
    assert bool((indptr == -7).all()) and bool((indices == -7).all()) and int(status.item()) == 0 and torch.equal(Y, before)
    update.zero_()
    gains.fill_(1.0)
    _native.check(gradient(), "tsne")                                # and the same calls with good arguments run
    _native.check(iterations(), "tsne")
    torch.cuda.synchronize()
    assert bool((grad != -7.0).all()) and bool((y1 != -7.0).all()) and float(z.item()) > 0 and torch.equal(Y, before)
    assert tsne.TILE == T
