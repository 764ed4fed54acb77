"""-m gpu: prosstt_amd.dpt (libprosstt_amd_dpt.so) against the numpy model of tests/dpt_model.py: the distance rows within one
unit in the last place, the concordance sums bit for bit on every slab count and both batch sizes, the whole call with one
branching stage by stage (each stage of the model is fed the device's output of the stage before), repeats and a second
stream, refusals through the ABI.

The bound of the rows.  The sum under the root is the same sequence of correctly rounded binary64 operations on the device
and in numpy (nothing is fused: -ffp-contract=off), so only the square root may differ: |d - model| <= 1 ulp of the model's
value.  On an MI355X every value was equal to the bit.

The sizes of the concordance cases: 3 is the smallest N; 255, 256, 257 lie on both sides of a tile edge (256 columns); 511,
512, 513 on both sides of a row-block edge (512 rows); 1000 takes two row blocks and four tiles, so that a block sees tiles
wholly below it, tiles that meet its rows, and (the first block) tiles wholly above it."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.stats

import dpt_model
import graph_model

pytestmark = pytest.mark.gpu

TABLE, SLACK = dpt_model.TABLE, dpt_model.SLACK
SLABS = (1, 2, 3, 0)
SIZES = (3, 255, 256, 257, 511, 512, 513, 1000)
KINDS = ("permutations", "four values", "all equal", "identical", "reversed")


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()               # (a copy: the shared model arrays are read-only)


# ---------------------------------------------------------------------------------------------------------------- rows

def _random_map(N, n_comps):
    from prosstt_amd.graph import DiffusionMap
    rng = np.random.default_rng(N + n_comps)
    vectors = rng.standard_normal((N, n_comps)) / np.sqrt(N)
    vectors[:, 0] = 1.0 / np.sqrt(N)                               # the trivial component: differences of exactly 0
    values = np.linspace(1.0, 0.3, n_comps)
    values[1:3] = (0.9997, 0.9993)[:len(values[1:3])]              # one weight of 1 beyond the first, one large weight
    return DiffusionMap(values, vectors, n_comps, np.zeros(n_comps), None)


@pytest.mark.parametrize("N,n_comps", [(3, 2), (65, 15), (1000, 15)])
@pytest.mark.parametrize("sources", [1, 4])
def test_rows_against_the_model(N, n_comps, sources):
    from prosstt_amd import dpt
    dm = _random_map(N, n_comps)
    src = [N - 1] if sources == 1 else [0, N // 2, N - 1, N // 2]
    for n_dcs in sorted({1, min(10, n_comps), n_comps}):
        want = dpt_model.rows(dm.eigenvectors, dpt_model.weights(dm.eigenvalues, n_dcs), src)
        got = dpt.distances(dm, src, n_dcs)
        on_device = dpt.distances(dm._replace(eigenvalues=_cuda(dm.eigenvalues), eigenvectors=_cuda(dm.eigenvectors)), src, n_dcs,
                                  out="torch")
        assert got.shape == (len(src), N) and got.dtype == np.float64
        assert np.array_equal(got, on_device.cpu().numpy())
        ulps = dpt_model.ulp_distance(got, want)
        print("(%d, %d), %d sources, n_dcs %d: largest error %.3g ulp, %d of %d values differ in a bit"
              % (N, n_comps, len(src), n_dcs, ulps.max(), int((got != want).sum()), got.size))
        assert np.all(ulps <= 1.0)
        assert np.all(got[np.arange(len(src)), src] == 0)
    default = dpt.distances(dm, src)
    assert np.array_equal(default, dpt.distances(dm, src, min(10, n_comps)))


# --------------------------------------------------------------------------------------------------------- concordance

@functools.lru_cache(maxsize=None)
def _sequences(N, batch):
    """{kind: (ru, rv, the model's lower, the model's upper)} for int32 (batch, N) sequences; read-only."""
    rng = np.random.default_rng(1000 * N + batch)
    base = np.tile(np.arange(N, dtype=np.int32), (batch, 1))
    perm = [np.stack([rng.permutation(N) for _ in range(batch)]).astype(np.int32) for _ in range(3)]
    pairs = {
        "permutations": (perm[0], perm[1]),
        # (ranks lie in [0, N): three values at N = 3)
        "four values": tuple(rng.integers(0, min(4, N), (batch, N)).astype(np.int32) for _ in range(2)),
        "all equal": (np.zeros((batch, N), dtype=np.int32), perm[2]),
        "identical": (perm[2], perm[2]),
        "reversed": (base, base[:, ::-1].copy()),
    }
    out = {}
    for kind, (ru, rv) in pairs.items():
        out[kind] = (ru, rv) + dpt_model.concordance(ru, rv)
        for arr in out[kind]:
            arr.setflags(write=False)
    return out


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("slabs", SLABS)
@pytest.mark.parametrize("N", SIZES)
def test_concordance_bit_for_bit(N, slabs, batch):
    from prosstt_amd import dpt
    for kind in KINDS:
        ru, rv, lower, upper = _sequences(N, batch)[kind]
        got_lower, got_upper = dpt.concordance(_cuda(ru), _cuda(rv), slabs)
        assert got_lower.dtype == got_upper.dtype and str(got_lower.dtype) == "torch.int64"
        assert np.array_equal(got_lower.cpu().numpy(), lower), kind
        assert np.array_equal(got_upper.cpu().numpy(), upper), kind
    # the closed forms the model was checked against
    r = np.arange(N)
    ru, rv, lower, upper = _sequences(N, batch)["reversed"]
    assert np.array_equal(lower, np.tile(-r, (batch, 1))) and np.array_equal(upper, np.tile(r + 1 - N, (batch, 1)))
    ru, rv, lower, upper = _sequences(N, batch)["identical"]
    assert np.array_equal(lower, np.tile(r, (batch, 1))) and np.array_equal(upper, np.tile(N - 1 - r, (batch, 1)))
    assert not _sequences(N, batch)["all equal"][2].any() and not _sequences(N, batch)["all equal"][3].any()


def test_concordance_of_identical_sorted_sequences_and_host_arrays():
    from prosstt_amd import dpt
    N = 700
    r = np.arange(N, dtype=np.int32)[None]
    lower, upper = dpt.concordance(r, r)                           # host arrays in, host arrays out
    assert isinstance(lower, np.ndarray) and lower.dtype == np.int64
    assert np.array_equal(lower[0], np.arange(N)) and np.array_equal(upper[0], N - 1 - np.arange(N))
    bad = _cuda(r)
    bad[0, 5] = N
    with pytest.raises(ValueError, match="outside"):
        dpt.concordance(bad, _cuda(r))


# ------------------------------------------------------------------------------------------------------ the whole call

@functools.lru_cache(maxsize=None)
def _device_run(N, k):
    """(the device's diffusion map of its own neighbours, the DPT result, its stages as host arrays) of graph_model.case(N, k)."""
    import torch
    from prosstt_amd import dpt, graph, neighbors
    nb = neighbors.knn(_cuda(graph_model.case(N, k)["P"]), k, out="torch")
    dm = graph.diffmap(nb, out="torch")
    root = dpt_model.truth(N, k)[2]
    res, stages = dpt.dpt(dm, root, n_branchings=1, _stages=True)
    torch.cuda.synchronize()
    return dm, res, {name: t.cpu().numpy() for name, t in stages.items()}


def _check_stages(res, st, values, vectors, root, n_dcs, m):
    """Every stage of the device's result against the model fed with the device's output of the stage before."""
    N = vectors.shape[0]
    assert res.pseudotime.dtype == np.float64 and res.pseudotime.shape == (N,)
    assert res.groups.dtype == np.int8 and res.groups.shape == (N,)
    assert res.tips == tuple(int(t) for t in st["tips"]) and res.splits == tuple(int(s) for s in st["splits"])
    # rows: the model from the device's eigenvectors
    want = dpt_model.rows(vectors, dpt_model.weights(values, n_dcs), [root] + list(res.tips))
    got = np.concatenate([st["root_row"][None], st["rows"]])
    ulps = dpt_model.ulp_distance(got, want)
    print("N %d, n_dcs %d: rows: largest error %.3g ulp, %d of %d values differ in a bit"
          % (N, n_dcs, ulps.max(), int((got != want).sum()), got.size))
    assert np.all(ulps <= 1.0)
    assert np.array_equal(res.pseudotime, st["root_row"] / st["root_row"].max())
    # tips: the model's argmax of the device's rows
    D = st["rows"]
    assert res.tips == (int(np.argmax(st["root_row"])), int(np.argmax(D[0])), int(np.argmax(D[0] + D[1])))
    # ranks from the device's rows, sums from the device's ranks, splits from the device's sums, groups from its splits
    order, ru, rv = dpt_model.ranks(D)
    assert np.array_equal(st["order"], order)
    assert st["ru"].dtype == np.int32 and np.array_equal(st["ru"], ru) and np.array_equal(st["rv"], rv)
    lower, upper = dpt_model.concordance(st["ru"], st["rv"])
    assert st["lower"].dtype == np.int64 and np.array_equal(st["lower"], lower) and np.array_equal(st["upper"], upper)
    assert res.splits == dpt_model.splits(st["lower"], st["upper"], m)
    assert np.array_equal(res.groups, dpt_model.groups(st["order"], res.splits))


@pytest.mark.parametrize("N,k", [(300, 5), (1000, 14)])
def test_the_whole_call_stage_by_stage(N, k):
    dm, res, st = _device_run(N, k)
    arm, pos, root, time = dpt_model.truth(N, k)
    _check_stages(res, st, dm.eigenvalues.cpu().numpy(), dm.eigenvectors.cpu().numpy(), root, 10, 5)
    # the structure the model shows on the CPU
    tip_arms, sizes, share, agreement = dpt_model.structure(dict(tips=res.tips, groups=res.groups), arm)
    tau = scipy.stats.kendalltau(res.pseudotime, time).statistic
    print("(%d, %d): tips %s in arms %s, groups %s, splits %s, share %.4f, agreement %.4f, tau %.4f"
          % (N, k, res.tips, tip_arms, sizes, res.splits, share, agreement, tau))
    assert sorted(tip_arms) == [0, 1, 2] and min(sizes) > 0
    assert share >= TABLE[N, k][0] - SLACK and agreement >= TABLE[N, k][1] - SLACK and tau >= TABLE[N, k][2] - SLACK


def test_without_a_branching_and_with_other_arguments():
    from prosstt_amd import dpt
    dm, res, st = _device_run(300, 5)
    root = dpt_model.truth(300, 5)[2]
    plain = dpt.dpt(dm, root)
    assert plain.groups is None and plain.tips is None and plain.splits is None
    assert np.array_equal(plain.pseudotime, res.pseudotime)
    # host arrays in, device tensors out, every component, a larger smallest group, two slabs
    values, vectors = dm.eigenvalues.cpu().numpy(), dm.eigenvectors.cpu().numpy()
    other, stages = dpt.dpt(dm._replace(eigenvalues=values, eigenvectors=vectors), root, 15, n_branchings=1, min_group_size=40,
                            slabs=2, out="torch", _stages=True)
    assert str(other.pseudotime.dtype) == "torch.float64" and str(other.groups.dtype) == "torch.int8"
    assert other.pseudotime.is_cuda and other.groups.is_cuda
    other = other._replace(pseudotime=other.pseudotime.cpu().numpy(), groups=other.groups.cpu().numpy())
    _check_stages(other, {name: t.cpu().numpy() for name, t in stages.items()}, values, vectors, root, 15, 40)
    assert min(other.splits) >= 40 and max(other.splits) <= 260


def test_equal_calls_give_equal_bits_on_any_stream():
    import torch
    from prosstt_amd import dpt
    dm, res, st = _device_run(1000, 14)
    root = dpt_model.truth(1000, 14)[2]
    again, st2 = dpt.dpt(dm, root, n_branchings=1, _stages=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third, st3 = dpt.dpt(dm, root, n_branchings=1, slabs=3, _stages=True)
    side.synchronize()
    for other, stages in ((again, st2), (third, st3)):
        assert np.array_equal(other.pseudotime.view(np.int64), res.pseudotime.view(np.int64))
        assert np.array_equal(other.groups, res.groups) and other.tips == res.tips and other.splits == res.splits
        for name in ("rows", "lower", "upper", "ru", "rv"):
            assert np.array_equal(stages[name].cpu().numpy(), st[name]), name


# ---------------------------------------------------------------------------------------------------------------- ABI

def test_the_abi_refuses():
    import torch
    from prosstt_amd import _native
    L = _native.load("dpt")
    need = ctypes.c_uint64(0)
    assert L.prosstt_amd_dpt_workspace_bytes(1000, 3, 2, ctypes.byref(need)) == 0
    assert need.value >= 3 * 2 * 2 * 1000 * 4
    for args in ((2, 1, 0), (1 << 31, 1, 0), (1000, 0, 0), (1000, 1025, 0), (1000, 1, -1), (1000, 1, 1025)):
        assert L.prosstt_amd_dpt_workspace_bytes(*args, ctypes.byref(need)) == _native.EINVAL, args
    assert L.prosstt_amd_dpt_workspace_bytes(1000, 1, 0, None) == _native.EINVAL
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    q = ctypes.c_void_p(buf.data_ptr() + (1 << 15))
    ok = (None, p, p, 1000, 1, 1, p, 1 << 15, q, ctypes.c_void_p(q.value + 8000))
    for at, value in ((1, None), (2, None), (6, None), (8, None), (9, None), (3, 2), (3, 1 << 31), (4, 0), (5, -1),
                      (6, ctypes.c_void_p(p.value + 8)), (7, 100), (9, q)):
        args = list(ok)
        args[at] = value
        assert L.prosstt_amd_dpt_concordance(*args) == _native.EINVAL, (at, value)
        assert L.prosstt_amd_dpt_last_error()
    ok = (None, p, 4, p, 1000, 4, p, 1, q)
    for at, value in ((1, None), (3, None), (6, None), (8, None), (4, 2), (4, 1 << 31), (5, 0), (5, 1000), (2, 3), (7, 0),
                      (7, 65536), (8, p)):
        args = list(ok)
        args[at] = value
        assert L.prosstt_amd_dpt_rows(*args) == _native.EINVAL, (at, value)
    with pytest.raises(_native.NativeError, match="N"):
        _native.check(L.prosstt_amd_dpt_workspace_bytes(2, 1, 0, ctypes.byref(need)), "dpt")
    torch.cuda.synchronize()
