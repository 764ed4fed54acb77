"""prosstt_amd/thin.py without a device: the grid rounding of ``split``, ``fold``'s intervals, ``downsample``'s fractions, ``Split.sizes``,
every refusal (each comes before any device use), the header's constants, and that each case of tests/test_gpu_thin.py reaches
the path it is there for (the aligned or the plain instantiation, the ragged strip, more than one row block), by the library's
own plan."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import thin_cases as C
import thin_model as T

torch = pytest.importorskip("torch")

from prosstt_amd import _native, thin  # noqa: E402


def _cpu(N=3, G=4):
    return torch.ones((N, G), dtype=torch.int32)


def test_the_constants_are_the_headers_and_the_models():
    header = open(os.path.join(ROOT, "include", "prosstt_amd_thin.h")).read()
    value = {name: int(v.rstrip("u")) for name, v in re.findall(r"#define PROSSTT_AMD_THIN_(\w+) (\d+u?)", header)}
    assert value == {"GRID": thin.GRID, "MAX_COUNT": thin.MAX_COUNT, "NEGATIVE": thin.NEGATIVE, "OVER": thin.OVER,
                     "RANGE": thin.RANGE}
    assert (thin.GRID, thin.MAX_COUNT) == (T.GRID, T.MAX_COUNT) == (65536, 1 << 24)
    source = open(os.path.join(ROOT, "prosstt_amd", "csrc", "thin", "thin.hip")).read()
    for name, constant in (("kCellSalt", T.CELL_SALT), ("kGeneSalt", T.GENE_SALT), ("kGolden", T.GOLDEN)):
        assert re.search(r"%s = 0x%Xull" % (name, int(constant)), source), name
    assert "0x%Xull" % int(T.M1) in source and "0x%Xull" % int(T.M2) in source
    for constant in (T.CELL_SALT, T.GENE_SALT, T.GOLDEN, T.M1, T.M2):
        assert "0x%X" % int(constant) in header
    assert "thin" in _native.NEWER_LIBRARIES


def test_split_rounds_to_the_grid():
    assert thin._fraction_to_grid(0.5) == 32768 and thin._fraction_to_grid(0.25) == 16384 and thin._fraction_to_grid(3 / 16) == 12288
    assert thin._fraction_to_grid(1e-9) == 1 and thin._fraction_to_grid(1 - 1e-9) == 65535
    assert thin._fraction_to_grid(0.1) == round(0.1 * 65536) == 6554
    for bad in (0, 1, 0.0, 1.0, -0.2, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 < fraction < 1"):
            thin._fraction_to_grid(bad)
    for bad in ("half", None, True, [0.5]):
        with pytest.raises(TypeError, match="fraction is a number"):
            thin._fraction_to_grid(bad)
    s = thin.Split("train", "test", 6554 / 65536)
    a, b = s.sizes(np.array([1.0, 2.0]))
    assert np.array_equal(a, s.fraction * np.array([1.0, 2.0])) and np.array_equal(b, (1.0 - s.fraction) * np.array([1.0, 2.0]))
    assert np.allclose(a + b, [1.0, 2.0], rtol=1e-15)


@pytest.mark.parametrize("K", range(2, 65))
def test_the_folds_tile_the_grid(K):
    pieces = [thin.fold_interval(K, f) for f in range(K)]
    assert pieces[0][0] == 0 and pieces[-1][1] == thin.GRID
    assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:])) and all(lo < hi for lo, hi in pieces)
    assert max(hi - lo for lo, hi in pieces) - min(hi - lo for lo, hi in pieces) <= 1


def test_fold_refusals():
    for K in (1, 65, 0, -3, 2.0, True, None):
        with pytest.raises(ValueError, match="2 <= K <= 64"):
            thin.fold_interval(K, 0)
    for f in (-1, 5, 1.0, None, False):
        with pytest.raises(ValueError, match="0 <= fold < 5"):
            thin.fold_interval(5, f)
    with pytest.raises(ValueError, match="2 <= K <= 64"):
        thin.fold(_cpu(), 70, 0)


def test_downsample_fractions():
    totals = np.array([0, 1, 999, 1000, 1001, 2000, 3000, 10 ** 9, 2 ** 40])
    k = thin.downsample_grid(totals, 1000)
    assert k.dtype == np.uint32
    assert k.tolist() == [65536, 65536, 65536, 65536, 65536 * 1000 // 1001, 32768, 65536 * 1000 // 3000, 0, 0]
    # floored: p never exceeds total / total_i, and is within one grid step of it
    for t, g in zip(totals.tolist(), k.tolist()):
        if t > 1000:
            assert g / 65536 <= 1000 / t < (g + 1) / 65536
    assert thin.downsample_grid(np.array([5, 7]), 0).tolist() == [0, 0]
    with pytest.raises(TypeError, match="integer array"):
        thin.downsample_grid(np.array([1.5]), 10)
    with pytest.raises(ValueError, match="negative"):
        thin.downsample_grid(np.array([-1]), 10)
    with pytest.raises(ValueError, match="total must be an integer >= 0"):
        thin.downsample_grid(np.array([1]), -10)
    with pytest.raises(ValueError, match="exactly one of total and fraction"):
        thin.downsample(_cpu())
    with pytest.raises(ValueError, match="exactly one of total and fraction"):
        thin.downsample(_cpu(), total=5, fraction=0.5)
    with pytest.raises(ValueError, match="0 <= fraction <= 1"):
        thin.downsample(_cpu(), fraction=1.5)
    with pytest.raises(ValueError, match="one number or one per cell"):
        thin.downsample(_cpu(), fraction=[0.5, 0.5])
    with pytest.raises(ValueError, match="totals needs one entry per cell"):
        thin.downsample(_cpu(), total=5, totals=[1, 2])
    with pytest.raises(ValueError, match="total must be an integer"):
        thin.downsample(_cpu(), total=2.5)
    with pytest.raises(ValueError, match="needs a device tensor"):        # everything else was in order
        thin.downsample(_cpu(), fraction=np.array([0.5, 0.25, 1.0]))
    with pytest.raises(ValueError, match="needs a device tensor"):
        thin.downsample(_cpu(), total=5, totals=[1, 2, 30])


def test_interval_refusals():
    X = _cpu()
    with pytest.raises(TypeError, match="host arrays are refused"):
        thin.interval(np.ones((3, 4), dtype=np.int32), 0, 1)
    with pytest.raises(TypeError, match="needs int32 counts"):
        thin.interval(X.to(torch.int64), 0, 1)
    with pytest.raises(ValueError, match="not 1 dimensions"):
        thin.interval(X[0], 0, 1)
    with pytest.raises(ValueError, match="at least one cell and one gene"):
        thin.interval(X[:0], 0, 1)
    with pytest.raises(ValueError, match="needs a device tensor"):
        thin.interval(X, 0, 1)
    with pytest.raises(ValueError, match="needs a device tensor"):
        thin.split(X)
    for lo, hi in ((2, 1), (65536, 0), (np.array([0, 5, 0]), 4), (3, np.array([5, 2, 9]))):
        with pytest.raises(ValueError, match="need lo <= hi"):
            thin.interval(X, lo, hi)
    for lo, hi in ((-1, 5), (0, 65537), (np.array([0, 0, -2]), 5), (0, np.array([1, 2, 70000]))):
        with pytest.raises(ValueError, match="on the grid"):
            thin.interval(X, lo, hi)
    for lo, hi in ((0.0, 5), (0, 0.5), (True, 5), (None, 5), (0, np.array([0.5, 0.5, 0.5])), (0, "all")):
        with pytest.raises(TypeError, match="grid integer"):
            thin.interval(X, lo, hi)
    for lo, hi in ((np.array([0, 0]), 5), (0, np.array([1, 2, 3, 4])), (0, np.zeros((3, 1), dtype=np.int64))):
        with pytest.raises(ValueError, match="one entry per cell"):
            thin.interval(X, lo, hi)
    for seed in (-1, 1 << 64, 0.5, None, True):
        with pytest.raises(ValueError, match="seed must be an integer"):
            thin.interval(X, 0, 1, seed=seed)
    for name in ("cell_offset", "gene_offset"):
        for value in (-1, 1.0, None, 1 << 62):
            with pytest.raises(ValueError, match=name):
                thin.interval(X, 0, 1, **{name: value})
    with pytest.raises(TypeError, match="takes a factors.Factors"):
        thin.heldout("fit", X, np.ones(3))
    with pytest.raises(ValueError, match="at least one k"):
        thin.rank_curve(X, np.ones(3), (), alpha=0.0, beta=1.0)
    with pytest.raises(ValueError, match="0 < fraction < 1"):
        thin.rank_curve(X, np.ones(3), (1,), alpha=0.0, beta=1.0, fraction=1.0)


def test_a_non_unit_column_stride_is_refused_on_the_host():
    class OnDevice:
        """What CountMatrix.on_device looks at, without a device."""
        def __init__(self, strides):
            self._strides, self.device = strides, type("D", (), {"type": "cuda"})()

        def stride(self, i):
            return self._strides[i]

    from prosstt_amd import device
    m = device.CountMatrix(_cpu(), "thin.interval")
    m.X = OnDevice((8, 2))
    with pytest.raises(ValueError, match="unit column stride"):
        m.on_device()
    m.X = OnDevice((3, 1))
    with pytest.raises(ValueError, match="rows overlap"):
        m.on_device()


def test_status_messages_name_the_entrys_kind():
    from prosstt_amd import device
    thin.check_status(0)
    with pytest.raises(ValueError, match="negative entry") as e:
        thin.check_status(thin.NEGATIVE | thin.OVER)
    assert str(e.value) == device.NEGATIVE_ENTRY
    with pytest.raises(ValueError, match=r"above 2\^24"):
        thin.check_status(thin.OVER)
    with pytest.raises(RuntimeError, match="lo / hi tables"):
        thin.check_status(thin.RANGE)


def _lib():
    if not os.path.exists(_native.NEWER_LIBRARIES["thin"].path):
        pytest.skip("libprosstt_amd_thin.so is not built")
    return _native.load("thin")


@pytest.mark.parametrize("case", list(C.CASES), ids=lambda c: "%dx%d-%s" % c)
def test_every_device_case_reaches_its_path(case):
    _lib()
    N, G, view = case
    vec, strips, last, blocks = C.CASES[case]
    off, ld = C.layout(N, G, view)
    base = 1 << 20
    for r_ptr in (0, 3 << 20):                                   # without and with the complement
        got = thin.plan(N, G, base + off, ld, 2 << 20, G, r_ptr, G if r_ptr else 0)
        assert got[0] is vec and got[1] == strips and G - 1024 * (strips - 1) == last
        assert (got[2] > 1) is blocks and got[2] * got[3] >= N > (got[2] - 1) * got[3]
    # an output whose rows do not start on 16 bytes takes the plain instantiation whatever the input
    assert thin.plan(N, G, base, ld, (2 << 20) + 4, G)[0] is False
    # the tables and the drawn counts are what the cases say
    X = C.counts(N, G)
    assert X.dtype == np.int32 and X.min() >= 0 and X.max() <= 4096
    if N * G >= 7:
        assert set(C.PLANTED) <= set(X.ravel().tolist())
    if N * G > 1000:
        assert 0.55 < (X == 0).mean() < 0.65
    lo, hi = C.tables(N)
    assert lo.shape == hi.shape == (N,) and np.all(lo <= hi)
    if N >= 13:
        rows = got[3]                                            # one row block holds every scalar interval
        assert set(C.SCALAR_INTERVALS) <= set(zip(lo[:rows].tolist(), hi[:rows].tolist()))


def test_the_abi_refuses_its_arguments_without_a_device():
    import ctypes
    L = _lib()
    vp = ctypes.c_void_p
    base = 1 << 20

    def call(X=base, N=4, G=8, ld=8, lo=0, hi=5, Y=2 << 20, ldy=8, R=None, ldr=0, status=3 << 20, co=0, go=0):
        rc = L.prosstt_amd_thin_interval(None, vp(X), N, G, ld, 7, None, co, go, lo, hi, None, None, vp(Y), ldy,
                                         vp(R) if R else None, ldr, vp(status))
        return rc, L.prosstt_amd_thin_last_error().decode()

    for kw, text in ((dict(N=0), "need 1 <= N"), (dict(N=1 << 31), "need 1 <= N"), (dict(G=0), "G >= 1"),
                     (dict(ld=7), "row stride 7 is below the row length 8"), (dict(ldy=7), "row stride 7 is below"),
                     (dict(R=4 << 20, ldr=7), "row stride 7 is below"), (dict(X=0), "NULL"), (dict(Y=0), "NULL"),
                     (dict(status=0), "NULL"), (dict(co=-1), "cell_offset and gene_offset"), (dict(go=-1), "cell_offset and gene_offset"),
                     (dict(lo=6, hi=5), "need 0 <= lo <= hi <= 65536"), (dict(hi=65537), "need 0 <= lo <= hi <= 65536"),
                     (dict(Y=base), "overlaps the input"), (dict(Y=base + 4 * 31), "overlaps the input"),
                     (dict(Y=base - 4 * 31), "overlaps the input"), (dict(R=base + 64, ldr=8), "overlaps the input"),
                     (dict(R=(2 << 20) + 32, ldr=8), "the two outputs overlap")):
        rc, message = call(**kw)
        assert rc == -1 and text in message, (kw, rc, message)
