"""-m gpu: libprosstt_amd_regress.so writes and reads nothing outside its buffers, by the checks of
tests/test_gpu_guard_bands.py (``_guarded_runs`` with tests/guard.py: every device input a copy between two bands of 65 536
bytes of a byte, every tensor the wrapper allocates between two such bands, under each byte of ``stale.BYTES``): no band
damaged, no input written, at least one guarded allocation, equal bytes of every result under the three bytes.  The library is
a row of ``_native.NEWER_LIBRARIES``, whose libraries bring their own guard-band file; this is regress's.

The calls: the stale-memory shape of the other count-matrix libraries (259 x 1025, the shifted and the aligned view: five
blocks of rows with a ragged last one, four whole strips of 256 genes and one gene more) with 60 design rows and 7
coefficients, the information and the meat, every split; and N = G = K = p = 1."""
import numpy as np
import pytest

import test_gpu_guard_bands as bands
import test_gpu_stale_memory as sm

pytestmark = pytest.mark.gpu


def calls_regress(place=sm._identity):
    from prosstt_amd import regress
    shifted, aligned, sc = sm._counts(place)
    rng = np.random.default_rng(259)
    labels = rng.integers(-1, 60, size=259)
    D = rng.dirichlet(np.ones(7), size=60)
    coef = rng.normal(0.0, 0.3, size=(1025, 7))
    alpha, beta = rng.uniform(0.0, 0.5, size=1025), rng.uniform(1.0, 3.0, size=1025)
    # (the drawn matrix holds counts up to 2^31 beside means near 1: every u and u^2 is finite)
    calls = {}
    for name, view in (("shifted", shifted), ("aligned", aligned)):
        args = (view, sc, labels, D, coef, alpha, beta)
        calls["information, " + name] = lambda args=args: regress.normal_equations(*args)
        calls["meat, out=torch, split 8, " + name] = lambda args=args: regress.normal_equations(*args, meat=True, out="torch", split=8)
        calls["information, split 32, " + name] = lambda args=args: regress.normal_equations(*args, split=32)
    return "regress.normal_equations", calls


def small_regress(place):
    from prosstt_amd import regress
    aligned, shifted = bands._one_by_one(place)
    args = (np.array([1.5]), np.array([0]), np.array([[1.0]]), np.array([[0.3]]), 0.2, 2.0)
    return "regress, N = G = K = p = 1", {
        "information, aligned": lambda: regress.normal_equations(aligned, *args),
        "meat, shifted, out=torch": lambda: regress.normal_equations(shifted, *args, meat=True, out="torch"),
        "information, shifted, split 32": lambda: regress.normal_equations(shifted, *args, split=32)}


def test_the_library_is_in_the_table_whose_rows_bring_their_own_file():
    from prosstt_amd import _native
    assert "regress" in _native.NEWER_LIBRARIES and "regress" not in bands.LIBRARIES


def test_no_access_outside_a_buffer():
    bands._guarded_runs("regress", calls_regress, "the stale-memory shapes")
    bands._guarded_runs("regress", small_regress, "the smallest problem")
