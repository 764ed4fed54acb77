"""-m gpu: libprosstt_amd_factors.so writes and reads nothing outside its buffers, by the checks of
tests/test_gpu_guard_bands.py (``_guarded_runs`` with tests/guard.py: every device input a copy between two bands of 65 536
bytes of a byte, every tensor the wrapper allocates between two such bands, under each byte of ``stale.BYTES``): no band
damaged, no input written, at least one guarded allocation, equal bytes of every result under the three bytes.  The library is
a row of ``_native.NEWER_LIBRARIES``, whose libraries bring their own guard-band file; this is factors'.

The calls: the stale-memory shape of the other count-matrix libraries (259 x 1025, the shifted and the aligned view: two blocks
of cells with a ragged last one of three, whole tiles of 32 genes and a last tile of one gene, which the aligned view reads
with 4-byte loads beside the 16-byte loads of the others) with 7 coefficients, genes left out, every split, and two gene
blockings (the library's own, and one tile per block: 33 blocks, the last of one gene); and N = G = p = 1."""
import numpy as np
import pytest

import test_gpu_guard_bands as bands
import test_gpu_stale_memory as sm

pytestmark = pytest.mark.gpu


def calls_factors(place=sm._identity):
    from prosstt_amd import factors
    shifted, aligned, sc = sm._counts(place)
    rng = np.random.default_rng(259)
    L = rng.normal(0.0, 0.3, size=(1025, 7))
    coef = rng.normal(0.0, 0.3, size=(259, 7))
    alpha, beta = rng.uniform(0.0, 0.5, size=1025), rng.uniform(1.0, 3.0, size=1025)
    use = np.where(rng.random(1025) < 0.1, -1, 0)
    assert factors.gene_blocks(259, 1025)[1] > 1 and factors.gene_blocks(259, 1025, 32) == (32, 33)
    # (the drawn matrix holds counts up to 2^31 beside means near 1: every u is finite)
    calls = {}
    for name, view in (("shifted", shifted), ("aligned", aligned)):
        args = (view, sc, L, coef, alpha, beta)
        calls["own blocking, " + name] = lambda args=args: factors.cell_equations(*args)
        calls["a tile per block, genes left out, out=torch, split 8, " + name] = lambda args=args: factors.cell_equations(
            *args, use=use, out="torch", split=8, genes_per_block=32)
        calls["split 16, genes left out, " + name] = lambda args=args: factors.cell_equations(*args, use=use, split=16)
        calls["a tile per block, split 32, " + name] = lambda args=args: factors.cell_equations(*args, split=32, genes_per_block=32)
    return "factors.cell_equations", calls


def small_factors(place):
    from prosstt_amd import factors
    aligned, shifted = bands._one_by_one(place)
    args = (np.array([1.5]), np.array([[1.0]]), np.array([[0.3]]), 0.2, 2.0)
    return "factors, N = G = p = 1", {
        "aligned": lambda: factors.cell_equations(aligned, *args),
        "shifted, out=torch": lambda: factors.cell_equations(shifted, *args, out="torch"),
        "shifted, split 32, a tile per block": lambda: factors.cell_equations(shifted, *args, split=32, genes_per_block=32)}


def test_the_library_is_in_the_table_whose_rows_bring_their_own_file():
    from prosstt_amd import _native
    assert "factors" in _native.NEWER_LIBRARIES and "factors" not in bands.LIBRARIES


def test_no_access_outside_a_buffer():
    bands._guarded_runs("factors", calls_factors, "the stale-memory shapes")
    bands._guarded_runs("factors", small_factors, "the smallest problem")
