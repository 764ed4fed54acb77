"""-m gpu: libprosstt_amd_evaluate.so writes and reads nothing outside its buffers, by the checks of
tests/test_gpu_guard_bands.py (``_guarded_runs`` with tests/guard.py: every device input a copy between two bands of 65 536
bytes of a byte, every tensor the wrapper allocates between two such bands, under each byte of ``stale.BYTES``): no band
damaged, no input written, at least one guarded allocation, equal bytes of every result under the three bytes.  The library is
a row of ``_native.NEWER_LIBRARIES``, whose libraries bring their own guard-band file; this is evaluate's.

The calls: the 259 cells of the other libraries' stale-memory shape (one tile of 256 columns and three more: a ragged tile, a
ragged row block) in five classes of which one is empty, the counts and the moments at the library's tiles_per_block, at 1 and
at the cap; and N = 2, K = 1."""
import numpy as np
import pytest

import test_gpu_guard_bands as bands
import test_gpu_stale_memory as sm

pytestmark = pytest.mark.gpu

MAX_DEPTH = 65535


def _inputs(N, K, K2):
    rng = np.random.default_rng(N)
    classes = rng.integers(0, K, N)
    classes[classes == 1] = 0                                     # (class 1 is empty where there are several)
    a, b = rng.integers(0, 9, N), rng.permutation(N)
    h, h2 = rng.integers(0, MAX_DEPTH + 1, N), rng.integers(0, MAX_DEPTH + 1, N)
    c2 = rng.integers(0, K2, N)
    J = np.full((K, K), 1000, dtype=np.int32)
    J[np.diag_indices(K)] = MAX_DEPTH
    J2 = np.full((K2, K2), 77, dtype=np.int32)
    J2[np.diag_indices(K2)] = MAX_DEPTH
    return classes, a, b, h, h2, c2, J, J2


def _calls(place, N, K, K2):
    from prosstt_amd import evaluate
    classes, a, b, h, h2, c2, J, J2 = _inputs(N, K, K2)
    dc, da, db, dh, dh2, dc2 = (place(sm._cuda(v)) for v in (classes, a, b, h, h2, c2))
    calls = {}
    for tiles in (0, 1, 4096):
        calls["counts, tiles_per_block %d" % tiles] = lambda tiles=tiles: evaluate.pair_counts(da, db, dc, K, tiles_per_block=tiles)
        calls["moments, out=torch, tiles_per_block %d" % tiles] = lambda tiles=tiles: evaluate.tree_moments(
            dh, dc, J, dh2, dc2, J2, tiles_per_block=tiles, out="torch").words
    calls["counts, host arrays, out=torch"] = lambda: evaluate.pair_counts(a, b, classes, K, out="torch")
    calls["moments, host arrays"] = lambda: evaluate.tree_moments(h, classes, J, h2, c2, J2).words
    return calls


def calls_evaluate(place=sm._identity):
    return "evaluate, 259 cells in five classes", _calls(place, 259, 5, 64)


def small_evaluate(place):
    return "evaluate, N = 2, K = 1", _calls(place, 2, 1, 1)


def test_the_library_is_in_the_table_whose_rows_bring_their_own_file():
    from prosstt_amd import _native
    assert "evaluate" in _native.NEWER_LIBRARIES and "evaluate" not in bands.LIBRARIES


def test_no_access_outside_a_buffer():
    bands._guarded_runs("evaluate", calls_evaluate, "259 cells")
    bands._guarded_runs("evaluate", small_evaluate, "the smallest problem")
