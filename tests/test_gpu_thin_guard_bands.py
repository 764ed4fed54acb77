"""-m gpu: libprosstt_amd_thin.so writes and reads nothing outside its buffers, by the checks of
tests/test_gpu_guard_bands.py (``_guarded_runs`` with tests/guard.py: every device input a copy between two bands of 65 536
bytes of a byte, every tensor the wrapper allocates between two such bands, under each byte of ``stale.BYTES``): no band
damaged, no input written, at least one guarded allocation, equal bytes of every result under the three bytes.  The library is
a row of ``_native.NEWER_LIBRARIES``, whose libraries bring their own guard-band file; this is thin's.

The calls: tests/thin_cases.py's 259 x 1025 in the shifted and the aligned view (five blocks of rows with a ragged last one, a
whole strip of 1024 genes and a last strip of one gene) with and without the complement and with per-cell tables, 5 x 1028 (the
aligned instantiation's 16-byte stores beside a ragged strip of four genes), and N = G = 1."""
import numpy as np
import pytest

import test_gpu_guard_bands as bands
import test_gpu_stale_memory as sm
import thin_cases as C

pytestmark = pytest.mark.gpu


def _placed(place, N, G, view):
    import torch
    host = torch.as_tensor(C.counts(N, G)).cuda()
    if view == "aligned":
        return place(host)
    off, ld = C.layout(N, G, view)
    wide = torch.full((N, ld), 12345, dtype=torch.int32, device="cuda")
    wide[:, 1:1 + G] = host
    return place(wide[:, 1:1 + G])


def calls_thin(place=sm._identity):
    from prosstt_amd import thin
    lo, hi = C.tables(259)
    calls = {}
    for view in ("shifted", "aligned"):
        X = _placed(place, 259, 1025, view)
        calls["[0, 32768), " + view] = lambda X=X: thin.interval(X, 0, 32768)
        calls["[1, 65536) with the complement, " + view] = lambda X=X: thin.interval(X, 1, 65536, complement=True)
        calls["per-cell tables, " + view] = lambda X=X: thin.interval(X, lo, hi)
        calls["per-cell tables with the complement, " + view] = lambda X=X: thin.interval(X, lo, hi, complement=True)
    wide = _placed(place, 5, 1028, "aligned")
    calls["5 x 1028 with the complement"] = lambda: thin.interval(wide, 777, 30001, complement=True)
    return "thin.interval", calls


def small_thin(place):
    from prosstt_amd import thin
    aligned, shifted = bands._one_by_one(place)
    return "thin, N = G = 1", {
        "aligned": lambda: thin.interval(aligned, 0, 32768),
        "shifted, with the complement": lambda: thin.interval(shifted, 1, 65536, complement=True),
        "shifted, per-cell tables": lambda: thin.interval(shifted, np.array([5]), np.array([40000]), complement=True)}


def test_the_library_is_in_the_table_whose_rows_bring_their_own_file():
    from prosstt_amd import _native
    assert "thin" in _native.NEWER_LIBRARIES and "thin" not in bands.LIBRARIES


def test_no_access_outside_a_buffer():
    bands._guarded_runs("thin", calls_thin, "the stale-memory shapes")
    bands._guarded_runs("thin", small_thin, "the smallest problem")
