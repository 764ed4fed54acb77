"""The cases that tests/test_gpu_thin.py runs on the device, and what tests/test_thin_host.py checks of them without one: the
shapes and views, the path each is there for, the drawn matrices, the intervals and the per-cell tables.  A helper: nothing
here is collected.

A view is "aligned" (a contiguous tensor: base on 16 bytes, row stride G) or "shifted" (one column into a wider tensor: base 4
bytes past 16, an odd row stride).  The outputs are new contiguous tensors with the row stride G, so rows go in 16-byte pieces
(the aligned instantiation) only when the input is aligned AND G is a multiple of 4; the aligned view of 1 025 genes takes the
plain instantiation, as the shifted one does, and 3 x 1 024 and 5 x 1 028 are the aligned instantiation's whole and ragged
strip."""
import numpy as np

import thin_model as T

PLANTED = (63, 64, 65, 127, 128, 129, 4096)

# (N, G, view) -> (vec, strips, genes of the last strip, more than one row block)
CASES = {
    (259, 1025, "shifted"): (False, 2, 1, True),
    (259, 1025, "aligned"): (False, 2, 1, True),
    (1, 1, "aligned"): (False, 1, 1, False),
    (1, 1, "shifted"): (False, 1, 1, False),
    (3, 1024, "aligned"): (True, 1, 1024, False),
    (3, 1024, "shifted"): (False, 1, 1024, False),
    (2, 1023, "aligned"): (False, 1, 1023, False),
    (5, 1028, "aligned"): (True, 2, 4, False),
}

SCALAR_INTERVALS = [(0, 32768), (32768, 65536), (0, 1), (0, 65535), (1, 65536), (0, 65536), (12345, 12345)]


def layout(N, G, view):
    """(offset of the view's base from 16 bytes, its row stride) as tests/test_gpu_thin.py builds it."""
    if view == "aligned":
        return 0, G
    return 4, G + (3 if G % 2 == 0 else 2)


def counts(N, G):
    """About 60 % zeros, the rest small, and the planted counts where there is room for them (a 1 x 1 matrix holds 65)."""
    rng = np.random.default_rng(1000 * N + G)
    X = (1 + rng.poisson(2.0, size=(N, G))) * (rng.random((N, G)) >= 0.6)
    if N * G >= len(PLANTED):
        X.ravel()[rng.choice(N * G, size=len(PLANTED), replace=False)] = PLANTED
    else:
        X[:] = 65
    return X.astype(np.int32)


def tables(N):
    """(lo, hi) per cell: the scalar intervals and a few more, mixed row by row, so that one row block holds all of them."""
    rng = np.random.default_rng(N)
    pairs = SCALAR_INTERVALS + [(0, 16384), (777, 30001), (0, 0), (65536, 65536), (16384, 49152), (0, 12288)]
    pick = np.arange(N) % len(pairs) if N >= len(pairs) else rng.integers(0, len(pairs), size=N)
    lo = np.array([pairs[i][0] for i in pick], dtype=np.int64)
    hi = np.array([pairs[i][1] for i in pick], dtype=np.int64)
    return lo, hi


_model = {}


def model(N, G, lo, hi, seed=0):
    """The model's part of ``counts(N, G)``, computed once per interval; ``lo`` and ``hi`` numbers, or "tables"."""
    key = (N, G, lo if isinstance(lo, str) else (int(lo), int(hi)), seed)
    if key not in _model:
        a, b = tables(N) if isinstance(lo, str) else (lo, hi)
        _model[key] = T.interval(counts(N, G), a, b, seed=seed)
        _model[key].setflags(write=False)
    return _model[key]
