"""The column kernels' plan on the host (prosstt_amd/csrc/column_device.h): fit and regress cut the rows
of a matrix by the one rule, ``row_blocking`` of abi_util.h, and ``regress.row_blocks`` is that rule in Python.  Their
``*_workspace_bytes`` are host code, so this needs no device: the byte counts are restated here from each library's slab
layout, every slab padded to 256 bytes.  The sums' bit patterns depend on the blocking (a gene's terms are added within a
block, then over the blocks), and a slip in the shared rule would otherwise show only as a last-bit difference on the GPU."""
import ctypes

import pytest

from prosstt_amd import _native, regress

SHAPES = [(1, 1), (64, 300), (65, 300), (700, 256), (300, 257), (300, 128), (50000, 20000), (2 ** 31 - 1, 1)]


def pad(n):
    return (n + 255) // 256 * 256


def asked(name, symbol, N, G, parameter):
    need = ctypes.c_uint64(0)
    _native.check(getattr(_native.load(name), symbol)(N, G, parameter, ctypes.byref(need)), name)
    return need.value


@pytest.mark.parametrize("N, G", SHAPES)
@pytest.mark.parametrize("C", [1, 16])
def test_fit_workspace_follows_the_row_blocks(N, G, C):
    cells = regress.row_blocks(N, G)[1] * G
    # ll [row_blocks][C][G] float64, base [row_blocks][G] float64, bad [row_blocks][G] uint32
    want = pad(cells * C * 8) + pad(cells * 8) + pad(cells * 4)
    assert asked("fit", "prosstt_amd_fit_workspace_bytes", N, G, C) == want


@pytest.mark.parametrize("N, G", SHAPES)
@pytest.mark.parametrize("p", [1, 16])
def test_regress_workspace_follows_the_row_blocks(N, G, p):
    cells = regress.row_blocks(N, G)[1] * G
    sums = p + p * (p + 1) // 2
    # U, I and Q [row_blocks][sums + 1][G] float64, used [row_blocks][G] uint32
    want = pad(cells * (sums + 1) * 8) + pad(cells * 4)
    assert asked("regress", "prosstt_amd_regress_workspace_bytes", N, G, p) == want
