"""Properties of the layout kernels' gfx950 code object (prosstt_amd/csrc/layout/layout.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no floating-point atomic anywhere, and no kernel uses
scratch."""
import re

import pytest

import isa

KERNELS = ["layout_epoch_kernelILi%dELi%dE" % (c, g) for c in (2, 3) for g in (4, 16, 64)] + ["layout_negatives_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("layout")
    names = set(re.findall(r"\.name:\s+(_Z\S*layout_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("layout")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomics():
    text = isa.assembly("layout")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # there is no atomic at all, in global memory or in LDS
    assert not isa.global_atomics(text)
    assert not isa.lds_atomics(text)
