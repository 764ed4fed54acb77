"""Properties of the hvg kernels' gfx950 code object (prosstt_amd/csrc/hvg/hvg.hip), read from the ISA hipcc writes with the
library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register, and
there is no floating-point atomic."""
import re

import pytest

import isa

KERNELS = ["hvg_clipped_kernelILb1E", "hvg_clipped_kernelILb0E", "hvg_clipped_sum_kernel", "hvg_moments_kernelILb1E",
           "hvg_moments_kernelILb0E", "hvg_moments_sum_kernel", "hvg_gather_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("hvg")
    names = set(re.findall(r"\.name:\s+(_Z\S*hvg_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("hvg")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic():
    text = isa.assembly("hvg")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found


def test_the_strip_kernels_read_aligned_rows_with_16_byte_loads():
    text = isa.assembly("hvg")
    for kernel in ("hvg_clipped_kernelILb1E", "hvg_moments_kernelILb1E"):
        assert "global_load_dwordx4" in isa.body(text, kernel), kernel
