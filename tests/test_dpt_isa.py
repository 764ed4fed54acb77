"""Properties of the DPT kernels' gfx950 code object (prosstt_amd/csrc/dpt/dpt.hip), read from the ISA hipcc writes with the
library's own flags (cross-compiles without a GPU): no kernel uses scratch or spills a register, there is no floating-point
atomic, and the concordance kernel is pure integer and reads its columns through LDS."""
import re

import pytest

import isa

KERNELS = ["dpt_rows_kernel", "dpt_concordance_kernel", "dpt_reduce_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("dpt")
    names = set(re.findall(r"\.name:\s+(_Z\S*dpt_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("dpt")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic():
    text = isa.assembly("dpt")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found


def test_the_concordance_kernel_is_pure_integer_and_reads_through_lds():
    body = isa.body(isa.assembly("dpt"), "dpt_concordance_kernel")
    code = [line.split(";")[0] for line in body.splitlines()]            # (comments aside)
    floating = sorted(set(m for line in code for m in re.findall(r"\b\w+_f(?:32|64)\b", line)))
    assert not floating, floating
    assert any("ds_read" in line or "ds_load" in line for line in code)
