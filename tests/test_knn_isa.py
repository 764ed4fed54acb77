"""Properties of the knn kernels' gfx950 code object (prosstt_amd/csrc/knn/knn.hip), read from the ISA hipcc writes with
the library's own flags (cross-compiles without a GPU): no scratch, no spills, no floating-point atomics anywhere, and a
distance kernel whose accumulation is a separate subtract, multiply and add (the definition: nothing fused)."""
import re

import pytest

import isa

DISTANCE = ["knn_distance_kernelILb1E", "knn_distance_kernelILb0E"]
KERNELS = DISTANCE + ["knn_select_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("knn")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomics():
    text = isa.assembly("knn")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # the atomics there are: the histogram's and the gather counter's integer adds in LDS, nothing in global memory
    assert not isa.global_atomics(text)
    assert set(isa.lds_atomics(text)) <= {"ds_add_u32", "ds_add_rtn_u32"}


@pytest.mark.parametrize("kernel", DISTANCE)
def test_distance_accumulation_is_not_fused(kernel):
    text = isa.assembly("knn")
    body = isa.body(text, kernel)
    # a full slice is unrolled: 32 coordinates x 16 pairs, each a v_sub_f32, a v_mul_f32 and a v_add_f32
    for op in ("v_sub_f32", "v_mul_f32", "v_add_f32"):
        assert len(re.findall(r"\b%s" % op, body)) >= 32 * 16, op
    # no fused multiply-add of any kind in the kernel (its address arithmetic is integer)
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)\b", body)
    assert not re.search(r"\bv_pk_(add|mul)_f32\b", body)


@pytest.mark.parametrize("kernel", DISTANCE)
def test_distance_tile_moves_16_bytes_at_a_time(kernel):
    text = isa.assembly("knn")
    body = isa.body(text, kernel)
    assert len(re.findall(r"\bds_read_b128\b|\bds_load_b128\b", body)) >= 2 * 32
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 4
    if kernel.endswith("Lb1E"):
        assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= 4
