"""Properties of the thin kernel's gfx950 code object (prosstt_amd/csrc/thin/thin.hip), read from the ISA hipcc writes with the
library's own flags (cross-compiles without a GPU), on tests/isa.py as tests/test_factors_isa.py uses it: both instantiations
are there, neither uses scratch or spills a register, there is no floating-point atomic and no atomic but the status word's OR,
no LDS, no floating-point instruction at all, 16-byte loads and stores of global memory only in the aligned instantiation, and
a register count that keeps at least three waves per SIMD."""
import re

import pytest

import isa

KERNELS = ["thin_interval_kernelILb1EE", "thin_interval_kernelILb0EE"]


def test_every_kernel_is_listed():
    text = isa.assembly("thin")
    names = set(re.findall(r"\.name:\s+(_Z\S*thin_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spill_and_no_lds(kernel):
    text = isa.assembly("thin")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0
    assert isa.meta(text, kernel, "group_segment_fixed_size") == 0
    assert not re.search(r"\bds_(read|write|load|store)\w*", isa.body(text, kernel))


def test_no_floating_point_atomic_and_no_atomic_but_the_status_word():
    text = isa.assembly("thin")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) == {"global_atomic_or"}
    assert not isa.lds_atomics(text)
    for kernel in KERNELS:
        assert len(isa.global_atomics(isa.body(text, kernel))) == 1, kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_integer_arithmetic_only(kernel):
    body = isa.body(isa.assembly("thin"), kernel)
    found = sorted(set(re.findall(r"\bv_\w+_(?:f16|bf16|f32|f64)\b|\bv_cvt_\w+", body)))
    assert not found, found
    assert "v_bcnt_u32_b32" in body                              # the population count of a word's trials


def test_only_the_aligned_kernel_moves_rows_in_16_byte_pieces():
    text = isa.assembly("thin")
    aligned, plain = (isa.body(text, k) for k in KERNELS)
    assert "global_load_dwordx4" in aligned and "global_store_dwordx4" in aligned
    assert "global_load_dwordx4" not in plain and "global_store_dwordx4" not in plain
    # the ragged strip's 4-byte loads and stores are in both
    for body in (aligned, plain):
        flat = body.replace("\t", " ")
        assert "global_load_dword " in flat and "global_store_dword " in flat


def test_at_least_three_waves_per_simd():
    """512 vector registers per SIMD lane: at most 168 per wave keep three waves resident.  As built both instantiations take
    47 (DESIGN section 37 has the table), which keeps eight; a margin of 16 shows a drift long before 168 is near."""
    text = isa.assembly("thin")
    for kernel in KERNELS:
        count = isa.meta(text, kernel, "vgpr_count")
        assert count <= min(168, 47 + 16), (kernel, count)
