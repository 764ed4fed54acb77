"""Properties of the trends kernels' gfx950 code object (prosstt_amd/csrc/trends/trends.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register,
there is no floating-point instruction in the pass at all and no atomic but the status word's OR, only the aligned
instantiation of the pass reads rows with 16-byte loads, an entry's index and weight come through scalar loads, the sums are
64-bit multiply-adds, and the vector registers of the pass are what the build gives."""
import re

import pytest

import isa

KERNELS = ["trends_table_kernel", "trends_pass_kernelILb1E", "trends_pass_kernelILb0E", "trends_finish_kernel"]
PASS = KERNELS[1:3]
# 512 vector registers per lane of a SIMD, handed out in blocks of 8: 80 -> 6 waves per SIMD, 81 -> 88 -> 5 waves
VGPRS = {"trends_pass_kernelILb1E": 80, "trends_pass_kernelILb0E": 81}
WAVES = {"trends_pass_kernelILb1E": 6, "trends_pass_kernelILb0E": 5}


def test_every_kernel_is_listed():
    text = isa.assembly("trends")
    names = set(re.findall(r"\.name:\s+(_Z\S*trends_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("trends")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0
    # LDS: the table kernel's scan of 1024 int64 alone
    assert isa.meta(text, kernel, "group_segment_fixed_size") == (8192 if kernel == "trends_table_kernel" else 0)


def test_no_floating_point_atomic_and_no_atomic_but_the_status_or():
    text = isa.assembly("trends")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) == {"global_atomic_or"}
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("kernel", PASS + ["trends_finish_kernel"])
def test_the_sums_are_integer_arithmetic(kernel):
    code = isa.body(isa.assembly("trends"), kernel)
    found = sorted(set(re.findall(r"\bv_\w+_f(?:16|32|64)\b", code)))
    assert not found, found
    if kernel in PASS:
        # per entry and gene: x^2, q x, q lo, q hi; the batch of four entries and the one-by-one tail, two strip forms at most
        assert code.count("v_mad_u64_u32") >= 4 * 4 * 5, code.count("v_mad_u64_u32")


def test_wide_loads_in_the_aligned_pass_only_and_scalar_loads_of_the_entries():
    text = isa.assembly("trends")
    assert "global_load_dwordx4" in isa.body(text, "trends_pass_kernelILb1E")
    assert "global_load_dwordx4" not in isa.body(text, "trends_pass_kernelILb0E")
    assert "global_load_dwordx4" not in isa.body(text, "trends_finish_kernel")
    for kernel in PASS:
        code = isa.body(text, kernel)
        assert "s_load_dwordx4" in code or "s_load_dword " in code, kernel        # indices and weights: block-uniform
        assert "global_load_dword " in code, kernel                               # the rows outside a whole strip


@pytest.mark.parametrize("kernel", PASS)
def test_vector_registers_of_the_pass(kernel):
    """24 accumulator registers and 16 of the four rows in flight per lane, and the addresses: 80 vector registers (six waves
    per SIMD) in the aligned instantiation, 81 (allocated as 88: five waves) in the other."""
    text = isa.assembly("trends")
    assert isa.meta(text, kernel, "vgpr_count") == VGPRS[kernel]
    assert 512 // (8 * -(-VGPRS[kernel] // 8)) == WAVES[kernel]
