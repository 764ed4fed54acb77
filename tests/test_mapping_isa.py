"""Properties of the mapping kernels' gfx950 code object (prosstt_amd/csrc/mapping/mapping.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register,
every instantiation of the pass multiplies with v_mfma_f32_32x32x2_f32 on counts converted by v_cvt_f32_i32 and adds its chains
in binary64 without a fused multiply-add, there is no floating-point atomic and no atomic but the status word's OR, only the
aligned instantiations read rows with 16-byte loads, and the LDS bytes and vector registers are what the build gives."""
import re

import pytest

import isa

PASS = ["mapping_pass_kernelILi%dELb%dE" % (nt, vec) for nt in (1, 2, 3, 4) for vec in (1, 0)]
KERNELS = PASS + ["mapping_finish_kernel"]
# the 32 genes x (32 NT + 2) nodes slice of the panel, binary32
LDS = {k: 32 * (32 * int(k[len("mapping_pass_kernelILi")]) + 2) * 4 for k in PASS}
# vector registers, accumulation registers included: 32 NT of the binary64 sums, 16 NT accumulators, the 16 counts in flight,
# their 16 conversions, 4 NT panel entries in flight and the panel values read ahead of the matrix instructions.  512 per lane
# of a SIMD, handed out in blocks of 8.
VGPRS = {"mapping_pass_kernelILi1ELb1E": 144, "mapping_pass_kernelILi1ELb0E": 144,
         "mapping_pass_kernelILi2ELb1E": 240, "mapping_pass_kernelILi2ELb0E": 240,
         "mapping_pass_kernelILi3ELb1E": 288, "mapping_pass_kernelILi3ELb0E": 288,
         "mapping_pass_kernelILi4ELb1E": 368, "mapping_pass_kernelILi4ELb0E": 370}
WAVES = {1: 3, 2: 2, 3: 1, 4: 1}              # waves per SIMD by NT


def test_every_kernel_is_listed():
    text = isa.assembly("mapping")
    names = set(re.findall(r"\.name:\s+(_Z\S*mapping_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spill_and_the_lds_of_the_panel_slice(kernel):
    text = isa.assembly("mapping")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0
    assert isa.meta(text, kernel, "group_segment_fixed_size") == LDS.get(kernel, 0)


def test_no_floating_point_atomic_and_no_atomic_but_the_status_or():
    text = isa.assembly("mapping")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) == {"global_atomic_or"}
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("kernel", PASS)
def test_the_pass_multiplies_on_the_matrix_cores_and_adds_its_chains_in_binary64(kernel):
    code = isa.body(isa.assembly("mapping"), kernel)
    nt = int(kernel[len("mapping_pass_kernelILi")])
    assert code.count("v_mfma_f32_32x32x2_f32") == 16 * nt           # one loop body: 16 k-steps per 32-node tile
    assert not re.findall(r"\bv_mfma_(?!f32_32x32x2_f32)\w+", code)
    assert code.count("v_cvt_f32_i32") == 16                          # the lane's 16 counts of a step
    assert code.count("v_cvt_f64_f32") >= 16 * nt and code.count("v_add_f64") >= 16 * nt
    assert "v_mul_f64" in code and "v_fma_f64" not in code            # S = (D - s m) + c, nothing contracted
    assert not re.findall(r"\bv_(?:fma|mac|fmac|mad)_f32\b", code)      # every binary32 product is the matrix instruction's


def test_wide_loads_in_the_aligned_pass_only():
    text = isa.assembly("mapping")
    for kernel in PASS:
        code = isa.body(text, kernel)
        assert ("global_load_dwordx4" in code) == kernel.endswith("Lb1E"), kernel
        assert "global_load_dword " in code, kernel                    # the panel, and the rows of a ragged step
    assert "global_load_dwordx4" not in isa.body(text, "mapping_finish_kernel")


@pytest.mark.parametrize("kernel", PASS)
def test_vector_registers_and_waves_per_simd_of_the_pass(kernel):
    text = isa.assembly("mapping")
    nt = int(kernel[len("mapping_pass_kernelILi")])
    assert isa.meta(text, kernel, "vgpr_count") == VGPRS[kernel]
    assert 512 // (8 * -(-VGPRS[kernel] // 8)) == WAVES[nt]
