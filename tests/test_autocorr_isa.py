"""Properties of the autocorr kernels' gfx950 code object (prosstt_amd/csrc/autocorr/autocorr.hip), read from the ISA hipcc
writes with the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or LDS or
spills a vector register, there is no floating-point atomic, nothing in the sums is fused into an fma (the numpy model
rounds every operation on its own), the four-genes-per-lane kernels read aligned rows with 16-byte loads, and what is
wave-uniform (the neighbour's index, weight and size factor) is read with scalar loads."""
import re

import pytest

import isa

KERNELS = ["autocorr_sums_kernelILi4E", "autocorr_sums_kernelILi1E", "autocorr_finish_kernel", "autocorr_smooth_kernelILi4E",
           "autocorr_smooth_kernelILi1E"]
FMA = re.compile(r"\bv_(fma|fmac|mad|mac|pk_fma)\w*_f(32|64)\b")


def test_every_kernel_is_listed():
    text = isa.assembly("autocorr")
    names = set(re.findall(r"\.name:\s+(_Z\S*autocorr_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_lds_and_no_spill(kernel):
    text = isa.assembly("autocorr")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "group_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    # (scalar registers: the two-path smoothing kernel at four genes per lane parks two of them in lanes of a vector
    # register, which costs a v_writelane / v_readlane each and no memory; the sums kernels park none)
    if "smooth" not in kernel:
        assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic():
    text = isa.assembly("autocorr")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) <= {"global_atomic_or"}            # the status word


@pytest.mark.parametrize("kernel", ["autocorr_sums_kernelILi4E", "autocorr_sums_kernelILi1E", "autocorr_finish_kernel"])
def test_the_sums_hold_no_fma(kernel):
    found = sorted(set(m.group(0) for m in FMA.finditer(isa.body(isa.assembly("autocorr"), kernel))))
    assert not found, found


def test_the_smoothing_kernels_fuse_only_inside_their_division():
    """1 / d_i is a correctly rounded binary64 division, which the compiler expands with v_fma_f64; the sums m = m + w * a
    are not fused: there is a v_mul_f64 and a v_add_f64 per gene of the lane."""
    text = isa.assembly("autocorr")
    for kernel, genes in (("autocorr_smooth_kernelILi4E", 4), ("autocorr_smooth_kernelILi1E", 1)):
        code = isa.body(text, kernel)
        assert not re.search(r"\bv_(fma|fmac|mad|mac)\w*_f32\b", code), kernel
        assert "v_div_scale_f64" in code and "v_div_fixup_f64" in code, kernel
        assert code.count("v_mul_f64") >= genes and code.count("v_add_f64") >= genes, kernel


def test_wide_loads_and_scalar_loads():
    text = isa.assembly("autocorr")
    for kernel in ("autocorr_sums_kernelILi4E", "autocorr_smooth_kernelILi4E"):
        assert "global_load_dwordx4" in isa.body(text, kernel), kernel
    for kernel in KERNELS[:2] + KERNELS[3:]:
        code = isa.body(text, kernel)
        assert "s_load_dwordx2" in code and "s_load_dword " in code, kernel       # weights and indptr; indices and inv_size
        assert "global_load_dwordx4" not in code or kernel.endswith("Li4E"), kernel
