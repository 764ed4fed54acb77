"""Properties of the fit kernels' gfx950 code object (prosstt_amd/csrc/fit/fit.hip), read from the ISA hipcc writes with the
library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register, there
is no floating-point atomic, and the aligned kernel reads the matrix with 16-byte loads."""
import re

import pytest

import isa

KERNELS = ["fit_loglik_kernelILb1E", "fit_loglik_kernelILb0E", "fit_finish_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("fit")
    names = set(re.findall(r"\.name:\s+(_Z\S*fit_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("fit")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic_and_no_atomic_but_the_status_word():
    text = isa.assembly("fit")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) <= {"global_atomic_or", "flat_atomic_or"}
    assert not isa.lds_atomics(text)


def test_the_aligned_kernel_reads_rows_with_16_byte_loads_and_stages_them_in_lds():
    text = isa.assembly("fit")
    aligned = isa.body(text, "fit_loglik_kernelILb1E")
    assert "global_load_dwordx4" in aligned and "ds_write_b128" in aligned
    assert isa.meta(text, "fit_loglik_kernelILb1E", "group_segment_fixed_size") == 8 * 256 * 4
    assert "global_load_dwordx4" not in isa.body(text, "fit_loglik_kernelILb0E")


def test_three_waves_per_simd_fit():
    """512 vector registers per SIMD lane: at most 168 per wave keeps three waves resident, which is what hides the
    latency of the binary64 chains."""
    text = isa.assembly("fit")
    for kernel in KERNELS[:2]:
        assert isa.meta(text, kernel, "vgpr_count") <= 168, kernel
