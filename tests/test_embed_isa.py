"""Properties of the embed kernels' gfx950 code object (prosstt_amd/csrc/embed/embed.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no scratch, no spills, f32-input MFMA on the products, and
no floating-point atomics anywhere (the determinism rule: every reduction goes through slabs summed in a fixed order)."""
import re

import pytest

import isa

KERNELS = (["embed_moments_kernelILb1E", "embed_moments_kernelILb0E", "embed_sum_moments_kernel", "embed_sum_panels_kernel"]
           + ["embed_matmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)]
           + ["embed_rmatmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)])


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("embed")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomics():
    text = isa.assembly("embed")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # the one atomic there is: the status word's integer or
    assert set(re.findall(r"\b\w+_atomic_\w+", text)) <= {"global_atomic_or"}


@pytest.mark.parametrize("kernel,count", [("embed_matmul_kernelILi2ELb1E", 32), ("embed_rmatmul_kernelILi2ELb1E", 64)])
def test_products_run_on_f32_mfma(kernel, count):
    text = isa.assembly("embed")
    body = isa.body(text, kernel)
    # per step of 32: 16 k-steps of v_mfma_f32_32x32x2_f32 per 32 x 32 output tile (2 tiles for matmul, 4 for rmatmul)
    assert len(re.findall(r"v_mfma_f32_32x32x2_f32\b", body)) >= count
    assert not re.search(r"v_mfma_\w*(bf16|f16|xf32)", body)


def test_matmul_reads_the_matrix_with_16_byte_loads():
    text = isa.assembly("embed")
    assert len(re.findall(r"global_load_dwordx4\b", isa.body(text, "embed_matmul_kernelILi2ELb1E"))) >= 4
