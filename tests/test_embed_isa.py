"""Properties of the embed kernels' gfx950 code object (prosstt_amd/csrc/embed/embed.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no scratch, no spills, in every instantiation of the products
exactly the f32-input MFMAs of one loop body and no other, wide row loads in the aligned instantiations only, the LDS bytes
and vector registers the build gives, and no floating-point atomics anywhere (the determinism rule: every reduction goes
through slabs summed in a fixed order)."""
import re

import pytest

import isa

MATMUL = ["embed_matmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)]
RMATMUL = ["embed_rmatmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)]
KERNELS = (["embed_moments_kernelILb1E", "embed_moments_kernelILb0E", "embed_sum_moments_kernel", "embed_sum_panels_kernel"]
           + MATMUL + RMATMUL)
TILES = {k: int(k[k.index("ILi") + 3]) for k in MATMUL + RMATMUL}        # NT
# the 32 x (32 NT + 2) slice of the panel, binary32 (mfma_device.h); rmatmul also stages the 32 inverse sizes of a step
LDS = {k: 32 * (32 * TILES[k] + 2) * 4 + (128 if k in RMATMUL else 0) for k in MATMUL + RMATMUL}
# vector registers as the build gives them, accumulation registers included: 16 NT accumulators in matmul and 32 NT in
# rmatmul (two genes per lane), the 16 or 32 counts in flight, their entries log1p(x / s) and the temporaries of forming them,
# 4 NT panel entries in flight and the panel values read ahead of the matrix instructions.  512 per lane of a SIMD, handed
# out in blocks of 8.
VGPRS = {"embed_matmul_kernelILi1ELb1E": 152, "embed_matmul_kernelILi1ELb0E": 156,
         "embed_matmul_kernelILi2ELb1E": 192, "embed_matmul_kernelILi2ELb0E": 192,
         "embed_matmul_kernelILi3ELb1E": 232, "embed_matmul_kernelILi3ELb0E": 232,
         "embed_matmul_kernelILi4ELb1E": 264, "embed_matmul_kernelILi4ELb0E": 268,
         "embed_rmatmul_kernelILi1ELb1E": 228, "embed_rmatmul_kernelILi1ELb0E": 192,
         "embed_rmatmul_kernelILi2ELb1E": 280, "embed_rmatmul_kernelILi2ELb0E": 244,
         "embed_rmatmul_kernelILi3ELb1E": 340, "embed_rmatmul_kernelILi3ELb0E": 304,
         "embed_rmatmul_kernelILi4ELb1E": 386, "embed_rmatmul_kernelILi4ELb0E": 356}


def test_every_kernel_is_listed():
    text = isa.assembly("embed")
    names = set(re.findall(r"\.name:\s+(_Z\S*embed_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


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


@pytest.mark.parametrize("kernel,count", [(k, 16 * TILES[k]) for k in MATMUL] + [(k, 32 * TILES[k]) for k in RMATMUL])
def test_products_run_on_f32_mfma(kernel, count):
    text = isa.assembly("embed")
    body = isa.body(text, kernel)
    # one loop body: per step of 32, 16 k-steps of v_mfma_f32_32x32x2_f32 per 32 x 32 output tile (NT tiles for matmul, 2 NT
    # for rmatmul's two genes per lane)
    assert body.count("v_mfma_f32_32x32x2_f32") == count
    assert not re.findall(r"\bv_mfma_(?!f32_32x32x2_f32)\w+", body)


def test_matmul_reads_the_matrix_with_16_byte_loads():
    text = isa.assembly("embed")
    assert len(re.findall(r"global_load_dwordx4\b", isa.body(text, "embed_matmul_kernelILi2ELb1E"))) >= 4
    # wide row loads in the aligned instantiations only: 16 bytes in matmul (16 consecutive counts of a row), 8 in rmatmul
    # (the lane's two genes); the panel and the ragged steps take 4-byte loads everywhere
    for kernel in MATMUL + RMATMUL:
        code = isa.body(text, kernel)
        wide = "global_load_dwordx4" if kernel in MATMUL else "global_load_dwordx2"
        assert (wide in code) == kernel.endswith("Lb1E"), kernel
        assert "global_load_dwordx4" not in code or kernel in MATMUL, kernel
        assert "global_load_dword " in code, kernel


@pytest.mark.parametrize("kernel", MATMUL + RMATMUL)
def test_vector_registers_and_lds_of_the_products(kernel):
    text = isa.assembly("embed")
    assert isa.meta(text, kernel, "vgpr_count") == VGPRS[kernel]
    assert isa.meta(text, kernel, "group_segment_fixed_size") == LDS[kernel]
