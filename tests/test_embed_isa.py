"""Properties of the embed kernels' gfx950 code object (prosstt_amd/csrc/embed/embed.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no scratch, no spills, f32-input MFMA on the products, and
no floating-point atomics anywhere (the determinism rule: every reduction goes through slabs summed in a fixed order)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = (["embed_moments_kernelILb1E", "embed_moments_kernelILb0E", "embed_sum_moments_kernel", "embed_sum_panels_kernel"]
           + ["embed_matmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)]
           + ["embed_rmatmul_kernelILi%dELb%dE" % (nt, v) for nt in (1, 2, 3, 4) for v in (0, 1)])


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_embed_isa_")
    try:
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fPIC", "-shared",
                               "-fvisibility=hidden", "-save-temps", "-o", os.path.join(tmp, "lib.so"),
                               os.path.join(ROOT, "prosstt_amd", "csrc", "embed", "embed.hip")],
                              cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "embed-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return text


def _body(text, mangled_part):
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s+s_endpgm" % mangled_part, text, re.S | re.M)
    assert m, mangled_part
    return m.group(2)


def _meta(text, mangled_part, key):
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        if re.search(r"\.name:\s+\S*%s" % mangled_part, blk):
            return int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
    raise AssertionError(mangled_part)


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(isa, kernel):
    assert _meta(isa, kernel, "private_segment_fixed_size") == 0
    assert _meta(isa, kernel, "vgpr_spill_count") == 0
    assert _meta(isa, kernel, "sgpr_spill_count") == 0


# any floating-point atomic: global / flat / buffer / LDS add, min, max, pk_add on f16, bf16, f32 or f64
FLOAT_ATOMIC = re.compile(r"\b(global|flat|buffer|ds)_(atomic_)?(add|sub|pk_add|min|max|fmin|fmax|cmpswap)\w*_(f16|bf16|f32|f64)\b"
                          r"|\bds_(add|min|max)_rtn_f\d+\b|\b\w+_atomic_\w*f(32|64)\b")


def test_no_floating_point_atomics(isa):
    found = sorted(set(m.group(0) for m in FLOAT_ATOMIC.finditer(isa)))
    assert not found, found
    # the one atomic there is: the status word's integer or
    assert set(re.findall(r"\b\w+_atomic_\w+", isa)) <= {"global_atomic_or"}


@pytest.mark.parametrize("kernel,count", [("embed_matmul_kernelILi2ELb1E", 32), ("embed_rmatmul_kernelILi2ELb1E", 64)])
def test_products_run_on_f32_mfma(isa, kernel, count):
    body = _body(isa, kernel)
    # per step of 32: 16 k-steps of v_mfma_f32_32x32x2_f32 per 32 x 32 output tile (2 tiles for matmul, 4 for rmatmul)
    assert len(re.findall(r"v_mfma_f32_32x32x2_f32\b", body)) >= count
    assert not re.search(r"v_mfma_\w*(bf16|f16|xf32)", body)


def test_matmul_reads_the_matrix_with_16_byte_loads(isa):
    assert len(re.findall(r"global_load_dwordx4\b", _body(isa, "embed_matmul_kernelILi2ELb1E"))) >= 4
