"""Properties of the knn kernels' gfx950 code object (prosstt_amd/csrc/knn/knn.hip), read from the ISA hipcc writes with
the library's own flags (cross-compiles without a GPU): no scratch, no spills, no floating-point atomics anywhere, and a
distance kernel whose accumulation is a separate subtract, multiply and add (the definition: nothing fused)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
DISTANCE = ["knn_distance_kernelILb1E", "knn_distance_kernelILb0E"]
KERNELS = DISTANCE + ["knn_select_kernel"]


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_knn_isa_")
    try:
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fPIC", "-shared",
                               "-fvisibility=hidden", "-save-temps", "-o", os.path.join(tmp, "lib.so"),
                               os.path.join(ROOT, "prosstt_amd", "csrc", "knn", "knn.hip")],
                              cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "knn-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
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
    # the atomics there are: the histogram's and the gather counter's integer adds in LDS, nothing in global memory
    assert not re.findall(r"\b(?:global|flat|buffer)_atomic_\w+", isa)
    assert set(re.findall(r"\bds_(?:add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*", isa)) <= {"ds_add_u32", "ds_add_rtn_u32"}


@pytest.mark.parametrize("kernel", DISTANCE)
def test_distance_accumulation_is_not_fused(isa, kernel):
    body = _body(isa, kernel)
    # a full slice is unrolled: 32 coordinates x 16 pairs, each a v_sub_f32, a v_mul_f32 and a v_add_f32
    for op in ("v_sub_f32", "v_mul_f32", "v_add_f32"):
        assert len(re.findall(r"\b%s" % op, body)) >= 32 * 16, op
    # no fused multiply-add of any kind in the kernel (its address arithmetic is integer)
    assert not re.search(r"\bv_(pk_)?(fma|fmac|mad|mac)\w*_f(16|32|64)\b", body)
    assert not re.search(r"\bv_pk_(add|mul)_f32\b", body)


@pytest.mark.parametrize("kernel", DISTANCE)
def test_distance_tile_moves_16_bytes_at_a_time(isa, kernel):
    body = _body(isa, kernel)
    assert len(re.findall(r"\bds_read_b128\b|\bds_load_b128\b", body)) >= 2 * 32
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 4
    if kernel.endswith("Lb1E"):
        assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= 4
