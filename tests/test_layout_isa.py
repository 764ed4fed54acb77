"""Properties of the layout kernels' gfx950 code object (prosstt_amd/csrc/layout/layout.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no floating-point atomic anywhere, and no kernel uses
scratch."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["layout_epoch_kernelILi%dELi%dE" % (c, g) for c in (2, 3) for g in (4, 16, 64)] + ["layout_negatives_kernel"]


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_layout_isa_")
    try:
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fPIC", "-shared",
                               "-fvisibility=hidden", "-save-temps", "-o", os.path.join(tmp, "lib.so"),
                               os.path.join(ROOT, "prosstt_amd", "csrc", "layout", "layout.hip")],
                              cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "layout-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return text


def _meta(text, mangled_part, key):
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        if re.search(r"\.name:\s+\S*%s" % mangled_part, blk):
            return int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
    raise AssertionError(mangled_part)


def test_every_kernel_is_listed(isa):
    names = set(re.findall(r"\.name:\s+(_Z\S*layout_\S*_kernel\S*)", isa))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


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
    # there is no atomic at all, in global memory or in LDS
    assert not re.findall(r"\b(?:global|flat|buffer)_atomic_\w+", isa)
    assert not re.findall(r"\bds_(?:add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*", isa)
