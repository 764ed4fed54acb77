"""Properties of the count-summary kernels' gfx950 code object (prosstt_amd/csrc/stats/count_summary.hip), read from the
ISA hipcc writes with the library's own flags (cross-compiles without a GPU)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ["count_summary_kernelILb1E", "count_summary_kernelILb0E", "count_summary_genes_kernel", "count_summary_rows_kernel"]


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_stats_isa_")
    try:
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                               "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-fPIC", "-shared",
                               "-fvisibility=hidden", "-save-temps", "-o", os.path.join(tmp, "lib.so"),
                               os.path.join(ROOT, "prosstt_amd", "csrc", "stats", "count_summary.hip")],
                              cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(os.path.join(tmp, "count_summary-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
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


def test_main_kernel_reads_the_matrix_with_16_byte_loads(isa):
    body = _body(isa, "count_summary_kernelILb1E")
    # the full-strip path: one 16-byte load per lane and row, four rows at a time
    assert len(re.findall(r"global_load_dwordx4\b", body)) >= 4
    # four blocks of 256 threads per CU: one round of blocks over 256 CUs (the grid's sizing assumes it)
    assert _meta(isa, "count_summary_kernelILb1E", "vgpr_count") <= 128
