"""Properties of the markers kernels' gfx950 code object (prosstt_amd/csrc/markers/markers.hip), read from the ISA hipcc
writes with the library's own flags (cross-compiles without a GPU): no kernel uses scratch or spills a register, there is no
floating-point atomic, and the pass reads the matrix with 16-byte loads and its row indices with scalar loads."""
import re

import pytest

import isa

KERNELS = ["markers_table_kernel", "markers_pass_kernelILb1E", "markers_pass_kernelILb0E", "markers_finish_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("markers")
    names = set(re.findall(r"\.name:\s+(_Z\S*markers_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("markers")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic():
    text = isa.assembly("markers")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # the one atomic there is: the status word's integer or
    assert set(re.findall(r"\b\w+_atomic_\w+", text)) <= {"global_atomic_or"}


def test_the_pass_loads_rows_wide_and_their_indices_as_scalars():
    body = isa.body(isa.assembly("markers"), "markers_pass_kernelILb1E")
    code = [line.split(";")[0] for line in body.splitlines()]
    assert sum("global_load_dwordx4" in line for line in code) >= 4          # a batch of rows in flight
    assert any(re.search(r"\bs_load_dword(x\d)?\b", line) for line in code)
    assert any(re.search(r"v_fmac?_f64", line) for line in code) and any("v_log_f32" in line for line in code)
