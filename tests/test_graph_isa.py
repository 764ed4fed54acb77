"""Properties of the graph kernels' gfx950 code object (prosstt_amd/csrc/graph/graph.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): no floating-point atomic anywhere, and no kernel uses
scratch."""
import re

import pytest

import isa

KERNELS = ["graph_memberships_kernel", "graph_emit_kernel", "graph_fold_kernel", "graph_normalize_kernelILi0E",
           "graph_normalize_kernelILi1E", "graph_normalize_kernelILi2E", "graph_spmv_kernelILi4E",
           "graph_spmv_kernelILi16E", "graph_spmv_kernelILi64E"]


def test_every_kernel_is_listed():
    text = isa.assembly("graph")
    names = set(re.findall(r"\.name:\s+(_Z\S*graph_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("graph")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomics():
    text = isa.assembly("graph")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # the atomics there are: the integer OR into the status word, nothing in LDS
    assert set(isa.global_atomics(text)) <= {"global_atomic_or"}
    assert not isa.lds_atomics(text)
