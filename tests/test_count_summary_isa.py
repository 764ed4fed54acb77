"""Properties of the count-summary kernels' gfx950 code object (prosstt_amd/csrc/stats/count_summary.hip), read from the
ISA hipcc writes with the library's own flags (cross-compiles without a GPU)."""
import re

import pytest

import isa

KERNELS = ["count_summary_kernelILb1E", "count_summary_kernelILb0E", "count_summary_genes_kernel", "count_summary_rows_kernel"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("stats")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0


def test_main_kernel_reads_the_matrix_with_16_byte_loads():
    text = isa.assembly("stats")
    body = isa.body(text, "count_summary_kernelILb1E")
    # the full-strip path: one 16-byte load per lane and row, four rows at a time
    assert len(re.findall(r"global_load_dwordx4\b", body)) >= 4
    # four blocks of 256 threads per CU: one round of blocks over 256 CUs (the grid's sizing assumes it)
    assert isa.meta(text, "count_summary_kernelILb1E", "vgpr_count") <= 128
