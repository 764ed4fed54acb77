"""Properties of the cluster kernels' gfx950 code object (prosstt_amd/csrc/cluster/cluster.hip), read from the ISA hipcc
writes with the library's own flags (cross-compiles without a GPU): no kernel uses scratch or spills a register, there is no
floating-point atomic, every atomic is an integer one, and the sweep's short-row paths use no LDS."""
import re

import pytest

import isa

KERNELS = ["cluster_quantize_kernel", "cluster_sweep_group_kernelILi16E", "cluster_sweep_group_kernelILi64E",
           "cluster_sweep_table_kernel", "cluster_sweep_range_kernel", "cluster_totals_kernel", "cluster_emit_kernel",
           "cluster_fold_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("cluster")
    names = set(re.findall(r"\.name:\s+(_Z\S*cluster_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("cluster")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic():
    text = isa.assembly("cluster")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # the atomics there are: the status word's or, the moved counter's add, the 64-bit adds of the totals and of the fold
    assert set(isa.global_atomics(text)) <= {"global_atomic_or", "global_atomic_add", "global_atomic_add_x2"}
    # and on LDS: the table's claim and add, the range kernel's add, presence bits and the row's lowest and highest community
    assert set(isa.lds_atomics(text)) <= {"ds_cmpst_rtn_b32", "ds_add_u64", "ds_or_b32", "ds_min_i32", "ds_max_i32"}


@pytest.mark.parametrize("kernel", ["cluster_sweep_group_kernelILi16E", "cluster_sweep_group_kernelILi64E"])
def test_the_short_row_paths_use_no_lds(kernel):
    text = isa.assembly("cluster")
    assert isa.meta(text, kernel, "group_segment_fixed_size") == 0
    body = isa.body(text, kernel)
    assert not isa.lds_atomics(body)
    assert "ds_read" not in body and "ds_load" not in body


@pytest.mark.parametrize("kernel,bytes_", [("cluster_sweep_table_kernel", 1024 * 12), ("cluster_sweep_range_kernel", 2048 * 8 + 256)])
def test_the_long_row_paths_keep_their_sums_in_lds(kernel, bytes_):
    text = isa.assembly("cluster")
    lds = isa.meta(text, kernel, "group_segment_fixed_size")
    assert bytes_ <= lds <= bytes_ + 128                      # the table or the range's array, and the reduction's few words
