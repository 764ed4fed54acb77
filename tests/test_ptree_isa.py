"""Properties of the ptree kernels' gfx950 code object (prosstt_amd/csrc/ptree/ptree.hip), read from the ISA hipcc writes with
the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register, the
sums are separate binary64 multiplies and adds, the distances separate binary32 ones, and there is no floating-point atomic and
no atomic but the status word's OR.

The soft per-cell kernel and the projection divide in binary64, and the soft kernel calls exp and log: hipcc expands a
correctly rounded division, and the device library its exp and log, with v_fma_f64 of their own.  Those two kernels can
therefore not be free of v_fma_f64; that their own products are not contracted is pinned bit for bit by tests/test_gpu_ptree.py
(t and q of the projection, the exact cases of the soft pass).  Every other kernel is checked here."""
import re

import pytest

import isa

SUMS = ["ptree_sums_kernelILi%dELb%dE" % (q, hard) for q in (1, 2, 4, 8, 16) for hard in (0, 1)]
CELL = ["ptree_cell_kernelILb0E", "ptree_cell_kernelILb1E"]
KERNELS = ["ptree_distance_kernel", "ptree_fold_kernel", "ptree_project_kernel"] + CELL + SUMS
DIVIDING = ("ptree_cell_kernelILb1E", "ptree_project_kernel")


def test_every_kernel_is_listed():
    text = isa.assembly("ptree")
    names = set(re.findall(r"\.name:\s+(_Z\S*ptree_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("ptree")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic_and_no_atomic_but_the_status_or():
    text = isa.assembly("ptree")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) == {"global_atomic_or"}
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("kernel", SUMS + ["ptree_project_kernel", "ptree_cell_kernelILb1E"])
def test_the_passes_multiply_and_add_in_binary64(kernel):
    code = isa.body(isa.assembly("ptree"), kernel)
    assert "v_mul_f64" in code and "v_add_f64" in code


@pytest.mark.parametrize("kernel", [k for k in KERNELS if k not in DIVIDING])
def test_nothing_is_fused_where_nothing_divides(kernel):
    code = isa.body(isa.assembly("ptree"), kernel)
    assert "v_fma_f64" not in code
    assert not re.findall(r"\bv_(?:fma|mac|fmac|mad)_f32\b", code)


@pytest.mark.parametrize("kernel", DIVIDING)
def test_no_binary32_fma_in_the_dividing_kernels(kernel):
    assert not re.findall(r"\bv_(?:fma|mac|fmac|mad)_f32\b", isa.body(isa.assembly("ptree"), kernel))


def test_the_distances_are_separate_binary32_operations():
    code = isa.body(isa.assembly("ptree"), "ptree_distance_kernel")
    assert "v_sub_f32" in code and "v_mul_f32" in code and "v_add_f32" in code
