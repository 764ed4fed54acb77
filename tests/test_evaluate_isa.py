"""Properties of the evaluate kernels' gfx950 code object (prosstt_amd/csrc/evaluate/evaluate.hip), read from the ISA hipcc
writes with the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills, there
is no floating-point atomic, no LDS atomic and no global atomic but the status word's, the LDS of each instantiation is what
its arrays add up to, and the two passes are pure integer and read their columns through LDS."""
import re

import pytest

import isa

TABLE, FOLD_COUNTS, FOLD_MOMENTS = "evaluate_table_kernel", "evaluate_fold_kernelILb0", "evaluate_fold_kernelILb1"
PASS_COUNTS, PASS_MOMENTS = "evaluate_pass_kernelILb0", "evaluate_pass_kernelILb1"
KERNELS = [TABLE, PASS_COUNTS, PASS_MOMENTS, FOLD_COUNTS, FOLD_MOMENTS]
# a tile's columns (256 x 8) and keys (256 x 4), the four waves' five sums (4 x 5 x 8); the moments add J2 (64 x 64 x 4) and
# the four waves' flags
LDS = {TABLE: (2 * 64 + 2 * 65) * 8, PASS_COUNTS: 2048 + 1024 + 160, PASS_MOMENTS: 2048 + 1024 + 160 + 16384 + 16,
       FOLD_COUNTS: 2 * 256 * 8, FOLD_MOMENTS: 2 * 256 * 8}


def _code(kernel):
    """The kernel's instructions, comments aside, up to the end of the function (``isa.body`` stops at the first s_endpgm,
    which here is the early exit of a block without work)."""
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)^\.Lfunc_end" % kernel, isa.assembly("evaluate"), re.S | re.M)
    assert m, kernel
    return [line.split(";")[0] for line in m.group(2).splitlines()]


def test_every_kernel_is_listed():
    text = isa.assembly("evaluate")
    names = set(re.findall(r"\.name:\s+(_Z\S*evaluate_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_no_spill_and_the_lds_of_each_instantiation(kernel):
    text = isa.assembly("evaluate")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0
    lds = isa.meta(text, kernel, "group_segment_fixed_size")
    assert LDS[kernel] <= lds <= LDS[kernel] + 256, (kernel, lds)         # (the arrays, and the padding between them)


def test_the_only_atomic_is_the_status_words_or():
    text = isa.assembly("evaluate")
    assert not sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not isa.lds_atomics(text)
    for kernel in KERNELS:
        found = set(isa.global_atomics("\n".join(_code(kernel))))
        assert found <= {"global_atomic_or", "flat_atomic_or"}, (kernel, found)
        if kernel in (FOLD_COUNTS, FOLD_MOMENTS, PASS_COUNTS):
            assert not found, (kernel, found)                             # (the counts have nothing to report)


@pytest.mark.parametrize("kernel", [PASS_COUNTS, PASS_MOMENTS])
def test_the_passes_are_pure_integer_and_read_through_lds(kernel):
    code = _code(kernel)
    floating = sorted(set(m for line in code for m in re.findall(r"\bv_\w+_f(?:16|32|64)\b", line)))
    assert not floating, floating
    assert any("ds_read" in line or "ds_load" in line for line in code)
    if kernel == PASS_COUNTS:
        assert sum("v_med3_i32" in line for line in code) >= 64 and any("v_mad_i32_i24" in line for line in code)
    else:
        assert any("v_min3_i32" in line for line in code) and any("v_mad_u64_u32" in line for line in code)
