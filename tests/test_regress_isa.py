"""Properties of the regress kernels' gfx950 code object (prosstt_amd/csrc/regress/regress.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU): every kernel is there, none uses scratch or spills a register,
there is no floating-point atomic, only the aligned kernels read the matrix with 16-byte loads, and the products and sums of
the definition are not contracted.

On contraction.  Binary64 division on gfx950 is a sequence of v_fma_f64 around v_rcp_f64 (v_div_scale, v_div_fmas, v_div_fixup),
and HIP's exp, log1p and log are polynomials in v_fma_f64, so the text of a pass that divides and takes an exponential cannot
be free of the instruction (libprosstt_amd_fit.so holds 534 of them).  What the definition asks is that none of ITS products
and sums is fused.  The kernels that add the sums of (U, I) hold, per block, ACC accumulations "sum + factor * value" and the
16 of eta: compiled with contraction allowed every one of them becomes a fused multiply-add, so the count of v_fma_f64 rises
by at least ACC from the library's build to that one, and the library's build holds at least as many v_mul_f64 and v_add_f64
as the definition has products and sums.  Both are asserted; -ffp-contract=off is the makefile's flag for every library.

And directly: a sums kernel calls exp once and divides twice (w and u), and log1p and log belong to the instantiation that adds
Q, so the fused operations of its text are those of one exp and two divisions whatever ACC is.  Their count is therefore the
SAME in the six sums kernels (23 with ROCm 7: 9 v_fma_f64 and 14 v_fmac_f64), within the budget of two divisions (at most 8
each, one v_div_fmas_f64 apiece) and one exp (at most 16), while the separate multiplies and adds grow by exactly 3 per sum (one
in the loop of a block of one kind, two in that of a mixed block).  One contracted accumulation makes the count depend on ACC;
a contracted eta adds 16 and leaves the budget."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import isa

SPLITS = (8, 16, 32, 0)                 # ACC of an instantiation; 0 adds Q and used
KERNELS = ["regress_pass_kernelILb%dELi%dE" % (vec, acc) for acc in SPLITS for vec in (1, 0)] + ["regress_finish_kernel"]


def test_every_kernel_is_listed():
    text = isa.assembly("regress")
    names = set(re.findall(r"\.name:\s+(_Z\S*regress_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("regress")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic_and_no_atomic_but_the_status_word():
    text = isa.assembly("regress")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) <= {"global_atomic_or", "flat_atomic_or"}
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("acc", SPLITS)
def test_only_the_aligned_kernel_reads_rows_with_16_byte_loads_and_stages_them_in_lds(acc):
    text = isa.assembly("regress")
    aligned = isa.body(text, "regress_pass_kernelILb1ELi%dE" % acc)
    assert "global_load_dwordx4" in aligned and "ds_write_b128" in aligned
    assert "global_load_dwordx4" not in isa.body(text, "regress_pass_kernelILb0ELi%dE" % acc)
    # the tile of 8 rows of 256 counts, beside the rows' sizes, design rows and factors
    tile = 8 * 256 * 4
    lds = isa.meta(text, "regress_pass_kernelILb1ELi%dE" % acc, "group_segment_fixed_size")
    assert tile < lds <= tile + 8 * (8 + 8 + 4 + 128 + 2 * 8 * max(acc, 1))
    assert isa.meta(text, "regress_pass_kernelILb0ELi%dE" % acc, "group_segment_fixed_size") < tile


def test_the_waves_per_simd_that_the_registers_allow():
    """512 vector registers per SIMD lane: at most 168 per wave keep three waves resident, at most 256 two (DESIGN section
    31 holds the counts of this build and what was measured with them)."""
    text = isa.assembly("regress")
    for vec in (1, 0):
        assert isa.meta(text, "regress_pass_kernelILb%dELi8E" % vec, "vgpr_count") <= 168
        assert isa.meta(text, "regress_pass_kernelILb%dELi0E" % vec, "vgpr_count") <= 168
        assert isa.meta(text, "regress_pass_kernelILb%dELi16E" % vec, "vgpr_count") <= 256
        assert isa.meta(text, "regress_pass_kernelILb%dELi32E" % vec, "vgpr_count") <= 256


FUSED = re.compile(r"\bv_(fma|fmac)_f64")


def test_the_fused_operations_of_a_sums_kernel_are_those_of_exp_and_two_divisions():
    text = isa.assembly("regress")
    counts = {}
    for acc in (8, 16, 32):
        for vec in (1, 0):
            body = isa.body(text, "regress_pass_kernelILb%dELi%dE" % (vec, acc))
            assert len(re.findall(r"\bv_div_fmas_f64", body)) == 2, (vec, acc)          # w and u, nothing else divides
            counts[vec, acc] = (len(FUSED.findall(body)), len(re.findall(r"\bv_mul_f64", body)) - 3 * acc,
                                len(re.findall(r"\bv_add_f64", body)) - 3 * acc)
    assert len(set(counts.values())) == 1, counts                # nothing depends on ACC or on the loads
    fused, multiplies, adds = counts[1, 8]
    assert 0 < fused <= 2 * 8 + 16, counts
    assert multiplies >= 16 and adds >= 16, counts               # eta's sixteen products and sums are separate instructions


def _contracted():
    """The assembly of the library compiled with contraction allowed (EXTRA comes after the makefile's own flags)."""
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_regress_contract_")
    try:
        subprocess.check_call(["make", "-C", os.path.join(isa.ROOT, "prosstt_amd", "csrc"), "isa-regress", "ISA_DIR=" + tmp,
                               "EXTRA=-ffp-contract=fast"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(os.path.join(tmp, "regress.s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_the_products_and_sums_of_the_definition_are_not_contracted():
    makefile = open(os.path.join(isa.ROOT, "prosstt_amd", "csrc", "Makefile")).read()
    assert re.search(r"^FLAGS\s*:=.*-ffp-contract=off", makefile, re.M)
    text, fused = isa.assembly("regress"), _contracted()
    fma = re.compile(r"\bv_(fma|fmac)_f64")
    for acc in (8, 16, 32):
        for vec in (1, 0):
            kernel = "regress_pass_kernelILb%dELi%dE" % (vec, acc)
            ours, theirs = isa.body(text, kernel), isa.body(fused, kernel)
            # eta's 16 and the block's acc accumulations (twice acc more in the branch of a block that mixes U and I)
            assert len(fma.findall(theirs)) - len(fma.findall(ours)) >= acc + 16, kernel
            assert len(re.findall(r"\bv_mul_f64", ours)) >= acc + 16 and len(re.findall(r"\bv_add_f64", ours)) >= acc + 16, kernel
