"""Properties of the factors kernels' gfx950 code object (prosstt_amd/csrc/factors/factors.hip), read from the ISA hipcc writes
with the library's own flags (cross-compiles without a GPU), on tests/isa.py as tests/test_regress_isa.py uses it: every
kernel is there, none uses scratch or spills a register, there is no floating-point atomic, only the aligned kernels read the
matrix with 16-byte loads, every instantiation stays in its occupancy class, and the products and sums of the definition are
not contracted.

On contraction (tests/test_regress_isa.py has the argument in full).  Binary64 division and HIP's exp are sequences of
v_fma_f64, so a pass that divides and takes an exponential cannot be free of the instruction; what the definition asks is that
none of ITS products and sums is fused.  A sums kernel calls exp once and divides twice (w and u) whatever ACC is, so the count
of fused operations is the SAME in the six sums kernels, while the separate multiplies and adds grow by exactly 3 per sum (one
in the loop of a block of one kind, two in that of a mixed block), and the multiplies by one more per eight sums: the product
of two loadings that a thread forms for the tile's table of factors, for ACC / 8 genes of a tile.  One contracted accumulation
makes the count depend on ACC; a contracted eta adds 16 and leaves the budget of one exp and two divisions."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import isa

SPLITS = (8, 16, 32, 0)                 # ACC of an instantiation; 0 adds Q and used
KERNELS = ["factors_pass_kernelILb%dELi%dE" % (vec, acc) for acc in SPLITS for vec in (1, 0)] + ["factors_finish_kernel"]
TILE = 256 * 33 * 4                     # 256 cells x 32 genes at a row stride of 33 words


def test_every_kernel_is_listed():
    text = isa.assembly("factors")
    names = set(re.findall(r"\.name:\s+(_Z\S*factors_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spill(kernel):
    text = isa.assembly("factors")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_floating_point_atomic_and_no_atomic_but_the_status_word():
    text = isa.assembly("factors")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    assert set(isa.global_atomics(text)) <= {"global_atomic_or", "flat_atomic_or"}
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("acc", SPLITS)
def test_only_the_aligned_kernel_reads_rows_with_16_byte_loads_and_both_transpose_through_lds(acc):
    text = isa.assembly("factors")
    aligned, plain = (isa.body(text, "factors_pass_kernelILb%dELi%dE" % (vec, acc)) for vec in (1, 0))
    assert "global_load_dwordx4" in aligned and "global_load_dwordx4" not in plain
    # the odd row stride: no 16-byte store into the tile, in either kernel; the ragged tile's 4-byte loads are in both
    for body in (aligned, plain):
        assert "ds_write_b128" not in body and "ds_write_b32" in body and "global_load_dword " in body.replace("\t", " ")
    # the tile, beside the genes' use, parameters, loadings and the factors of the block's sums
    tables = 32 * (4 + 3 * 8 + 16 * 8 + 2 * 8 * max(acc, 1))
    for vec in (1, 0):
        lds = isa.meta(text, "factors_pass_kernelILb%dELi%dE" % (vec, acc), "group_segment_fixed_size")
        assert TILE < lds <= TILE + tables, (vec, acc, lds)


def test_the_occupancy_class_of_every_instantiation():
    """512 vector registers per SIMD lane: at most 168 per wave keep three waves resident, at most 256 two; 160 KiB of LDS per
    CU: at most 53 KiB per block keep three blocks (of four waves, one per SIMD) resident, at most 80 KiB two.  The smaller of
    the two is the class.  A block of 256 threads is one wave per SIMD, so a kernel may take up to 512 registers without a
    spill: the first build of ACC = 32 took 274 and fell to one wave, which the bound of 256 is there to catch.  Beside the
    class, the counts of DESIGN section 35's table are held with a margin of 8 registers, so that a build that drifts towards
    the next class is seen before it gets there (168 and 256 stay the hard limits)."""
    text = isa.assembly("factors")
    KiB = 1024
    table = {(1, 8): 167, (0, 8): 156, (1, 16): 210, (0, 16): 198, (1, 32): 248, (0, 32): 236, (1, 0): 168, (0, 0): 144}
    for vec in (1, 0):
        for acc, registers, lds in ((8, 168, 53 * KiB), (0, 168, 53 * KiB), (16, 256, 53 * KiB), (32, 256, 80 * KiB)):
            kernel = "factors_pass_kernelILb%dELi%dE" % (vec, acc)
            count = isa.meta(text, kernel, "vgpr_count")
            assert count <= min(registers, table[vec, acc] + 8), (kernel, count)
            assert isa.meta(text, kernel, "group_segment_fixed_size") <= lds, kernel
            # the tile, the loadings and the two factor tables, and at most 1 KiB of the genes' use, parameters and padding
            assert isa.meta(text, kernel, "group_segment_fixed_size") <= 33792 + 4096 + 512 * max(acc, 1) + 1024, kernel


FUSED = re.compile(r"\bv_(fma|fmac)_f64")


def test_the_fused_operations_of_a_sums_kernel_are_those_of_exp_and_two_divisions():
    text = isa.assembly("factors")
    counts = {}
    for acc in (8, 16, 32):
        for vec in (1, 0):
            body = isa.body(text, "factors_pass_kernelILb%dELi%dE" % (vec, acc))
            assert len(re.findall(r"\bv_div_fmas_f64", body)) == 2, (vec, acc)          # w and u, nothing else divides
            # (acc / 8 more products where the tile's tables are formed: a thread multiplies the two loadings of its sum for
            # 32 acc / 256 genes of the tile, in a loop that is unrolled)
            counts[vec, acc] = (len(FUSED.findall(body)), len(re.findall(r"\bv_mul_f64", body)) - 3 * acc - acc // 8,
                                len(re.findall(r"\bv_add_f64", body)) - 3 * acc)
    assert len(set(counts.values())) == 1, counts                # nothing depends on ACC or on the loads
    fused, multiplies, adds = counts[1, 8]
    assert 0 < fused <= 2 * 8 + 16, counts
    assert multiplies >= 16 and adds >= 16, counts               # eta's sixteen products and sums are separate instructions


def _contracted():
    """The assembly of the library compiled with contraction allowed (EXTRA comes after the makefile's own flags)."""
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_factors_contract_")
    try:
        subprocess.check_call(["make", "-C", os.path.join(isa.ROOT, "prosstt_amd", "csrc"), "isa-factors", "ISA_DIR=" + tmp,
                               "EXTRA=-ffp-contract=fast"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(os.path.join(tmp, "factors.s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def test_the_products_and_sums_of_the_definition_are_not_contracted():
    makefile = open(os.path.join(isa.ROOT, "prosstt_amd", "csrc", "Makefile")).read()
    assert re.search(r"^FLAGS\s*:=.*-ffp-contract=off", makefile, re.M)
    text, fused = isa.assembly("factors"), _contracted()
    for acc in (8, 16, 32):
        for vec in (1, 0):
            kernel = "factors_pass_kernelILb%dELi%dE" % (vec, acc)
            ours, theirs = isa.body(text, kernel), isa.body(fused, kernel)
            # eta's 16 and the block's acc accumulations (twice acc more in the branch of a block that mixes U and I)
            assert len(FUSED.findall(theirs)) - len(FUSED.findall(ours)) >= acc + 16, kernel
            assert len(re.findall(r"\bv_mul_f64", ours)) >= acc + 16 and len(re.findall(r"\bv_add_f64", ours)) >= acc + 16, kernel
