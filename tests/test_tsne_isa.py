"""Properties of the t-SNE kernels' gfx950 code object (prosstt_amd/csrc/tsne/tsne.hip), read from the ISA hipcc writes with
the library's own flags (cross-compiles without a GPU): no kernel uses scratch, there is no atomic of any kind, and the pair
kernel takes the hardware reciprocal instead of a division."""
import re

import pytest

import isa

KERNELS = (["tsne_affinities_kernel", "tsne_fold_kernel", "tsne_zsum_kernel"] +
           ["tsne_pair_kernelILi%dELb%dE" % (c, a) for c in (2, 3) for a in (0, 1)] +
           ["tsne_row_kernelILi%dELb%dE" % (c, s) for c in (2, 3) for s in (0, 1)] +
           ["tsne_objective_kernelILi%dE" % c for c in (2, 3)])


def test_every_kernel_is_listed():
    text = isa.assembly("tsne")
    names = set(re.findall(r"\.name:\s+(_Z\S*tsne_\S*_kernel\S*)", text))
    names = {n for n in names if not n.endswith(".kd")}
    assert len(names) == len(KERNELS), sorted(names)
    for kernel in KERNELS:
        assert any(kernel in n for n in names), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch(kernel):
    text = isa.assembly("tsne")
    assert isa.meta(text, kernel, "private_segment_fixed_size") == 0
    assert isa.meta(text, kernel, "vgpr_spill_count") == 0
    assert isa.meta(text, kernel, "sgpr_spill_count") == 0


def test_no_atomics():
    text = isa.assembly("tsne")
    found = sorted(set(m.group(0) for m in isa.FLOAT_ATOMIC.finditer(text)))
    assert not found, found
    # there is no atomic at all, in global memory or in LDS: the status bytes are plain stores
    assert not isa.global_atomics(text)
    assert not isa.lds_atomics(text)


@pytest.mark.parametrize("kernel", [k for k in KERNELS if "pair" in k])
def test_the_pair_kernel_takes_the_hardware_reciprocal(kernel):
    body = isa.body(isa.assembly("tsne"), kernel)
    assert "v_rcp_f32" in body
    assert "v_div_scale_f32" not in body and "v_div_fmas_f32" not in body
    assert "ds_read" in body or "ds_load" in body                 # the columns come through LDS
