"""The cases of tests/test_gpu_embed_paths.py, and the proof from the launch geometry that they reach all 18 kernel
instantiations of libprosstt_amd_embed.so where they can go wrong: for embed_matmul_kernel<NT, VEC> and
embed_rmatmul_kernel<NT, VEC> (NT = 1..4) a block with more than two steps of the software-pipelined loop, a multi-step
block whose last step is ragged, and more than one slab; for embed_moments_kernel<VEC> a full and a partial strip.

The geometry is restated here from prosstt_amd/csrc/embed/embed.hip (geometry) and prosstt_amd/csrc/abi_util.h
(strip_geometry, aligned) and pinned to the built library through prosstt_amd_embed_workspace_bytes: whoever changes
kTargetBlocks or a tile size finds out here that the cases no longer reach what they were chosen for."""
import ctypes
import os

import pytest

from prosstt_amd import _native

TARGET_BLOCKS, STEP, ROWS_MM, GENES_RM, STRIP, STRIP_MIN_ROWS = 1024, 32, 128, 256, 1024, 64

# (N, G) and the column views (pad, shift) of an (N, G + pad) tensor, base 4 * shift bytes past a 16-byte boundary
DEEP = (5542, 2999)
DEEP_VIEWS = [(1, 0), (3, 1), (3, 2)]
DEEP_LS = [32, 64, 96, 128]                    # one per NT
SMALL = [(1, 1), (2, 3), (33, 65), (129, 257), (257, 130)]
SMALL_VIEWS = [(0, 0), (3, 1)]
SMALL_LS = [1, 31, 33, 65, 95, 97, 127]        # l < lp for every NT: the col < l masks and sum_panels with l < lp

# (N, G, pad, shift): the matrices; with l: the product cases
MATRICES = [DEEP + v for v in DEEP_VIEWS] + [shape + v for shape in SMALL for v in SMALL_VIEWS]
PRODUCTS = ([DEEP + v + (l,) for v in DEEP_VIEWS for l in DEEP_LS]
            + [shape + v + (l,) for shape in SMALL for v in SMALL_VIEWS for l in SMALL_LS])


def cdiv(a, b):
    return -(-a // b)


def clamp(v, lo, hi):
    return max(lo, min(v, hi))


def pad256(b):
    return cdiv(b, 256) * 256


def geometry(N, G, l):
    """embed.hip's geometry(): lp, the moments' strips / row blocks / rows per block, matmul's parts and genes per
    part, rmatmul's row blocks and rows per block, and the three workspace sizes."""
    g = dict(lp=cdiv(l, 32) * 32, strips=cdiv(G, STRIP))
    g["m_rows"] = cdiv(N, clamp(TARGET_BLOCKS // g["strips"], 1, cdiv(N, STRIP_MIN_ROWS)))
    g["m_blocks"] = cdiv(N, g["m_rows"])
    chunks = cdiv(G, STEP)
    g["mm_genes"] = cdiv(chunks, clamp(TARGET_BLOCKS // cdiv(N, ROWS_MM), 1, chunks)) * STEP
    g["mm_parts"] = cdiv(G, g["mm_genes"])
    row_steps = cdiv(N, STEP)
    g["rm_rows"] = cdiv(row_steps, clamp(TARGET_BLOCKS // cdiv(G, GENES_RM), 1, row_steps)) * STEP
    g["rm_blocks"] = cdiv(N, g["rm_rows"])
    g["bytes"] = max(2 * pad256(g["m_blocks"] * G * 8), pad256(g["mm_parts"] * N * g["lp"] * 4),
                     pad256(g["rm_blocks"] * G * g["lp"] * 4))
    return g


def vectorized(kernel, N, G, pad, shift):
    """aligned(X, ld, elems) of the entry points: 16-byte loads (4 counts) in matmul and the moments, 8-byte loads (2) in
    rmatmul.  A one-row tensor has no row stride: device.CountMatrix passes ld = G."""
    elems = 2 if kernel == "rmatmul" else 4
    ld = G + pad if N > 1 else G
    return (4 * shift) % (4 * elems) == 0 and ld % elems == 0


def instantiation(kernel, N, G, pad, shift, l=None):
    """The kernel instantiation a call launches, as the test ids name it."""
    vec = "vec" if vectorized(kernel, N, G, pad, shift) else "scalar"
    return "moments-%s" % vec if kernel == "moments" else "%s-NT%d-%s" % (kernel, cdiv(l, 32), vec)


def blocks(kernel, N, G, l):
    """(slabs, [(steps, entries in the last step)] per slab) of a product's k loop: genes (matmul) or rows (rmatmul)."""
    g = geometry(N, G, l)
    total, per, n = (G, g["mm_genes"], g["mm_parts"]) if kernel == "matmul" else (N, g["rm_rows"], g["rm_blocks"])
    sizes = [min(per, total - b * per) for b in range(n)]
    return n, [(cdiv(k, STEP), k - (cdiv(k, STEP) - 1) * STEP) for k in sizes]


def case_id(kernel, N, G, pad, shift, l=None):
    return "%s-%dx%d-pad%d-shift%d" % (instantiation(kernel, N, G, pad, shift, l), N, G, pad, shift) + (
        "" if l is None else "-l%d" % l)


def test_the_issue_s_geometry_of_the_deep_shape():
    N, G = DEEP
    g = geometry(N, G, 64)
    assert (g["mm_parts"], g["mm_genes"]) == (19, 160) and blocks("matmul", N, G, 64)[1][-1] == (4, 23)
    assert (g["rm_blocks"], g["rm_rows"]) == (58, 96) and blocks("rmatmul", N, G, 64)[1][-1] == (3, 6)
    assert (g["m_blocks"], g["strips"], G - 2 * STRIP) == (87, 3, 951)
    assert [vectorized(k, N, G, *v) for v in DEEP_VIEWS for k in ("matmul", "moments", "rmatmul")] == [
        True, True, True, False, False, False, False, False, True]


def test_cases_reach_every_instantiation_where_it_can_go_wrong():
    deep, ragged, slabs, narrow = set(), set(), set(), set()
    for N, G, pad, shift, l in PRODUCTS:
        for kernel in ("matmul", "rmatmul"):
            inst = instantiation(kernel, N, G, pad, shift, l)
            n, steps = blocks(kernel, N, G, l)
            if any(s > 2 for s, _ in steps):
                deep.add(inst)
            if any(s > 1 and last < STEP for s, last in steps):
                ragged.add(inst)
            if n > 1:
                slabs.add(inst)
            if l % 32:
                narrow.add(inst.rsplit("-", 1)[0])
    every = {"%s-NT%d-%s" % (k, nt, v) for k in ("matmul", "rmatmul") for nt in (1, 2, 3, 4) for v in ("vec", "scalar")}
    assert len(every) == 16
    assert deep == every, sorted(every - deep)                 # more than two steps in a block
    assert ragged == every, sorted(every - ragged)             # a ragged last step of a multi-step block
    assert slabs == every, sorted(every - slabs)               # more than one slab for sum_panels
    assert narrow == {"%s-NT%d" % (k, nt) for k in ("matmul", "rmatmul") for nt in (1, 2, 3, 4)}     # l < lp
    full, partial = set(), set()
    for N, G, pad, shift in MATRICES:
        inst = instantiation("moments", N, G, pad, shift)
        if G >= STRIP:
            full.add(inst)
        if G % STRIP:
            partial.add(inst)
        if geometry(N, G, 1)["m_blocks"] > 1:
            slabs.add(inst)
    both = {"moments-vec", "moments-scalar"}
    assert full == both and partial == both and both <= slabs


def test_restated_geometry_is_the_library_s():
    if not os.path.exists(_native.LIBRARIES["embed"].path):
        pytest.skip("libprosstt_amd_embed.so is not built")
    lib = ctypes.CDLL(_native.LIBRARIES["embed"].path)
    query = lib.prosstt_amd_embed_workspace_bytes
    query.restype = ctypes.c_int
    query.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64)]
    shapes = {(N, G, l) for N, G, _, _, l in PRODUCTS} | {(N, G, 1) for N, G, _, _ in MATRICES}
    shapes |= {(2048, 64, 64), (4096, 128, 128), (50000, 20000, 60), (110000, 20000, 8)}
    for N, G, l in sorted(shapes):
        need = ctypes.c_uint64(0)
        assert query(N, G, l, ctypes.byref(need)) == 0
        assert need.value == geometry(N, G, l)["bytes"], (N, G, l)
