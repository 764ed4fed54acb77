"""The cases of tests/test_gpu_factors.py and tests/test_gpu_factors_guard_bands.py, and the proof from the launch geometry
that they reach the launches they name, without a GPU: both loads of the tile (16-byte pieces under an aligned view, 4-byte
pieces under the others), the ragged last tile under either, a last block of cells that is not full, several blocks of genes,
every split with a slice of one kind and a mixed one, and the instantiation that adds Q (every call launches it).

The geometry is restated here from prosstt_amd/csrc/factors/factors.hip (gene_blocking, geometry, the entry point's choice of
split and of <VEC>) and pinned to the built library through its two queries: whoever changes the tile, the cells of a block or
the blocking finds out here that the cases no longer reach what they were chosen for."""
import ctypes


import test_gpu_factors as T
import test_gpu_factors_guard_bands as B

from prosstt_amd import _native, factors

TILE, CELLS = 32, 256


def cdiv(a, b):
    return -(-a // b)


def aligned(N, G, layout):
    """aligned(X, ld, 4) of the entry point for the views of ``test_gpu_factors._view``: the base on 16 bytes and a row stride
    that is a multiple of 4.  A one-row tensor has no row stride: device.CountMatrix passes ld = G."""
    ld = {"plain": G, "wide": G + 1, "shifted": G + 3, "padded": cdiv(G, 4) * 4 + 4}[layout] if N > 1 else G
    return layout != "shifted" and ld % 4 == 0


def launch(N, G, p, layout, split, per):
    """What a call launches: the instantiation of the sums kernel, and what its blocks meet."""
    sums = p + p * (p + 1) // 2
    acc = split or (16 if sums <= 48 else 32)
    per, blocks = factors.gene_blocks(N, G, per)
    vec = aligned(N, G, layout)
    last = G - (blocks - 1) * per                                  # genes of the last block
    slices = [(a0, min(acc, sums - a0)) for a0 in range(0, sums, acc)]
    kinds = {"mixed" if a0 < p < a0 + n else ("U" if a0 < p else "I") for a0, n in slices}
    return dict(kernel=(vec, acc), gene_blocks=blocks, cell_blocks=cdiv(N, CELLS), ragged_cells=N % CELLS != 0,
                whole_tiles=(per if blocks > 1 else last) >= TILE, ragged_tile=last % TILE != 0, several_tiles=min(per, G) > TILE,
                kinds=kinds, slices=len(slices))


def test_the_bit_exact_cases_reach_every_instantiation_where_it_can_go_wrong():
    reached = [launch(N, G, p, layout, split, per) for N, G, p, layout, split, per, _ in T.CASES]
    every = {(vec, acc) for vec in (True, False) for acc in (8, 16, 32)}
    assert {r["kernel"] for r in reached} == every
    for what in ("whole_tiles", "ragged_tile", "ragged_cells", "several_tiles"):
        assert {r["kernel"] for r in reached if r[what]} == every, what
    assert {r["kernel"] for r in reached if r["gene_blocks"] > 1} == every
    assert {r["kernel"] for r in reached if r["cell_blocks"] > 1} == every
    assert {r["kernel"] for r in reached if r["slices"] > 1} == every
    # a slice of sums of U alone, of I alone, and one that mixes them (the two-table branch), for every ACC
    # (p <= 16: a slice of 32 sums always reaches past the sums of U)
    for kind, accs in (("U", {8, 16}), ("I", {8, 16, 32}), ("mixed", {8, 16, 32})):
        assert {r["kernel"][1] for r in reached if kind in r["kinds"]} == accs, kind
    # the library's own choice of the split: 16 up to 48 sums, 32 above
    own = {(launch(N, G, p, layout, 0, per)["kernel"][1], p) for N, G, p, layout, split, per, _ in T.CASES if split == 0}
    assert {acc for acc, _ in own} == {16, 32} and all((acc == 16) == (p <= 8) for acc, p in own)
    # the 16-byte loads with a whole tile and the 4-byte loads of the ragged one in ONE block
    assert any(r["kernel"][0] and r["whole_tiles"] and r["ragged_tile"] for r in reached)
    # the smallest problem, and a full block of cells exactly
    assert any(N == 1 for N, *_ in T.CASES) and any(G == 1 for _, G, *_ in T.CASES) and any(N == CELLS for N, *_ in T.CASES)


def test_the_other_gpu_cases_reach_what_they_name():
    # the real-valued sums: both loads, the library's own blocking with several blocks, one block for all genes
    real = [launch(257, 513, 7, layout, 0, per) for layout, per in (("plain", 0), ("shifted", 0), ("padded", 4 * TILE), ("plain", 544))]
    assert [r["kernel"] for r in real] == [(False, 16), (False, 16), (True, 16), (False, 16)]
    assert [r["gene_blocks"] for r in real] == [5, 5, 5, 1] and all(r["cell_blocks"] == 2 and r["ragged_tile"] for r in real)
    # equal bits: every split, and a cell alone is one block of one lane with the blocking of the whole
    assert {launch(257, 513, 7, "plain", split, 0)["kernel"][1] for split in (0, 8, 16, 32)} == {8, 16, 32}
    assert launch(1, 513, 7, "plain", 0, 128)["gene_blocks"] == launch(257, 513, 7, "plain", 0, 128)["gene_blocks"] == 5
    # the halves and the loop at 300 x 257, k = 3: p = 4, 14 sums in one mixed slice, three blocks of genes
    half = launch(300, 257, 4, "plain", 0, 0)
    assert half["kernel"] == (False, 16) and half["kinds"] == {"mixed"} and half["gene_blocks"] == 3 and half["ragged_tile"]
    # the guard bands: 259 x 1025 in both alignments, every split, the library's blocking and a tile per block
    shifted = [launch(259, 1025, 7, "shifted", split, per) for split, per in ((0, 0), (8, 32), (16, 0), (32, 32))]
    assert {r["kernel"] for r in shifted} == {(False, 8), (False, 16), (False, 32)}
    assert [r["gene_blocks"] for r in shifted] == [9, 33, 9, 33] and all(r["ragged_cells"] and r["ragged_tile"] for r in shifted)
    padded = [launch(259, 1025, 7, "padded", split, per) for split, per in ((0, 0), (8, 32), (16, 0), (32, 32))]
    assert {r["kernel"] for r in padded} == {(True, 8), (True, 16), (True, 32)} and all(r["whole_tiles"] for r in padded)
    assert callable(B.calls_factors) and callable(B.small_factors)
    small = launch(1, 1, 1, "plain", 0, 0)
    assert small["gene_blocks"] == small["cell_blocks"] == small["slices"] == 1 and not small["whole_tiles"]


def test_restated_geometry_is_the_library_s():
    lib = _native.load("factors")                                  # (a missing library fails here, it does not skip)
    shapes = {(N, G, p, per) for N, G, p, _, _, per, _ in T.CASES} | {(257, 513, 7, 0), (257, 513, 7, 544), (259, 1025, 7, 32),
                                                                       (300, 257, 4, 0), (50000, 20000, 16, 0), (50000, 2000, 8, 0)}
    need, own = ctypes.c_uint64(0), ctypes.c_int64(0)
    for N, G, p, per in sorted(shapes):
        genes, blocks = factors.gene_blocks(N, G, per)
        assert lib.prosstt_amd_factors_gene_blocking(N, G, ctypes.byref(own)) == 0
        assert own.value == factors.gene_blocks(N, G)[0]
        sums = p + p * (p + 1) // 2
        want = cdiv(blocks * N * (sums + 1) * 8, 256) * 256 + cdiv(blocks * N * 4, 256) * 256
        assert lib.prosstt_amd_factors_workspace_bytes(N, G, p, per, ctypes.byref(need)) == 0 and need.value == want, (N, G, p, per)
