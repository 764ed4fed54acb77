"""
The strip plan of the stream sampler (k3::strip_plan, exported as prosstt_amd_strip_plan) against its statement in numpy
(tests/strip_rule.py), and the properties the three kernels and the workspace lean on.  No device work.
"""
import itertools

import numpy as np
import pytest

from run_rule import run_words
from strip_rule import plan_run_words, strip_plan, strips_of_blocks

NS = [1, 63, 64, 613, 4097, 50000, 200000]
GS = [8, 256, 520, 20000]
RS = [1, 2, 1280]
# (strip_cells, taper): the rule alone, the two hooks of the tests and tools alone and together
HOOKS = [(0, 0), (64, 0), (16, 0), (0, 1), (64, 1), (32, 3), (64, 640), (128, 1), (128, 0)]


def library_plan(N, G, R, strip_cells, taper):
    from prosstt_amd import device
    return device.strip_plan(N, G, R, strip_cells=strip_cells, taper=taper)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("N", NS)
def test_plan_is_the_rule_and_covers_the_cells_once(N, G):
    for R, (strip_cells, taper) in itertools.product(RS, HOOKS):
        classes, tiles, blocks = library_plan(N, G, R, strip_cells, taper)
        want, want_tiles, want_blocks = strip_plan(N, G, R, strip_cells, taper)
        np.testing.assert_array_equal(classes, want)
        assert (tiles, blocks) == (want_tiles, want_blocks) and tiles == -(-G // 256)
        first, length, first_block = classes.T
        # the classes cover [0, N) once, in order; boundaries are multiples of 64; lengths divide 64 and halve
        assert 1 <= len(classes) <= 4 and first[0] == 0 and first_block[0] == 0
        assert np.all(np.diff(first) > 0) and first[-1] < N and np.all(first % 64 == 0)
        assert np.all(64 % length[1:] == 0) and np.all(length >= 8) and np.all(length[1:] * 2 == length[:-1])
        # 128-cell strips: only as the bulk of a graded plan whose length nobody forced, and then in whole strips
        assert 64 % length[0] == 0 or (length[0] == 128 and len(classes) > 1 and strip_cells in (0, 128) and first[1] % 128 == 0)
        if strip_cells:
            assert length[0] == strip_cells or (strip_cells == 128 and len(classes) == 1 and length[0] == 64)
        # without the taper hook a launch of fewer than 4 R blocks is one uniform class: the geometry of every earlier test
        uniform_blocks = -(-(-(-N // min(64, int(length[0])))) // 4) * tiles
        if not taper and uniform_blocks < 4 * R:
            assert len(classes) == 1
        if strip_cells in (0, 128) and not taper and uniform_blocks >= 4 * R and length[0] >= 16 and N >= 512:
            assert len(classes) > 1
        if len(classes) == 1:
            assert blocks == uniform_blocks
        # block -> (tile, strip) is a bijection onto the strips: the strips of a tile, in cell order, follow each other
        # from cell 0 to N without a gap; the regions are as many as the workspace is sized for (4 per block)
        regions = strips_of_blocks(classes, tiles, blocks, N)
        assert regions.shape[0] == 4 * blocks
        live = regions[regions[:, 2] > 0]
        live = live[np.lexsort((live[:, 1], live[:, 0]))].reshape(tiles, -1, 3)
        assert np.all(live[:, :, 0] == np.arange(tiles)[:, None]) and np.all(live[:, 0, 1] == 0)
        assert np.all(live[:, 1:, 1] == live[:, :-1, 1] + live[:, :-1, 2]) and np.all(live[:, -1, 1] + live[:, -1, 2] == N)
        assert np.all(regions.reshape(blocks, 4, 3)[:, 0, 2] > 0)
        assert np.all(regions[:, 0] < tiles)


def test_the_graded_plan_of_the_headline_shape():
    """50 000 x 20 000 on 256 compute units (1 280 resident blocks): 85 % of the cells in 128-cell strips, then about one
    residency each of 64-, 32- and 16-cell strips."""
    classes, tiles, blocks = library_plan(50000, 20000, 1280, 0, 0)
    assert tiles == 79
    np.testing.assert_array_equal(classes[:, :2], [[0, 128], [42752, 64], [46912, 32], [48960, 16]])
    per_class = np.diff(np.r_[classes[:, 2], blocks])
    assert per_class[0] == 84 * 79 and np.all(np.abs(per_class[1:] - 1280) < 130)


def test_the_plan_of_the_taper_test():
    """N = 613, G = 520, bulk 64, one resident block: 384 cells in 64-cell strips (two groups, the second half empty),
    64 cells each in strips of 32 and 16, and 101 cells in strips of 8, the last of 5 cells."""
    classes, tiles, blocks = library_plan(613, 520, 1280, 64, 1)
    np.testing.assert_array_equal(classes, [[0, 64, 0], [384, 32, 6], [448, 16, 9], [512, 8, 12]])
    assert (tiles, blocks) == (3, 24)
    regions = strips_of_blocks(classes, tiles, blocks, 613)
    np.testing.assert_array_equal(regions[4:8], [[0, 256, 64], [0, 320, 64], [0, 384, 0], [0, 448, 0]])
    assert regions[regions[:, 2] > 0][:, 2].min() == 5


@pytest.mark.parametrize("N", [613, 4097])
def test_run_words_of_a_graded_plan_are_the_rule_class_by_class(N):
    from prosstt_amd import device
    rng = np.random.default_rng(N)
    rows = 9
    roc = np.repeat(rng.integers(0, rows, N), rng.integers(1, 40, N))[:N].astype(np.int32)
    classes, _, _ = library_plan(N, 520, 1280, 64, 1)
    assert len(classes) == 4
    words = plan_run_words(roc, rows, classes)
    ends = np.r_[classes[1:, 0], N]
    for (first, length, _), end in zip(classes.tolist(), ends.tolist()):
        # a class starts on a multiple of its strip length, so the library's words for that length agree inside the class
        np.testing.assert_array_equal(words[first:end], device.run_plan(roc, rows, length)[first:end])
    np.testing.assert_array_equal(words[N:], 1)
    one, _, _ = library_plan(N, 520, 1280, 64, 0)
    np.testing.assert_array_equal(plan_run_words(roc, rows, one), run_words(roc, rows, 64))


def test_the_plan_entry_points_are_declared_listed_and_exported():
    """include/prosstt_amd_plan.h, _native.SAMPLER_LATER and the built sampler library name the same symbols, and none of
    them is one of prosstt_amd.h's."""
    import os
    import re
    from conftest import ROOT
    from prosstt_amd import _native
    header_name, symbols = _native.SAMPLER_LATER
    declared = re.findall(r"\b(prosstt_amd_\w+)\s*\(", open(os.path.join(ROOT, "include", header_name)).read())
    assert sorted(declared) == sorted(symbols) == ["prosstt_amd_last_strip_plan", "prosstt_amd_strip_plan"]
    assert not set(symbols) & set(_native.LIBRARIES["sampler"].symbols)
    lib = _native.load()
    for symbol, (restype, argtypes) in symbols.items():
        assert getattr(lib, symbol).argtypes == argtypes
