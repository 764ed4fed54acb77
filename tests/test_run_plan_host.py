"""prosstt_amd_run_plan (host helper of the C ABI, no device): the words the sampler's preparation kernel writes into the
cell records, against the rule written out in numpy (tests/run_rule.py)."""
import numpy as np
import pytest

from run_rule import loops, run_words

STRIPS = (8, 16, 32, 64)


def rows_of_runs(lengths, row_ids):
    return np.repeat(np.asarray(row_ids, np.int32), lengths)


def random_plan(seed, rows, target):
    """Runs of 1 to 200 cells, neighbouring runs on different rows, until `target` cells are passed."""
    rng = np.random.default_rng(seed)
    lengths, ids, prev = [], [], -1
    while sum(lengths) < target:
        lengths.append(int(rng.integers(1, 201)) if rng.random() < 0.5 else int(rng.integers(1, 12)))
        r = int(rng.integers(0, rows))
        ids.append(r if r != prev else (r + 1) % rows)
        prev = ids[-1]
    return rows_of_runs(lengths, ids)


@pytest.mark.parametrize("strip", STRIPS)
@pytest.mark.parametrize("seed,N", [(1, 2048), (2, 2011), (3, 777), (4, 65), (5, 7), (6, 1)])
def test_run_plan_matches_the_numpy_rule(strip, seed, N):
    from prosstt_amd import device
    roc = random_plan(seed, 23, N)[:N]            # (cut anywhere: N is no multiple of the strip in most cases)
    assert roc.size == N
    got = device.run_plan(roc, 23, strip)
    want = run_words(roc, 23, strip)
    assert got.dtype == np.uint32 and got.shape == (N + 4,)
    np.testing.assert_array_equal(got, want)
    # what the words say, spelled out once more: the lengths of a strip's runs add up to its cells, ...
    for first in range(0, N, strip):
        cells = min(strip, N - first)
        w = got[first:first + cells]
        assert int((w & 0xffff).sum()) == cells
        assert int(w[0] >> 16) == np.count_nonzero(w & 0xffff) and not (w[1:] >> 16).any()
    assert (got[N:] == 1).all()


@pytest.mark.parametrize("strip", STRIPS)
def test_runs_crossing_strip_boundaries_are_cut_there(strip):
    from prosstt_amd import device
    roc = rows_of_runs([strip + 3, 2 * strip, 1, strip - 1, 5], [4, 0, 4, 2, 3])
    got = device.run_plan(roc, 5, strip)
    np.testing.assert_array_equal(got, run_words(roc, 5, strip))
    assert got[0] == (1 << 16 | strip)                       # the strip's one run ends with the strip ...
    assert got[strip] == (2 << 16 | 3) and got[strip + 3] == strip - 3       # ... and goes on as a new run of the next one


@pytest.mark.parametrize("strip", STRIPS)
def test_rows_outside_the_tensor_are_clamped_as_in_the_kernels(strip):
    from prosstt_amd import device
    # -3 counts as row 0 and 12 as row 9: they join the runs beside them
    roc = np.array([0] * 5 + [-3] * 4 + [1] * 3 + [9] * 6 + [12] * 7 + [2 ** 31 - 1] * 2 + [-2 ** 31] + [0] * 3, np.int32)
    got = device.run_plan(roc, 10, strip)
    np.testing.assert_array_equal(got, run_words(roc, 10, strip))
    np.testing.assert_array_equal(got, device.run_plan(np.clip(roc, 0, 9), 10, strip))
    assert (got[0] & 0xffff) == min(9, strip)


def test_loop_choice_by_strip():
    roc = rows_of_runs([1, 70, 3, 8, 8, 8, 40, 2, 1, 1, 58], [11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11])
    assert loops(run_words(roc, 12, 64), 200, 64) == "RRRR"
    assert loops(run_words(roc, 12, 16), 200, 16) == "RRRRTTRRTRRRR"


def test_bad_arguments_are_refused():
    from prosstt_amd import device, _native
    roc = np.zeros(10, np.int32)
    for rows, strip in ((0, 8), (4, 0), (4, 129)):
        with pytest.raises(_native.NativeError):
            device.run_plan(roc, rows, strip)
    assert (device.run_plan(np.zeros(0, np.int32), 3, 8) == 1).all()
