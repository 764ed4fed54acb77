"""
-m gpu: the two strip loops of the stream kernel (k3_stream.h: the run loop, which loads a mean segment once per run of
cells on one row, and the loop that loads one per cell), count for count against oracle/nb_model.c.

Every case is about 200 cells x 520 genes on a mean tensor of 12 rows (its last row among the used ones), presented with
cell_index, and runs with strips of 64 and of 16 cells (PROSSTT_AMD_STRIP_CELLS: a problem this small gets 8-cell strips
otherwise).  Each also reads back the run words the preparation kernel wrote, compares them with the rule in numpy
(tests/run_rule.py), and names the loop every strip takes by them, so that no case passes without running its loop.
"""
import numpy as np
import pytest

from run_rule import loops, run_words

pytestmark = pytest.mark.gpu

ROWS, N = 12, 200
B_LENGTHS = [1, 70, 3, 8, 8, 8, 40, 2, 1, 1, 58]
B_ROWS = [11, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11]
# a run of one cell on a strip's last cell (cells 63 and 191 of 64-cell strips, cell 15 of a 16-cell strip)
TAIL_LENGTHS = [15, 48, 65, 63, 1, 8]
TAIL_ROWS = [3, 11, 0, 7, 2, 11]


@pytest.fixture(scope="module")
def ctx():
    from prosstt_amd import device
    return device.get_context()


def inputs(G, seed=5):
    rng = np.random.default_rng(seed)
    base = np.exp(rng.normal(0.8, 1.0, G))
    means = (np.exp(rng.normal(0.0, 0.6, (ROWS, G)).cumsum(axis=0) * 0.15) * base).astype(np.float32)
    means[:, rng.random(G) < 0.05] *= 200.0                      # some genes of the gamma-Poisson class
    scaling = np.exp(rng.normal(0, 0.7, N))
    alpha = np.exp(rng.normal(np.log(0.2), np.log(1.5), G))
    beta = np.exp(rng.normal(np.log(1.0), np.log(1.5), G)) + 1
    cell_index = rng.permutation(10 * N)[:N].astype(np.int64) + (1 << 33)
    return means, scaling, alpha, beta, cell_index


def plan(name):
    if name == "one_row":
        return np.full(N, 11, np.int32)
    if name == "b":
        return np.repeat(np.asarray(B_ROWS, np.int32), B_LENGTHS)
    if name == "tail":
        return np.repeat(np.asarray(TAIL_ROWS, np.int32), TAIL_LENGTHS)
    assert name == "alternating"
    return np.asarray([(11, 0, 5)[i % 3] for i in range(N)], np.int32)


# the loop of every strip ('R' the run loop, 'T' the loop that loads per cell), by strip length
LOOPS = {
    # (a) one row: one run per strip; the last strip of 64-cell strips has 8 cells, which is runs * 8 = cells
    "one_row": {64: "RRRR", 16: "R" * 13},
    # (b) 16-cell strips 0 and 6 have two runs (runs * 8 = cells), strips 4, 5 and 8 have three and five (above it)
    "b": {64: "RRRR", 16: "RRRRTTRRTRRRR"},
    # (c) neighbours always on different rows
    "alternating": {64: "TTTT", 16: "T" * 13},
    "tail": {64: "RRRR", 16: "RRRRRRRRRRRRR"},
}

_want = {}


def model(key, means, roc, scaling, alpha, beta, seed, cell_index):
    """The model's counts of a case, computed once for both strip lengths."""
    if key not in _want:
        from oracle import nb_model
        _want[key] = nb_model.sample_counts(means, roc, scaling, alpha, beta, seed, 0, cell_index)
        _want[key].setflags(write=False)
    return _want[key]


def run_and_compare(ctx, monkeypatch, name, strip, G, seed, ld=None, **kw):
    import torch
    monkeypatch.setenv("PROSSTT_AMD_STRIP_CELLS", str(strip))
    means, scaling, alpha, beta, cell_index = inputs(G)
    roc = plan(name)
    assert roc.size == N and roc.max() == ROWS - 1
    out = None
    if ld is not None:
        full = torch.full((N, ld), -7, dtype=torch.int32, device="cuda")
        out = full[:, :G]
    got = ctx.sample_counts(means, roc, scaling, alpha, beta, seed=seed, cell_index=cell_index, out=out,
                            check_domain=kw.pop("check_domain", False), **kw)
    words, strip_used = ctx.last_run_plan()
    assert strip_used == strip
    np.testing.assert_array_equal(words, run_words(roc, ROWS, strip))
    assert loops(words, N, strip) == LOOPS[name][strip]
    want = model((name, G, seed), means, roc, scaling, alpha, beta, seed, cell_index)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert want.max() > 4
    if ld is not None:
        assert bool((full[:, G:] == -7).all())            # the padding behind G is not written
    return got


@pytest.mark.parametrize("strip", [64, 16])
@pytest.mark.parametrize("name", ["one_row", "b", "alternating", "tail"])
def test_counts_by_loop(ctx, monkeypatch, name, strip):
    """(a), (b), (c) and a run of one cell at the end of a strip: G = 520, three gene tiles, the last one of 8 genes."""
    run_and_compare(ctx, monkeypatch, name, strip, 520, seed=1234 + len(name))


@pytest.mark.parametrize("strip", [64, 16])
@pytest.mark.parametrize("G,ld", [(521, 521), (521, 528), (520, 528)])
def test_counts_of_the_scalar_kernels_and_padded_rows(ctx, monkeypatch, strip, G, ld):
    """(d): case (b) with G = 521 (G % 4 != 0: the instantiations that load and store element by element) and with rows
    of `out` longer than G."""
    run_and_compare(ctx, monkeypatch, "b", strip, G, seed=77, ld=ld)


@pytest.mark.parametrize("strip", [64, 16])
def test_deferred_domain_verdict(ctx, monkeypatch, strip):
    """(e): case (b) with check_domain="deferred".  A row of the mean tensor with a zero in it that no cell uses leaves
    the verdict clean; used by a cell it raises, as it did before there were two loops -- and the counts are the
    model's either way."""
    monkeypatch.setenv("PROSSTT_AMD_STRIP_CELLS", str(strip))
    try:
        ctx.domain_status()                               # (whatever an earlier deferred call on this ctx left is not this test's)
    except Exception:
        pass
    G = 520
    means, scaling, alpha, beta, cell_index = inputs(G)
    means[9, 100] = 0.0                                   # row 9: no run of case (b) is on it
    from oracle import nb_model
    for used in (False, True):
        roc = plan("b")
        if used:
            roc[90:98] = 9                                # the run of cells 90 .. 97 moves to the bad row (same runs)
        got = ctx.sample_counts(means, roc, scaling, alpha, beta, seed=31, cell_index=cell_index, check_domain="deferred")
        words, strip_used = ctx.last_run_plan()
        assert strip_used == strip
        np.testing.assert_array_equal(words, run_words(roc, ROWS, strip))
        assert loops(words, N, strip) == LOOPS["b"][strip]
        np.testing.assert_array_equal(got.cpu().numpy(), nb_model.sample_counts(means, roc, scaling, alpha, beta, 31, 0, cell_index))
        if used:
            with pytest.raises(ValueError):
                ctx.domain_status()
        else:
            ctx.domain_status()


@pytest.mark.parametrize("strip", [8, 16, 32, 64])
def test_run_words_of_the_preparation_kernel(ctx, monkeypatch, strip):
    """The words of a longer, random plan at every strip length (1337 cells: the last strip and the last wave of the
    preparation kernel are partial), and the counts behind them."""
    from oracle import nb_model
    monkeypatch.setenv("PROSSTT_AMD_STRIP_CELLS", str(strip))
    rng = np.random.default_rng(strip)
    n, G = 1337, 8
    lengths = np.where(rng.random(400) < 0.4, rng.integers(1, 201, 400), rng.integers(1, 6, 400))
    ids = np.cumsum(rng.integers(1, ROWS, 400)) % ROWS            # neighbouring runs on different rows
    roc = np.repeat(ids.astype(np.int32), lengths)[:n]
    assert roc.size == n
    means = np.exp(rng.normal(0.5, 1.0, (ROWS, G))).astype(np.float32)
    scaling, alpha, beta = np.exp(rng.normal(0, 0.5, n)), np.full(G, 0.2), np.full(G, 2.0)
    got = ctx.sample_counts(means, roc, scaling, alpha, beta, seed=strip, check_domain=False)
    words, strip_used = ctx.last_run_plan()
    assert strip_used == strip
    want_words = run_words(roc, ROWS, strip)
    np.testing.assert_array_equal(words, want_words)
    assert len(set(loops(words, n, strip))) == 2                # strips of both kinds
    np.testing.assert_array_equal(got.cpu().numpy(), nb_model.sample_counts(means, roc, scaling, alpha, beta, strip))
