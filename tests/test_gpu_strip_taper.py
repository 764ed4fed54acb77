"""
-m gpu: the graded strip plan of the stream sampler (k3::strip_plan: long strips first, ever shorter ones behind them),
count for count against the same call under the uniform geometry and against oracle/nb_model.c.

613 cells with PROSSTT_AMD_STRIP_CELLS=64 and PROSSTT_AMD_STRIP_TAPER=1: 384 cells in 64-cell strips (the second group of
four half empty), 64 cells each in strips of 32 and 16, 101 cells in strips of 8, the last of 5 cells -- and the same with a
bulk of 128-cell strips, which is what a large launch gets by the rule (384 cells, then 64, 32 and 16).  G = 520 is three
gene tiles, the last 8 genes wide, on the 16-byte path; G = 522 takes the scalar path.  The first gene tile lists more
gamma-Poisson samples per region than the 32 a region keeps densely (they travel through the segments; fewer than one in
32, which is what the list of a 128-cell region holds), half the genes of
the second are of that class (more than one sample in 16: its regions overflow and K3h redoes them from the plan), and
walks end far past term 20 -- so every place where K3h maps a region back to cells runs, in every class of the plan.

What last_list() is compared on: the samples of the gamma-Poisson class outside the overflowing tile, which must be all of
them under either geometry.  The walks a strip hands over unfinished are listed too, and WHICH walks are unfinished when
a strip ends depends on where strips end, so the whole lists of two geometries differ by construction; those entries are
only required to be samples of the inversion class.
"""
import numpy as np
import pytest

from run_rule import run_words
from strip_rule import plan_loops, plan_run_words, strip_plan

pytestmark = pytest.mark.gpu

ROWS, N, SEED = 12, 613, 2024
# by bulk length: 64 as above; 128 (what a large launch gets by the rule: a strip is two waves of the preparation kernel)
PLAN = {64: [[0, 64, 0], [384, 32, 6], [448, 16, 9], [512, 8, 12]], 128: [[0, 128, 0], [384, 64, 3], [448, 32, 6], [512, 16, 9]]}
STRIPS = {64: (6, 2, 4, 13), 128: (3, 1, 2, 7)}


@pytest.fixture(scope="module")
def ctx():
    from prosstt_amd import device
    return device.get_context()


def inputs(G):
    rng = np.random.default_rng(G)
    base = np.exp(rng.normal(0.8, 1.0, G))
    means = (np.exp(rng.normal(0.0, 0.6, (ROWS, G)).cumsum(axis=0) * 0.15) * base).astype(np.float32)
    means[:, rng.choice(256, 6, replace=False)] *= 200.0        # tile 0: beyond a region's dense entries, under 1 in 32
    means[:, 256:512][:, rng.random(256) < 0.5] *= 200.0        # tile 1: its regions overflow
    means[:, 5] = 30.0                                          # long walks of the inversion class (alpha, beta below)
    scaling = np.exp(rng.normal(0, 0.5, N))
    alpha = np.exp(rng.normal(np.log(0.2), np.log(1.5), G))
    beta = np.exp(rng.normal(np.log(1.0), np.log(1.5), G)) + 1
    alpha[5], beta[5] = 0.05, 2.0
    return means, scaling, alpha, beta


def presentation(name):
    """(row_of_cell, cell_index): cells grouped by row, in an order that changes rows at every cell, and grouped with
    global cell ids that are not their positions."""
    rng = np.random.default_rng(len(name))
    if name == "plan_order":
        return (np.arange(N) * 5 % ROWS).astype(np.int32), None
    roc = np.sort(rng.integers(0, ROWS, N)).astype(np.int32)
    roc[-1] = ROWS - 1
    return roc, (rng.permutation(10 * N)[:N].astype(np.int64) + (1 << 33) if name == "shuffled" else None)


_model = {}


def model(G, name):
    """Counts and classes of a case by the scalar model, computed once and shared."""
    if (G, name) not in _model:
        from oracle import nb_model
        means, scaling, alpha, beta = inputs(G)
        roc, cell_index = presentation(name)
        want = nb_model.sample_counts(means, roc, scaling, alpha, beta, SEED, 0, cell_index)
        path = nb_model.nb_params(means, roc, scaling, alpha, beta)[3]
        want.setflags(write=False)
        path.setflags(write=False)
        _model[(G, name)] = want, path
    return _model[(G, name)]


def listed(ctx, path):
    cells, genes, total, overflowed = ctx.last_list()
    assert total == cells.size
    keys = np.unique(cells * 4096 + genes)
    cls = path[keys // 4096, keys % 4096]
    assert np.all(cls[(keys % 4096 < 256) | (keys % 4096 >= 512)] >= 1)
    heavy = keys[(cls == 2) & ((keys % 4096 < 256) | (keys % 4096 >= 512))]
    return heavy, overflowed


@pytest.mark.parametrize("name", ["grouped", "plan_order", "shuffled"])
@pytest.mark.parametrize("G", [520, 522])
@pytest.mark.parametrize("bulk", [64, 128])
def test_graded_plan_counts_equal_the_uniform_geometry_and_the_model(ctx, monkeypatch, bulk, G, name):
    means, scaling, alpha, beta = inputs(G)
    roc, cell_index = presentation(name)
    want, path = model(G, name)
    # the case is what the docstring says it is
    share = [(path[:, a:b] == 2).mean() for a, b in ((0, 256), (256, 512))]
    assert 32 / (8 * 256) < share[0] < 1 / 32 and 1 / 16 < share[1] and want[path == 1].max() > 40

    def call():
        return ctx.sample_counts(means, roc, scaling, alpha, beta, seed=SEED, cell_index=cell_index, check_domain=False).cpu().numpy()

    monkeypatch.setenv("PROSSTT_AMD_STRIP_CELLS", "64")
    uniform = call()
    classes, tiles, blocks = ctx.last_strip_plan()
    np.testing.assert_array_equal(classes, [[0, 64, 0]])
    assert (tiles, blocks) == (3, 9)
    words, strip = ctx.last_run_plan()
    np.testing.assert_array_equal(words, run_words(roc, ROWS, 64))
    heavy_uniform, overflowed_uniform = listed(ctx, path)

    monkeypatch.setenv("PROSSTT_AMD_STRIP_TAPER", "1")
    monkeypatch.setenv("PROSSTT_AMD_STRIP_CELLS", str(bulk))
    graded = call()
    classes, tiles, blocks = ctx.last_strip_plan()
    rule = strip_plan(N, G, 1280, bulk, 1)
    np.testing.assert_array_equal(classes, PLAN[bulk])
    np.testing.assert_array_equal(classes, rule[0])
    assert (tiles, blocks) == rule[1:] == (3, {64: 24, 128: 15}[bulk])
    words, strip = ctx.last_run_plan()
    assert strip == bulk
    np.testing.assert_array_equal(words, plan_run_words(roc, ROWS, classes))
    # the loop every strip takes: the run loop in every class when the cells are grouped, the per-cell loop otherwise
    loops = plan_loops(words, classes, N)
    assert len(loops) == sum(STRIPS[bulk])
    bounds = np.cumsum((0,) + STRIPS[bulk])
    if name == "plan_order":
        assert set(loops) == {"T"}
    else:
        assert all("R" in loops[a:b] for a, b in zip(bounds[:-1], bounds[1:]))
    heavy_graded, overflowed_graded = listed(ctx, path)

    np.testing.assert_array_equal(graded, uniform)
    np.testing.assert_array_equal(graded, want)
    assert overflowed_uniform and overflowed_graded
    np.testing.assert_array_equal(heavy_graded, heavy_uniform)
    outside = np.ones(G, bool)
    outside[256:512] = False
    n_idx, g_idx = np.nonzero((path == 2) & outside)
    np.testing.assert_array_equal(heavy_graded, np.unique(n_idx * 4096 + g_idx))


def test_a_small_launch_keeps_the_uniform_geometry(ctx, monkeypatch):
    """Fewer than four residencies of blocks and no hook: one class of the rule's length (8 cells at this size), the run
    words and counts of the uniform launch."""
    import torch
    monkeypatch.delenv("PROSSTT_AMD_STRIP_CELLS", raising=False)
    monkeypatch.delenv("PROSSTT_AMD_STRIP_TAPER", raising=False)
    G = 520
    means, scaling, alpha, beta = inputs(G)
    roc, cell_index = presentation("grouped")
    got = ctx.sample_counts(means, roc, scaling, alpha, beta, seed=SEED, check_domain=False).cpu().numpy()
    resident = 5 * torch.cuda.get_device_properties(0).multi_processor_count
    classes, tiles, blocks = ctx.last_strip_plan()
    np.testing.assert_array_equal(classes, strip_plan(N, G, resident)[0])
    np.testing.assert_array_equal(classes, [[0, 8, 0]])
    assert (tiles, blocks) == (3, 3 * 20) and blocks < 4 * resident
    words, strip = ctx.last_run_plan()
    assert strip == 8
    np.testing.assert_array_equal(words, run_words(roc, ROWS, 8))
    np.testing.assert_array_equal(got, model(G, "grouped")[0])
