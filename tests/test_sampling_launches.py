"""
What every sampling entry point sends to the count sampler, on the CPU: ``device.get_context`` is replaced by a fake
that records each ``sample_counts`` call and counts the reads of the deferred domain check's verdict.

The expectations are formed here from the plan itself -- ``_density_plan`` / ``cover_whole_tree``, ``calc_scalings``,
``cell_rows`` and a stable argsort by row (the order of presentation) -- never from the output of the code under test.
The tree is the one of test_gpu_domain_check (3 branches, 18 rows, 40 genes); 20 cells in chunks of 7 make three chunks
with a short last one.
"""
import numpy as np
import pytest
import torch

import test_gpu_domain_check as domain
from prosstt_amd import count_model, device, parallel
from prosstt_amd import sim_utils as sut
from prosstt_amd import simulation as sim

G = domain.G_TREE
CELLS, CHUNK = 20, 7
RANGES = [(0, 7), (7, 14), (14, 20)]
AL, BE = np.full(G, domain.ALPHA0), np.full(G, domain.BETA0)


class Recorder:
    """Stand-in for device.Context: CPU tensors, a sampler that records its arguments and returns zeros (or ``out``),
    a verdict that is only counted.  ``fail_at=k``: the k-th launch raises instead of being recorded."""

    def __init__(self, fail_at=None):
        self.torch_device = torch.device("cpu")
        self.launches, self.reads, self.fail_at = [], 0, fail_at

    def tensor(self, array, dtype):
        return torch.as_tensor(np.array(array)).to(dtype)

    def sample_counts(self, means, rows, scaling, alpha, beta, seed, cell_offset=0, out=None, check_domain=True,
                      time_kernel=False, cell_index=None, means_token=None):
        if self.fail_at == len(self.launches) + 1:
            raise RuntimeError("the launch failed")
        self.launches.append(dict(rows=np.array(rows), scaling=np.array(scaling), alpha=alpha, beta=beta, seed=seed,
                                  cell_offset=cell_offset, cell_index=None if cell_index is None else np.array(cell_index),
                                  check_domain=check_domain, means_token=means_token, out_given=out is not None,
                                  reads_before=self.reads))
        return out if out is not None else torch.zeros((len(rows), means.shape[1]), dtype=torch.int32)

    def domain_status(self):
        self.reads += 1


@pytest.fixture
def tree():
    return domain._tiny_tree()


@pytest.fixture
def fake(monkeypatch):
    """``fake()`` installs and returns a fresh Recorder; the host copies are recorded in ``fake.returns``."""
    def install(**kw):
        rec = Recorder(**kw)
        monkeypatch.setattr(device, "get_context", lambda *a, **k: rec)
        return rec
    install.returns = []

    def host_return(counts, out, row_order=None):
        install.returns.append((out, row_order))
        return np.zeros(tuple(counts.shape), np.int32)
    monkeypatch.setattr(sim, "_host_return", host_return)
    return install


def density_plan(tree, cells=CELLS):
    """The plan of sample_density and its kin at numpy seed 33, their default seed and the stream position behind it."""
    np.random.seed(33)
    pt, br = sim._density_plan(tree, cells)
    sc = sut.calc_scalings(cells, True, 0., 0.7)
    return pt, br, sc, own_seed(), np.random.get_state()


def own_seed():
    lo, hi = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
    return int(lo) | (int(hi) << 32)


def presented(rows):
    return np.argsort(rows, kind="stable")


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def per_gene(launch, alpha, beta):
    for got, want in ((launch["alpha"], alpha), (launch["beta"], beta)):
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (G,) and np.all(got == want)


# ---- one launch: sample_density, sample_whole_tree, draw_counts -----------------------------------------------------------

def _one_launch_calls(tree):
    """name -> (call(**options) after np.random.seed(33), its plan)."""
    pt, br, sc, _, _ = density_plan(tree)
    np.random.seed(33)
    wpt, wbr = (np.repeat(v, 2) for v in sim.cover_whole_tree(tree))
    wsc = sut.calc_scalings(len(wpt), True, 0., 0.7)
    return {
        "sample_density": (lambda **o: sim.sample_density(tree, CELLS, alpha=AL, beta=BE, **o)[0], (pt, br, sc)),
        "sample_whole_tree": (lambda **o: sim.sample_whole_tree(tree, 2, alpha=AL, beta=BE, **o)[0], (wpt, wbr, wsc)),
        "draw_counts": (lambda **o: sim.draw_counts(tree, pt, br, sc, AL, BE, **o), (pt, br, sc)),
    }


@pytest.mark.parametrize("name", ["sample_density", "sample_whole_tree", "draw_counts"])
def test_one_launch_entry_points(tree, fake, name):
    call, (pt, br, sc) = _one_launch_calls(tree)[name]
    rows = sim.cell_rows(tree, pt, br)
    perm = presented(rows)
    assert len(np.unique(rows)) < len(rows)
    assert name == "sample_whole_tree" or not np.array_equal(perm, np.arange(len(rows)))     # (that plan is sorted as it is)
    for out in ("torch", "numpy32", "csr"):
        ctx = fake()
        np.random.seed(33)
        result = call(seed=5, out=out)
        (launch,) = ctx.launches
        assert np.array_equal(launch["rows"], rows[perm]) and np.array_equal(launch["scaling"], sc[perm])
        assert np.array_equal(launch["cell_index"], perm) and launch["cell_index"].dtype == np.int64
        assert launch["check_domain"] == "deferred" and launch["means_token"] == tree.means_token()
        assert launch["seed"] == 5 and launch["cell_offset"] == 0 and not launch["out_given"]
        per_gene(launch, AL, BE)
        assert ctx.reads == 1 and launch["reads_before"] == 0
        if out == "torch":
            assert isinstance(result, device.PresentedCounts) and np.array_equal(result.cell_of_row, perm)
            assert result.shape == (len(rows), G)
        else:
            (returned,) = fake.returns[-1:]
            assert returned[0] == out and np.array_equal(returned[1], perm) and result.shape == (len(rows), G)
    ctx = fake()
    np.random.seed(33)
    result = call(seed=5, out="torch", order="plan")
    (launch,) = ctx.launches
    assert np.array_equal(launch["rows"], rows) and np.array_equal(launch["scaling"], sc)
    assert launch["cell_index"] is None and launch["cell_offset"] == 0
    assert launch["check_domain"] == "deferred" and launch["means_token"] == tree.means_token() and ctx.reads == 1
    assert isinstance(result, torch.Tensor) and tuple(result.shape) == (len(rows), G)
    for options in (dict(out="torch"), dict(out="torch", order="plan"), dict(out="numpy")):
        ctx = fake()
        np.random.seed(33)
        call(seed=5, strict=False, **options)
        (launch,) = ctx.launches
        assert launch["check_domain"] is False and ctx.reads == 0


def test_draw_counts_without_cells_still_launches_once(tree, fake):
    none = np.zeros(0, np.int64)
    for options, form in ((dict(out="torch"), device.PresentedCounts), (dict(out="torch", order="plan"), torch.Tensor),
                          (dict(out="numpy32"), np.ndarray)):
        ctx = fake()
        result = sim.draw_counts(tree, none, np.zeros(0, "<U1"), np.zeros(0), AL, BE, seed=5, **options)
        (launch,) = ctx.launches
        assert launch["rows"].shape == (0,) and ctx.reads == 1
        assert isinstance(result, form) and tuple(result.shape) == (0, G)


# ---- sample_density_chunks -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(out="torch"), dict(out="torch", order="plan"), dict(out="numpy32"),
                                     dict(out="numpy32", order="plan")], ids=str)
def test_chunks_are_keyed_by_plan_position_and_enqueued_one_ahead(tree, fake, options):
    pt, br, sc, _, _ = density_plan(tree)
    rows = sim.cell_rows(tree, pt, br)
    in_plan_order = options == dict(out="torch", order="plan")
    ctx = fake()
    np.random.seed(33)
    served = 0
    for c, (part, cpt, cbr, csc) in enumerate(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5,
                                                                         **options)):
        lo, hi = RANGES[c]
        # chunk c + 1 has been enqueued, and the verdict behind chunk c read, before chunk c is handed over
        assert len(ctx.launches) == min(c + 2, 3) and ctx.reads == c + 1
        assert np.array_equal(cpt, pt[lo:hi]) and np.array_equal(cbr, br[lo:hi]) and np.array_equal(csc, sc[lo:hi])
        perm = presented(rows[lo:hi])
        if in_plan_order:
            assert isinstance(part, torch.Tensor) and tuple(part.shape) == (hi - lo, G)
        elif options["out"] == "torch":
            assert isinstance(part, device.PresentedCounts) and np.array_equal(part.cell_of_row, perm)
        else:
            assert fake.returns[-1][0] == "numpy32" and np.array_equal(fake.returns[-1][1], perm)
        served += 1
    assert served == 3 and len(ctx.launches) == 3 and ctx.reads == 3
    for (lo, hi), launch in zip(RANGES, ctx.launches):
        perm = presented(rows[lo:hi])
        assert launch["seed"] == 5 and launch["check_domain"] == "deferred" and launch["means_token"] == tree.means_token()
        per_gene(launch, AL, BE)
        if in_plan_order:
            assert np.array_equal(launch["rows"], rows[lo:hi]) and np.array_equal(launch["scaling"], sc[lo:hi])
            assert launch["cell_index"] is None and launch["cell_offset"] == lo
        else:
            assert np.array_equal(launch["rows"], rows[lo:hi][perm]) and np.array_equal(launch["scaling"], sc[lo:hi][perm])
            assert np.array_equal(launch["cell_index"], lo + perm) and launch["cell_offset"] == 0
    # the launch of chunk c + 1 precedes the read behind chunk c
    assert [launch["reads_before"] for launch in ctx.launches] == [0, 0, 1]
    ctx = fake()
    assert list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, strict=False, **options)) and \
        ctx.reads == 0 and [launch["check_domain"] for launch in ctx.launches] == [False] * 3
    ctx = fake()
    assert list(sim.sample_density_chunks(tree, 0, CHUNK, alpha=AL, beta=BE, seed=5, **options)) == []
    assert ctx.launches == [] and ctx.reads == 0


# ---- parallel, single process ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["presented", "plan"])
def test_sharded_launch(tree, fake, order):
    pt, br, sc, _, _ = density_plan(tree)
    rows = sim.cell_rows(tree, pt, br)
    for strict in (True, False):
        ctx = fake()
        np.random.seed(33)
        counts, mine, gpt, gbr, gsc = parallel.sample_density_sharded(tree, CELLS, alpha=AL, beta=BE, seed=5, order=order,
                                                                      strict=strict)
        (launch,) = ctx.launches
        assert launch["check_domain"] is strict and launch["means_token"] is None and ctx.reads == 0
        assert np.array_equal(gpt, pt) and np.array_equal(gbr, br) and np.array_equal(gsc, sc)
        want = presented(rows) if order == "presented" else np.arange(CELLS)
        assert np.array_equal(mine, want) and mine.dtype == np.int64 and np.array_equal(launch["cell_index"], mine)
        assert np.array_equal(launch["rows"], rows[mine]) and np.array_equal(launch["scaling"], sc[mine])
        assert launch["seed"] == 5 and launch["cell_offset"] == 0 and not launch["out_given"]
        per_gene(launch, AL, BE)
        assert tuple(counts.shape) == (CELLS, G)


@pytest.mark.parametrize("order", ["shard", "plan"])
def test_gathered_launches(tree, fake, order):
    pt, br, sc, _, _ = density_plan(tree)
    layout = np.concatenate(parallel.shards_in_presentation_order(tree, pt, br, 1))
    assert np.array_equal(layout, presented(sim.cell_rows(tree, pt, br)))
    ctx = fake()
    np.random.seed(33)
    out, cell_of_row, gpt, gbr, gsc = parallel.sample_and_gather(tree, CELLS, alpha=AL, beta=BE, seed=5, order=order,
                                                                 chunk_cells=CHUNK)
    assert len(ctx.launches) == 3 and ctx.reads == 1
    for launch in ctx.launches:
        assert launch["out_given"] and launch["check_domain"] == "deferred" and launch["means_token"] == tree.means_token()
        assert launch["seed"] == 5 and launch["reads_before"] == 0
        per_gene(launch, AL, BE)
        at = launch["cell_index"]
        assert np.array_equal(launch["rows"], sim.cell_rows(tree, pt[at], br[at])) and np.array_equal(launch["scaling"], sc[at])
    assert np.array_equal(np.concatenate([launch["cell_index"] for launch in ctx.launches]), layout)
    assert [len(launch["rows"]) for launch in ctx.launches] == [7, 7, 6]
    assert tuple(out.shape) == (CELLS, G) and np.array_equal(gpt, pt) and np.array_equal(gsc, sc)
    assert np.array_equal(cell_of_row, layout) if order == "shard" else cell_of_row is None
    ctx = fake()
    parallel.sample_and_gather(tree, CELLS, alpha=AL, beta=BE, seed=5, order=order, chunk_cells=CHUNK, strict=False)
    assert [launch["check_domain"] for launch in ctx.launches] == [False] * 3 and ctx.reads == 0


# ---- the two entry points with a synchronous check -------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [True, False, 1, 0])
def test_add_non_diff_genes_and_count_model(fake, strict):
    ctx = fake()
    params = dict(alpha=np.full(6, 0.2), beta=np.full(6, 2.0), base_expr=np.arange(1.0, 7.0))
    scalings = np.linspace(0.5, 2.0, 9)
    wide = sim.add_non_diff_genes(np.ones((9, 4)), 6, params, scalings, seed=8, strict=strict)
    (launch,) = ctx.launches
    assert launch["check_domain"] is bool(strict) and launch["means_token"] is None and ctx.reads == 0
    assert np.array_equal(launch["rows"], np.zeros(9)) and np.array_equal(launch["scaling"], scalings) and launch["seed"] == 8
    assert wide.shape == (9, 10)
    ctx = fake()
    mu = np.random.default_rng(2).uniform(0.5, 4.0, (9, G))
    counts = count_model.sample_counts(mu, AL, BE, seed=8, out="torch", strict=strict)
    (launch,) = ctx.launches
    assert bool(launch["check_domain"]) is bool(strict) and launch["check_domain"] != "deferred" and ctx.reads == 0
    assert np.array_equal(launch["rows"], np.arange(9)) and np.array_equal(launch["scaling"], np.ones(9))
    assert launch["seed"] == 8 and launch["cell_index"] is None and tuple(counts.shape) == (9, G)


# ---- the default seed and the stream position ------------------------------------------------------------------------------

def _seeded_calls(tree):
    """name -> (call(seed), the numpy draws the entry point makes in front of its seed)."""
    pt, br, sc, _, _ = density_plan(tree)
    params = dict(alpha=np.full(6, 0.2), beta=np.full(6, 2.0), base_expr=np.arange(1.0, 7.0))
    mu = np.ones((9, G))

    def plan():
        sim._density_plan(tree, CELLS)
        sut.calc_scalings(CELLS, True, 0., 0.7)

    def whole():
        sut.calc_scalings(2 * 18, True, 0., 0.7)

    return {
        "draw_counts": (lambda seed: sim.draw_counts(tree, pt, br, sc, AL, BE, seed=seed, out="torch"), lambda: None),
        "sample_density": (lambda seed: sim.sample_density(tree, CELLS, alpha=AL, beta=BE, seed=seed, out="torch"), plan),
        "sample_whole_tree": (lambda seed: sim.sample_whole_tree(tree, 2, alpha=AL, beta=BE, seed=seed, out="torch"), whole),
        "sample_density_chunks": (lambda seed: list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=seed,
                                                                              out="torch")), plan),
        "sample_density_sharded": (lambda seed: parallel.sample_density_sharded(tree, CELLS, alpha=AL, beta=BE, seed=seed), plan),
        "sample_and_gather": (lambda seed: parallel.sample_and_gather(tree, CELLS, alpha=AL, beta=BE, seed=seed,
                                                                      chunk_cells=CHUNK), plan),
        "add_non_diff_genes": (lambda seed: sim.add_non_diff_genes(np.ones((9, 4)), 6, params, np.ones(9), seed=seed),
                               lambda: None),
        "count_model.sample_counts": (lambda seed: count_model.sample_counts(mu, AL, BE, seed=seed, out="torch"), lambda: None),
    }


ENTRY_POINTS = ["draw_counts", "sample_density", "sample_whole_tree", "sample_density_chunks", "sample_density_sharded",
                "sample_and_gather", "add_non_diff_genes", "count_model.sample_counts"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_default_seed_is_two_draws_at_the_entry_points_own_place(tree, fake, name):
    call, draws_in_front = _seeded_calls(tree)[name]
    ctx = fake()
    np.random.seed(33)
    call(None)
    drawn, behind = {launch["seed"] for launch in ctx.launches}, np.random.get_state()
    # the test's own draws, at the place where the entry point makes them
    np.random.seed(33)
    draws_in_front()
    seed = own_seed()
    assert drawn == {seed} and same_state(behind, np.random.get_state())
    # the same call, given that seed: the same launches, and the stream two draws short of the same position
    ctx = fake()
    np.random.seed(33)
    call(seed)
    assert {launch["seed"] for launch in ctx.launches} == {seed}
    own_seed()
    assert same_state(behind, np.random.get_state())


def test_density_entry_points_share_seed_and_stream_position(tree, fake):
    _, _, _, seed, behind = density_plan(tree)
    calls = _seeded_calls(tree)
    for name in ("sample_density", "sample_density_chunks", "sample_density_sharded", "sample_and_gather"):
        ctx = fake()
        np.random.seed(33)
        calls[name][0](None)
        assert {launch["seed"] for launch in ctx.launches} == {seed}, name
        assert same_state(behind, np.random.get_state()), name


# ---- per-gene parameters -----------------------------------------------------------------------------------------------

def test_scalar_parameters_arrive_one_per_gene(tree, fake):
    calls = {
        "sample_density": lambda: sim.sample_density(tree, CELLS, alpha=0.25, beta=3, seed=5, out="torch"),
        "sample_density (defaults)": lambda: sim.sample_density(tree, CELLS, seed=5, out="torch"),
        "sample_whole_tree": lambda: sim.sample_whole_tree(tree, 2, alpha=0.25, beta=3, seed=5, out="torch"),
        "sample_pseudotime_series": lambda: sim.sample_pseudotime_series(tree, 20, [3, 9], 2.0, alpha=0.25, beta=3, seed=5,
                                                                         out="torch"),
        "sample_density_chunks": lambda: list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=0.25, beta=3, seed=5,
                                                                        out="torch")),
        "sample_density_sharded": lambda: parallel.sample_density_sharded(tree, CELLS, alpha=0.25, beta=3, seed=5),
        "sample_and_gather": lambda: parallel.sample_and_gather(tree, CELLS, alpha=0.25, beta=3, seed=5, chunk_cells=CHUNK),
    }
    for name, call in calls.items():
        ctx = fake()
        np.random.seed(33)
        call()
        assert ctx.launches, name
        for launch in ctx.launches:
            per_gene(launch, *((0.3, 2) if "defaults" in name else (0.25, 3)))
    # a list of per-gene values, and the per-gene arrays of the two entry points that broadcast
    ctx = fake()
    np.random.seed(33)
    sim.sample_density(tree, CELLS, alpha=list(AL), beta=list(BE), seed=5, out="torch")
    per_gene(ctx.launches[0], AL, BE)
    ctx = fake()
    count_model.sample_counts(np.ones((9, G)), 0.25, 3, seed=5, out="torch")
    per_gene(ctx.launches[0], 0.25, 3)


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_refused_arguments_launch_nothing(tree, fake):
    pt, br, sc, _, _ = density_plan(tree)
    refused = [
        lambda: sim.draw_counts(tree, pt, br, sc, AL, BE, seed=5, out="numpy64"),
        lambda: sim.draw_counts(tree, pt, br, sc, AL, BE, seed=5, order="sorted"),
        lambda: sim.draw_counts(tree, pt, br, sc, AL, BE, seed=5, out="torch", order="sorted"),
        lambda: sim.draw_counts(tree, pt[:-1], br, sc, AL, BE, seed=5),
        lambda: sim.draw_counts(tree, pt, br, sc[:-1], AL, BE, seed=5),
        lambda: sim.sample_density(tree, CELLS, alpha=AL, beta=BE, seed=5, out="numpy64"),
        lambda: sim.sample_whole_tree(tree, 2, alpha=AL, beta=BE, seed=5, order="sorted"),
        lambda: list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, out="numpy64")),
        lambda: list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, order="sorted")),
        lambda: list(sim.sample_density_chunks(tree, CELLS, 0, alpha=AL, beta=BE, seed=5)),
        lambda: list(sim.sample_density_chunks(tree, CELLS, -7, alpha=AL, beta=BE, seed=5)),
        lambda: parallel.sample_density_sharded(tree, CELLS, alpha=AL, beta=BE, seed=5, order="shard"),
        lambda: parallel.sample_and_gather(tree, CELLS, alpha=AL, beta=BE, seed=5, order="presented"),
    ]
    for i, call in enumerate(refused):
        ctx = fake()
        np.random.seed(33)
        with pytest.raises(ValueError):
            call()
        assert ctx.launches == [] and ctx.reads == 0, i
    fake()
    with pytest.raises(ValueError, match="out must be"):
        count_model.sample_counts(np.ones((9, G)), AL, BE, seed=5, out="numpy64")
    for call in refused[:3]:
        with pytest.raises(ValueError, match="must be"):
            call()


# ---- no verdict outlives a failed call -----------------------------------------------------------------------------------

def _overflowing(monkeypatch):
    def host_return(counts, out, row_order=None):
        raise OverflowError("a count does not fit")
    monkeypatch.setattr(sim, "_host_return", host_return)


@pytest.mark.parametrize("strict, reads", [(True, 1), (False, 0)])
def test_draw_counts_and_chunks_read_the_verdict_of_a_call_that_fails(tree, fake, monkeypatch, strict, reads):
    pt, br, sc, _, _ = density_plan(tree)
    # the second launch fails while the first is unread
    ctx = fake(fail_at=2)
    np.random.seed(33)
    with pytest.raises(RuntimeError, match="the launch failed"):
        list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, strict=strict))
    assert len(ctx.launches) == 1 and ctx.reads == reads
    # the consumer drops the generator behind its first chunk, while the second launch is unread
    ctx = fake()
    np.random.seed(33)
    chunks = sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, strict=strict)
    next(chunks)
    assert len(ctx.launches) == 2 and ctx.reads == reads
    chunks.close()
    assert ctx.reads == 2 * reads
    # the copy to the host fails
    _overflowing(monkeypatch)
    ctx = fake()
    with pytest.raises(OverflowError):
        sim.draw_counts(tree, pt, br, sc, AL, BE, seed=5, out="numpy16", strict=strict)
    assert len(ctx.launches) == 1 and ctx.reads == reads
    ctx = fake()
    np.random.seed(33)
    with pytest.raises(OverflowError):
        list(sim.sample_density_chunks(tree, CELLS, CHUNK, alpha=AL, beta=BE, seed=5, out="numpy16", strict=strict))
    assert len(ctx.launches) == 2 and ctx.reads == reads


@pytest.mark.parametrize("strict, reads", [(True, 1), (False, 0)])
def test_sample_and_gather_reads_the_verdict_of_a_call_that_fails(tree, fake, strict, reads):
    """A launch fails behind a checked chunk that is already enqueued: its verdict is read on the way out, so that the
    next, unrelated call's ``domain_status()`` has nothing of this call's to raise."""
    ctx = fake(fail_at=2)
    np.random.seed(33)
    with pytest.raises(RuntimeError, match="the launch failed"):
        parallel.sample_and_gather(tree, CELLS, alpha=AL, beta=BE, seed=5, chunk_cells=CHUNK, strict=strict)
    assert len(ctx.launches) == 1 and ctx.reads == reads
