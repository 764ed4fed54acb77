"""-m gpu: no kernel writes or reads outside its buffers, as far as a test that cannot fault can tell.  For every library,
every call of its shared list (the ``calls_*`` functions of tests/test_gpu_stale_memory.py, test_gpu_mapping.py,
test_gpu_trends.py and test_gpu_ptree.py: the stale-memory shapes, 259 x 1025 at the largest) and every call of a second
list, the smallest problem the library admits (where a vector store or a whole-tile store overruns), runs under each byte of
``stale.BYTES`` with tests/guard.py: the device inputs are copies between two bands of 65 536 bytes of that byte, with the
padding columns of a view holding it too, and every tensor the wrappers allocate during the call lies between two such
bands, its interior 0x00 before the call's own fill.  After each call

  1. every band of every allocation still holds the byte: no WRITE outside an output, a slab or a workspace;
  2. every placed input, bands and padding included, is as it was: the inputs are read-only in every library (the one
     documented exception is the sampler's ``out=``: include/prosstt_amd.h line 87, prosstt_amd_sample_counts, "out
     [N][ld_out] int32 counts", is that call's output; its elements are exempt, its bands and padding are not);
  3. the wrappers made at least one guarded allocation, so that another style of allocation cannot empty the test (but for
     ``sample_counts`` with ``out=``, which allocates nothing: there the placed ``out`` is the guarded tensor);
  4. every field of the result has the same bytes under 0x00, 0xFF and 0x7F.  The interior of every allocation is 0x00 each
     time, so a difference can only come from a READ outside a buffer: of a band, or of a padding column.

Out of reach: what the sampler's native context allocates itself (its staging, flags and lists), tensors held from before
the call (the tree's mean tensor), what torch's own operators allocate (``clone``, ``cat``, ``.cuda()``, arithmetic: the
first of the two ping-pong position buffers of ``layout`` and ``tsne`` is such a clone; its twin, which the same kernels
write in every other epoch, is an ``empty_like`` and has its bands), reads outside a buffer that change no result, and
overruns of more than 65 536 bytes.

The census (that every library of _native has a row here) is tests/test_guard.py's, which needs no GPU."""
import numpy as np
import pytest

import guard
import stale
import test_gpu_stale_memory as sm

pytestmark = pytest.mark.gpu


class Placer:
    """The placement handed to a ``calls_*`` function: every device tensor of an input, alone or in a named tuple, becomes a
    copy between guard bands of ``byte``; everything else (host arrays, None, numbers) is handed through."""

    def __init__(self, byte):
        self.byte, self.placed, self.written = byte, [], []

    def __call__(self, value, written=False):
        import torch
        if isinstance(value, torch.Tensor):
            if not value.is_cuda or value.numel() == 0:
                return value
            p = guard.place(value, self.byte, "input %d" % len(self.placed))
            (self.written if written else self.placed).append(p)
            return p.tensor
        if isinstance(value, tuple) and hasattr(value, "_fields"):
            return type(value)(*(self(item) for item in value))
        if isinstance(value, (tuple, list)):
            return type(value)(self(item) for item in value)
        return value

    def check(self):
        for p in self.placed:
            p.check_untouched()
        for p in self.written:                                   # an argument the header documents as written
            p.check_untouched(elements=False)


def _guarded_runs(library, builder, report):
    """``builder``'s calls under every byte: checks 1 to 4 of the module docstring.  Returns (calls, allocations per run)."""
    import torch
    from prosstt_amd import device
    runs, allocations = {}, {}
    for byte in stale.BYTES:
        placer = Placer(byte)
        label, calls = builder(placer)
        for name, call in calls.items():
            what = "%s, %s, byte 0x%02X" % (label, name, byte)
            torch.cuda.synchronize()
            device.release_result_memory()
            with guard.guarded(byte) as state:
                result = call()
                torch.cuda.synchronize()
            try:
                state.check()
                placer.check()
            except AssertionError as exc:
                raise AssertionError("%s: %s" % (what, exc)) from None
            if name == OUT_IS_PLACED:                            # its one output is the placed ``out``, checked above
                assert placer.written and state.allocations == 0, what
            else:
                assert state.allocations > 0, "%s made no allocation that the helper sees" % what
            runs.setdefault(name, []).append(sm._flatten(result))
            allocations.setdefault(name, []).append(state.allocations)
            del result
            state.release()
        assert placer.placed or label in NOTHING_TO_PLACE, "%s: no input was placed" % label
        del placer, calls
        torch.cuda.empty_cache()
    for name, (first, *others) in runs.items():
        assert len(first) > 0 and sum(len(v[3]) for v in first.values()) > 0, (library, name)
        for byte, other in zip(stale.BYTES[1:], others):
            assert sorted(other) == sorted(first), (library, name)
            for path in first:
                assert other[path][:3] == first[path][:3], (library, name, path, "0x%02X" % byte)
                if other[path][3] != first[path][3]:
                    a, b = np.frombuffer(first[path][3], np.uint8), np.frombuffer(other[path][3], np.uint8)
                    where = np.flatnonzero(a != b) if a.size == b.size else np.array([-1])
                    raise AssertionError(
                        "%s %s: %s differs between bands of 0x00 and of 0x%02X in %d of %d bytes, the first at byte %d; the "
                        "interior of every allocation is 0x00 in both runs, so the call READ outside a buffer (a band, or a "
                        "padding column of an input)" % (library, name, path, byte, where.size, a.size, int(where[0])))
    total = sum(a[0] for a in allocations.values())
    print("%s, %s: %d calls, %d guarded allocations under each byte (%s), every band intact, every input untouched, equal "
          "bytes in the three runs" % (library, report, len(runs), total, "/".join(str(a[0]) for a in allocations.values())))
    return len(runs), total


# ------------------------------------------------------------------------------------------------ the smallest problems

def _i32(rows):
    """A count matrix of the given rows on the device as a "shifted" view: one column in, a row stride three above G."""
    import torch
    X = np.asarray(rows, dtype=np.int32)
    wide = torch.full((X.shape[0], X.shape[1] + 3), 12345, dtype=torch.int32, device="cuda")
    wide[:, 1:1 + X.shape[1]] = torch.from_numpy(X).cuda()
    return wide[:, 1:1 + X.shape[1]]


def _one_by_one(place):
    """The (1, 1) count matrix, aligned and shifted."""
    import torch
    return place(torch.tensor([[5]], dtype=torch.int32, device="cuda")), place(_i32([[5]]))


OUT_IS_PLACED = "sample_counts, one row into out="               # the wrapper allocates nothing then: check 3 does not apply


def small_sampler(place):
    """``sample_density`` for a handful of cells; ``Context.sample_counts`` into a placed ``out=`` of one row."""
    import torch
    import test_gpu_fit
    from prosstt_amd import device, simulation as sim
    tree = test_gpu_fit._tree()
    alpha, beta = np.full(300, 0.2), np.full(300, 2.0)

    def density():
        np.random.seed(1234)
        return sim.sample_density(tree, 5, alpha=alpha, beta=beta, seed=11, out="torch")

    means = place(torch.from_numpy(np.random.default_rng(3).lognormal(0.0, 1.0, (4, 7)).astype(np.float32)).cuda())
    wide = torch.full((1, 11), 12345, dtype=torch.int32, device="cuda")
    out = place(wide[:, 1:8], written=True)                      # prosstt_amd_sample_counts writes ``out``: see the docstring

    def one_row():
        got = device.get_context().sample_counts(means, np.array([2], dtype=np.int32), np.array([1.5]), np.full(7, 0.2),
                                                 np.full(7, 2.0), 7, out=out)
        assert got.data_ptr() == out.data_ptr()
        return got

    return "sampler, smallest", {"sample_density of 5 cells": density, OUT_IS_PLACED: one_row}


def small_stats(place):
    from prosstt_amd import summary
    aligned, shifted = _one_by_one(place)
    return "summary, (1, 1)", {"aligned": lambda: summary.count_summary(aligned),
                               "shifted": lambda: summary.count_summary(shifted)}


def small_embed(place):
    import torch
    from prosstt_amd import embed
    aligned, shifted = _one_by_one(place)
    s = np.array([1.5])
    W = place(torch.tensor([[0.75]], dtype=torch.float32, device="cuda"))
    calls = {}
    for name, X in (("aligned", aligned), ("shifted", shifted)):
        calls["matmul, l = 1, " + name] = lambda X=X: embed.LogNormalized(X, s).matmul(W)
        calls["rmatmul, l = 1, " + name] = lambda X=X: embed.LogNormalized(X, s).rmatmul(W)
        calls["gene_moments " + name] = lambda X=X: embed.LogNormalized(X, s).gene_moments()
    return "embed, (1, 1)", calls


def small_hvg(place):
    from prosstt_amd import hvg
    aligned, shifted = _one_by_one(place)
    s = np.array([1.5])
    calls = {}
    for name, X in (("aligned", aligned), ("shifted", shifted)):
        calls["clipped_sums " + name] = lambda X=X: hvg.clipped_sums(X, np.array([3]))
        calls["normalized_moments " + name] = lambda X=X: hvg.normalized_moments(X, s)
        calls["select_genes " + name] = lambda X=X: hvg.select_genes(X, np.array([0]))
    return "hvg, (1, 1)", calls


def small_markers(place):
    from prosstt_amd import markers
    aligned, shifted = _one_by_one(place)
    s, labels = np.array([1.5]), np.array([0])
    return "markers, (1, 1)", {
        "group_moments aligned": lambda: markers.group_moments(aligned, s, labels),
        "group_moments shifted, out=torch": lambda: markers.group_moments(shifted, s, labels, rows_per_block=1, out="torch")}


def small_ranks(place):
    """One labelled cell (the first of test_gpu_ranks' sizes), with five genes as there and with one."""
    import test_gpu_ranks as tr
    from prosstt_amd import ranks
    labels, N = tr._labels(1, 3)
    s = tr._input("a", N, 5)[1]
    calls = {}
    for view in tr.VIEWS:
        X = place(tr._view("a", N, 5, view))
        calls["n_sel = 1, G = 5, " + view] = lambda X=X: ranks.rank_sums(X, s, labels)
        calls["n_sel = 1, G = 1, out=torch, " + view] = lambda X=X: ranks.rank_sums(X[:, :1], s, labels, out="torch")
    return "ranks, one labelled cell", calls


def small_fit(place):
    from prosstt_amd import fit
    aligned, shifted = _one_by_one(place)
    args = (np.array([1.5]), np.array([0]), np.array([[2.0]]), np.array([[0.2]]), np.array([[2.0]]))
    return "fit, (1, 1, K = 1, C = 1)", {"loglik aligned": lambda: fit.loglik(aligned, *args),
                                         "loglik shifted, out=torch": lambda: fit.loglik(shifted, *args, out="torch")}


def small_autocorr(place):
    """(1, 1) with the hand-made graph, the first of test_gpu_autocorr's cases."""
    import test_gpu_autocorr as ta
    import test_gpu_markers as tm
    from prosstt_amd import autocorr
    N, G, kind = ta.CASES[0]
    assert (N, G) == (1, 1)
    s = tm._host(N, G)[1]
    g = place(ta._as_graph(ta._graph(N, kind)))
    calls = {}
    for view in tm.VIEWS:
        X = place(tm._view(N, G, view))
        calls["graph_sums " + view] = lambda X=X: autocorr.graph_sums(X, s, g)
        calls["smooth " + view] = lambda X=X: autocorr.smooth(X, s, g)
    return "autocorr, (1, 1)", calls


def small_knn(place):
    """N = 2, d = 1, k = 1, the first of test_gpu_knn's cases, in both views."""
    import knn_model
    import test_gpu_knn as tk
    from prosstt_amd import neighbors
    N, d, k = tk.CASES[0][:3]
    assert (N, d, k) == (2, 1, 1)
    P = knn_model.gaussian(N, d, 1000 * N + 10 * d + k)
    calls = {}
    for view in ((0, 0), (3, 1)):
        Pv = place(tk._input(P, view))
        calls["view %s" % (view,)] = lambda Pv=Pv: neighbors.knn(Pv, k)
        calls["view %s, out=torch, chunks of 1" % (view,)] = lambda Pv=Pv: neighbors.knn(Pv, k, out="torch", chunk_rows=1)
    return "knn, N = 2, d = 1, k = 1", calls


def _smallest_graph():
    """The (3, 2) kNN case of test_gpu_cluster.KNN_CASES."""
    import graph_model
    import test_gpu_cluster as tc
    assert tc.KNN_CASES[0] == (3, 2)
    return graph_model.case(3, 2)


def small_graph(place):
    import test_gpu_graph as tg
    from prosstt_amd import graph
    nb = place(tg._neighbors(_smallest_graph()))
    g = place(graph.connectivities(nb, out="torch"))
    return "graph, (3, 2)", {
        "connectivities, out=torch": lambda: graph.connectivities(nb, out="torch"),
        "connectivities": lambda: graph.connectivities(nb),
        "transitions of connectivities": lambda: graph.transitions(g),
        "transitions of neighbours": lambda: graph.transitions(nb),
        "diffmap, 2 components": lambda: graph.diffmap(nb, 2)}


def small_layout(place):
    import layout_model
    import test_gpu_layout as tl
    from prosstt_amd import layout
    conn = place(tl._conn_of(_smallest_graph()["W"]))
    calls = {}
    for c in (2, 3):
        Y = place(sm._cuda(np.random.default_rng(c).uniform(-10, 10, (3, c)).astype(np.float32)))
        for lanes in tl.LANES:
            calls["c = %d, %d lanes" % (c, lanes)] = lambda Y=Y, lanes=lanes: layout.optimize(
                conn, Y, 0, 3, lanes_per_row=lanes, n_epochs=50, a=layout_model.A, b=layout_model.B, seed=3)
    return "layout, (3, 2)", calls


def small_tsne(place):
    """Three cells with two neighbours each; the perplexity must lie in (1, 2)."""
    import test_gpu_tsne as tt
    from prosstt_amd import tsne
    case = _smallest_graph()
    nb = place(tt._neighbors(case["idx"], case["d2"]))
    aff = place(tsne.affinities(nb, 1.5, out="torch"))
    calls = {"affinities, out=torch": lambda: tsne.affinities(nb, 1.5, out="torch"),
             "affinities": lambda: tsne.affinities(nb, 1.5)}
    for c in (2, 3):
        Y = place(sm._cuda(np.random.default_rng(c).uniform(-1, 1, (3, c)).astype(np.float32)))
        for slabs in (0, 3):
            tag = "c = %d, slabs %d" % (c, slabs)
            calls["gradient " + tag] = lambda Y=Y, slabs=slabs: tsne.gradient(aff, Y, exaggeration=12.0, slabs=slabs, _sums=True)
            calls["optimize " + tag] = lambda Y=Y, slabs=slabs: tsne.optimize(aff, Y, 0, 3, exploration=2, learning_rate=50.0,
                                                                             slabs=slabs)
    return "tsne, (3, 2)", calls


def small_dpt(place):
    """test_gpu_dpt's smallest map (3 cells, 2 components) and its smallest concordance (3 ranks); ``dpt.dpt`` refuses fewer
    than 4 cells (2 <= min_group_size and 2 min_group_size <= cells), so it gets a map of 4."""
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    dm = td._random_map(3, 2)
    dm = place(dm._replace(eigenvalues=td._cuda(dm.eigenvalues), eigenvectors=td._cuda(dm.eigenvectors)))
    dm4 = td._random_map(4, 2)
    dm4 = place(dm4._replace(eigenvalues=td._cuda(dm4.eigenvalues), eigenvectors=td._cuda(dm4.eigenvectors)))
    r = place(td._cuda(np.array([[2, 0, 1]], dtype=np.int32)))    # (batch, cells)
    r2 = place(td._cuda(np.array([[1, 2, 0]], dtype=np.int32)))
    return "dpt, 3 cells", {
        "distances, one source": lambda: dpt.distances(dm, [2], 1),
        "distances, four sources, out=torch": lambda: dpt.distances(dm, [0, 1, 2, 1], 2, out="torch"),
        "concordance": lambda: dpt.concordance(r, r2),
        "concordance, slabs 3": lambda: dpt.concordance(r, r2, 3),
        "dpt of 4 cells without a branching": lambda: dpt.dpt(dm4, 0, min_group_size=2),
        "dpt of 4 cells, one branching, slabs 3, out=torch": lambda: dpt.dpt(dm4, 3, 2, n_branchings=1, min_group_size=2, slabs=3,
                                                                             out="torch")}


def small_cluster(place):
    import test_gpu_cluster as tc
    from prosstt_amd import cluster, graph
    host = tc._connectivities(*tc.KNN_CASES[0])
    g = place(graph.Connectivities(sm._cuda(host.indptr), sm._cuda(host.indices), sm._cuda(host.data), None, None))
    calls = {"path %d" % path: (lambda path=path: cluster.louvain(g, path=path)) for path in tc.PATHS}
    calls["out=torch"] = lambda: cluster.louvain(g, 2.0, out="torch")
    return "cluster, (3, 2)", calls


def small_trends(place):
    """N = G = R = 1, the first of each of test_gpu_trends' lists, on its three layouts."""
    import test_gpu_trends as tt
    from prosstt_amd import trends
    assert (tt.NS[0], tt.GS[0], tt.RS[0]) == (1, 1, 1)
    w = trends.NodeWeights(np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([4096], dtype=np.int32), 1)
    calls = {}
    for layout in tt.LAYOUTS:
        X = place(tt._view(np.array([[7]], dtype=np.int32), layout))
        calls[layout] = lambda X=X: trends.node_sums(X, w)
        calls[layout + ", out=torch, chunks of 1"] = lambda X=X: trends.node_sums(X, w, entries_per_block=1, out="torch")
    return "trends, N = G = R = 1", calls


def small_mapping(place):
    """N = G = R = 1, the first of each of test_gpu_mapping's lists, on its three layouts."""
    import test_gpu_mapping as tm
    from prosstt_amd import mapping
    assert (tm.NS[0], tm.GS[0], tm.RS[0]) == (1, 1, 1)
    rng = np.random.default_rng(1)
    X, s, P, m, c = tm._exact_inputs(1, 1, 1, rng)
    offsets = tm._offsets(1, rng)
    Pd = place(sm._cuda(P))
    calls = {}
    for layout in tm.LAYOUTS:
        view = place(tm._view(X, layout))
        calls[layout] = lambda view=view: mapping.node_scores(view, s, P, m, c, offsets)
        calls[layout + ", scores, out=torch, a device panel"] = lambda view=view: mapping.node_scores(
            view, s, Pd, m, c, offsets, scores=True, out="torch", node_tile=1, genes_per_chain=32)
    return "mapping, N = G = R = 1", calls


def small_ptree(place):
    """N = R = d = 1 for the passes; the projection needs an edge, so R = 2 and E = 1 there."""
    import test_gpu_ptree as tp
    from prosstt_amd import ptree
    assert (tp.NS[0], tp.RS[0], tp.DS[0]) == (1, 1, 1)
    Y, C = np.array([[0.5]], dtype=np.float32), np.array([[-0.25]], dtype=np.float32)
    C2, edges = np.array([[-0.25], [1.0]], dtype=np.float32), np.array([[0, 1]], dtype=np.int32)
    calls = {}
    for layout in tp.LAYOUTS:
        Yv, Cv, C2v = place(tp._view(Y, layout)), place(tp._view(C, layout)), place(tp._view(C2, layout))
        calls["assign, hard, " + layout] = lambda Yv=Yv, Cv=Cv: ptree.assign(Yv, Cv, 0.0, responsibilities=True)
        calls["assign, soft, out=torch, " + layout] = lambda Yv=Yv, Cv=Cv: ptree.assign(Yv, Cv, 0.7, responsibilities=True,
                                                                                       out="torch")
        calls["project, R = 2, E = 1, " + layout] = lambda Yv=Yv, C2v=C2v: ptree.project(Yv, C2v, edges)
    return "ptree, N = R = d = 1", calls


# ------------------------------------------------------------------------------------------------------- every library

def _of(module, name):
    def builder(place):
        import importlib
        return getattr(importlib.import_module(module), name)(place)
    return builder


# library of prosstt_amd._native -> (its shared list, its smallest problems); "host" is host code only
LIBRARIES = {
    "sampler": (sm.calls_sampler, small_sampler),
    "stats": (sm.calls_summary, small_stats),
    "embed": (sm.calls_embed, small_embed),
    "knn": (sm.calls_knn, small_knn),
    "graph": (sm.calls_graph, small_graph),
    "layout": (sm.calls_layout, small_layout),
    "tsne": (sm.calls_tsne, small_tsne),
    "dpt": (sm.calls_dpt, small_dpt),
    "markers": (sm.calls_markers, small_markers),
    "cluster": (sm.calls_cluster, small_cluster),
    "ranks": (sm.calls_ranks, small_ranks),
    "hvg": (sm.calls_hvg, small_hvg),
    "autocorr": (sm.calls_autocorr, small_autocorr),
    "fit": (sm.calls_fit, small_fit),
    "trends": (_of("test_gpu_trends", "calls_trends"), small_trends),
    "mapping": (_of("test_gpu_mapping", "calls_mapping"), small_mapping),
    "ptree": (_of("test_gpu_ptree", "calls_ptree"), small_ptree),
}
NOT_ON_THE_DEVICE = {"host"}
NOTHING_TO_PLACE = {"simulation.sample_density", "cluster.louvain"}      # shared lists of the tree and of host arrays alone


@pytest.mark.parametrize("library", list(LIBRARIES))
def test_no_access_outside_a_buffer(library):
    shared, smallest = LIBRARIES[library]
    _guarded_runs(library, shared, "the stale-memory shapes")
    _guarded_runs(library, smallest, "the smallest problem")


def test_the_runs_see_a_store_past_an_output_and_a_read_of_a_band():
    """The checks as the runs above apply them, on the device: a store one element past the end of a wrapper-style
    allocation (into the helper's own band, through a view of the helper's own storage), a write to an input, and a result
    that holds what lies behind an input."""
    import torch

    def past(t, n=1):
        return torch.as_strided(t, (n,), (1,), t.storage_offset() + t.numel())

    def overrun(place):
        def call():
            out = torch.empty(6, dtype=torch.int32, device="cuda").fill_(3)
            past(out).fill_(0x3C3C3C3C)                          # (no byte of it is one of the three)
            return out
        return "the check", {"a store past the end": call}

    with pytest.raises(AssertionError, match=r"back band of \(6,\) of torch.int32 .* 4 bytes damaged, first at \+0 from"):
        _guarded_runs("the check", overrun, "the check")

    def writes_an_input(place):
        x = place(torch.arange(6, dtype=torch.int32, device="cuda"))
        return "the check", {"an input written": lambda: (x.add_(1), torch.zeros(1, device="cuda"))}

    with pytest.raises(AssertionError, match="an input was written: .* elements: 6 bytes changed"):
        _guarded_runs("the check", writes_an_input, "the check")

    def reads_a_band(place):
        x = place(torch.arange(6, dtype=torch.int32, device="cuda"))
        return "the check", {"a read past an input": lambda: torch.empty(7, dtype=torch.int32, device="cuda").copy_(
            torch.as_strided(x, (7,), (1,), x.storage_offset()))}

    with pytest.raises(AssertionError, match="differs between bands of 0x00 and of 0xFF in 4 of 28 bytes, the first at byte 24"):
        _guarded_runs("the check", reads_a_band, "the check")

    def in_full(place):
        x = place(torch.ones(4, dtype=torch.float64, device="cuda"))
        return "the check", {"written in full": lambda: torch.zeros((3, 4), dtype=torch.float64, device="cuda").add_(x)}

    _guarded_runs("the check", in_full, "the check")
