"""-m gpu: no result depends on what uninitialised memory held.  Every public entry point is called once under each byte
of tests/stale.py (0x00; 0xFF: NaN and -1; 0x7F: 3.4e38, 1.4e306 and 2139062143), which fills every tensor that the wrappers
get from ``torch.empty``, ``empty_like``, ``empty_strided`` or ``new_empty``: outputs, slabs, ping-pong positions, bounce
buffers and every workspace of ``device.workspace``.  Every field of the result must have the same bytes in the three runs
(every library already asserts equal bits across calls and streams, so there is no tolerance), and the count of poisoned
allocations must have risen during the call, so that another style of allocation cannot empty the test.  A kernel that
reads a slot before it writes it, sums a slab that it did not clear, or skips an output element fails here, where a fresh
process, which gets zero pages most of the time, shows nothing.

The shapes are the smallest of each library's own suite with a ragged last strip of genes, a ragged last block of rows and
more than one slab, chunk or pass; the inputs are those suites' own.

Out of reach of the helper, and so not covered: what the native context of the sampler allocates itself (its staging,
flags and lists: prosstt_amd_ctx_create), the tree's mean tensor and the lineage tensors held from before the block, the
diffusion map and the graphs handed in as inputs, numpy's host arrays (``np.empty`` in ``device.to_host`` for matrices of
2^24 counts or more: not reached at these sizes), and tensors that torch's own operators allocate (``clone``, ``zeros``,
arithmetic: written in full by the operator).  Before each run the recycled host blocks (``device.release_result_memory``)
and torch's cached device blocks are released, so that nothing a former run wrote is handed out again unpoisoned.

No header documents a result field as partly unspecified, so no field is left out of the comparison."""
import numpy as np
import pytest

import stale

pytestmark = pytest.mark.gpu


def _flatten(value, path="result", out=None):
    """{path: (type, dtype, shape, bytes)} of every array, tensor and scalar in a result: named tuples, tuples, lists, dicts,
    scipy CSR matrices, device.PresentedCounts and the libraries' result classes by their public attributes."""
    import scipy.sparse as sparse
    import torch
    out = {} if out is None else out
    if isinstance(value, torch.Tensor):
        host = value.detach().cpu().contiguous()
        body = host.reshape(-1).view(torch.uint8).numpy().tobytes() if host.numel() else b""
        out[path] = ("tensor", str(value.dtype), tuple(value.shape), body)
    elif isinstance(value, np.ndarray):
        body = repr(value.tolist()).encode() if value.dtype == object else np.ascontiguousarray(value).tobytes()
        out[path] = ("ndarray", str(value.dtype), value.shape, body)
    elif sparse.issparse(value):
        for name in ("indptr", "indices", "data"):
            _flatten(getattr(value, name), "%s.%s" % (path, name), out)
        out[path + ".shape"] = ("shape", "", (), repr(value.shape).encode())
    elif isinstance(value, tuple) and hasattr(value, "_fields"):
        for name in value._fields:
            _flatten(getattr(value, name), "%s.%s" % (path, name), out)
    elif isinstance(value, (tuple, list)):
        out[path + ".len"] = ("len", "", (), repr(len(value)).encode())
        for i, item in enumerate(value):
            _flatten(item, "%s[%d]" % (path, i), out)
    elif isinstance(value, dict):
        for key in sorted(value):
            _flatten(value[key], "%s[%r]" % (path, key), out)
    elif value is None or isinstance(value, (bool, int, float, str, bytes, np.generic)):
        out[path] = ("scalar", type(value).__name__, (), repr(value).encode())
    elif hasattr(value, "__dict__"):
        public = {k: v for k, v in vars(value).items() if not k.startswith("_")}
        assert public, "nothing to compare in %s (%s)" % (path, type(value).__name__)
        for name in sorted(public):
            _flatten(public[name], "%s.%s" % (path, name), out)
    else:
        raise TypeError("no rule to compare %s of type %s" % (path, type(value).__name__))
    return out


def _thrice(library, calls):
    """Each of ``calls`` ({name: a function without arguments}) under every byte: equal bytes in every field, and poisoned
    allocations in every run."""
    import torch
    from prosstt_amd import device
    for name, call in calls.items():
        runs, fills = [], []
        for byte in stale.BYTES:
            torch.cuda.synchronize()
            device.release_result_memory()
            torch.cuda.empty_cache()
            with stale.poisoned(byte) as poison:
                result = call()
                torch.cuda.synchronize()
            runs.append(_flatten(result))
            fills.append(poison.fills)
            del result
        assert min(fills) > 0, "%s %s made no allocation that the helper sees (%s)" % (library, name, fills)
        assert len(runs[0]) > 0 and sum(len(v[3]) for v in runs[0].values()) > 0
        for byte, other in zip(stale.BYTES[1:], runs[1:]):
            assert sorted(other) == sorted(runs[0]), (library, name)
            for path in runs[0]:
                assert other[path][:3] == runs[0][path][:3], (library, name, path, "0x%02X" % byte)
                if other[path][3] != runs[0][path][3]:
                    a = np.frombuffer(runs[0][path][3], np.uint8)
                    b = np.frombuffer(other[path][3], np.uint8)
                    where = np.flatnonzero(a != b) if a.size == b.size else np.array([-1])
                    raise AssertionError("%s %s: %s differs between 0x00 and 0x%02X in %d of %d bytes, the first at byte %d"
                                         % (library, name, path, byte, where.size, a.size, int(where[0])))
        print("%s %s: %s poisoned allocations under 0x00, 0xFF, 0x7F; %d fields of %d bytes identical in the three runs"
              % (library, name, "/".join(str(f) for f in fills), len(runs[0]), sum(len(v[3]) for v in runs[0].values())))


def _cuda(array):
    import torch
    return torch.from_numpy(np.array(array)).cuda()


def _identity(value):
    """The placement of the inputs in this module: where their suites put them.  tests/test_gpu_guard_bands.py hands the
    ``calls_*`` functions below (each returns its library's label and {name: a function without arguments}) a placement that
    copies every device tensor of an input between guard bands (tests/guard.py); device tensors, and named tuples of them,
    are what a placement is given."""
    return value


def _counts(place=_identity):
    """test_gpu_markers' draw at (259, 1025): five blocks of rows with a ragged last one, one whole strip of 1024 genes and
    a remainder; its shifted view (odd row stride, base off 16 bytes: the scalar loads), its aligned one, the size factors."""
    import test_gpu_markers as tm
    return place(tm._view(259, 1025, "shifted")), place(tm._view(259, 1025, "aligned")), tm._host(259, 1025)[1]


def test_the_comparison_sees_an_output_that_is_not_written():
    """The check itself: a result that is an allocation nobody wrote differs between the bytes, one written in full does not,
    and a call that allocates nothing through torch fails the counter."""
    import torch
    with pytest.raises(AssertionError, match="differs between 0x00 and 0xFF in 20 of 20 bytes"):
        _thrice("the check", {"an unwritten output": lambda: torch.empty(5, dtype=torch.float32, device="cuda")})
    with pytest.raises(AssertionError, match="differs between 0x00 and 0xFF in 4 of 24 bytes, the first at byte 20"):
        _thrice("the check", {"a skipped element": _skipped})
    _thrice("the check", {"written in full": lambda: torch.empty((3, 4), dtype=torch.float64, device="cuda").fill_(2.5)})
    with pytest.raises(AssertionError, match="made no allocation that the helper sees"):
        _thrice("the check", {"no allocation": lambda: torch.zeros(5, device="cuda")})


def _skipped():
    """Six int32 of which the kernel wrote five."""
    import torch
    out = torch.empty(6, dtype=torch.int32, device="cuda")
    out[:5] = 3
    return out


# ------------------------------------------------------------------------------------------------------------ sampler

def calls_sampler(place=_identity):
    """(Every input is a host array or the tree: nothing to place.)"""
    from prosstt_amd import simulation as sim
    import test_gpu_fit
    tree = test_gpu_fit._tree()
    alpha, beta = np.full(300, 0.2), np.full(300, 2.0)

    def draw(**kw):
        def call():
            np.random.seed(1234)
            return sim.sample_density(tree, 3000, alpha=alpha, beta=beta, seed=11, **kw)
        return call

    calls = {"out=%s" % out: draw(out=out) for out in ("numpy", "numpy32", "numpy16", "csr", "torch")}
    calls["out=torch, order=plan"] = draw(out="torch", order="plan")
    return "simulation.sample_density", calls


def test_simulation_sample_density():
    _thrice(*calls_sampler())


# ------------------------------------------------------------------------------------------------- count-matrix readers

def calls_summary(place=_identity):
    from prosstt_amd import summary
    shifted, aligned, _ = _counts(place)
    return "summary.count_summary", {"shifted": lambda: summary.count_summary(shifted),
                                     "aligned": lambda: summary.count_summary(aligned)}


def test_summary():
    _thrice(*calls_summary())


def calls_embed(place=_identity):
    import torch
    from prosstt_amd import embed
    shifted, aligned, s = _counts(place)
    rng = np.random.default_rng(5)
    W = place(torch.as_tensor(rng.standard_normal((1025, 50)).astype(np.float32)).cuda())
    Q = place(torch.as_tensor(rng.standard_normal((259, 50)).astype(np.float32)).cuda())
    calls = {}
    for name, X in (("shifted", shifted), ("aligned", aligned)):
        calls["pca " + name] = lambda X=X: embed.pca(X, s, 20)
        calls["matmul " + name] = lambda X=X: embed.LogNormalized(X, s).matmul(W)
        calls["rmatmul " + name] = lambda X=X: embed.LogNormalized(X, s).rmatmul(Q)
        calls["gene_moments " + name] = lambda X=X: embed.LogNormalized(X, s).gene_moments()
    return "embed", calls


def test_embed():
    _thrice(*calls_embed())


def calls_hvg(place=_identity):
    import torch
    import hvg_model
    import test_gpu_hvg
    from prosstt_amd import hvg
    X, _, n_top, sc = hvg_model.inputs("wide")                   # 257 x 1100: its suite's whole calls
    D = torch.as_tensor(X).cuda()
    wide = torch.full((257, 1103), 7, dtype=torch.int32, device="cuda")
    wide[:, 1:1101] = D
    D, view = place(D), place(wide[:, 1:1101])
    gather = place(test_gpu_hvg._gather_matrix()[1])             # 67 x 1100, row stride 1103, a base off 16 bytes
    idx = np.random.default_rng(257).permutation(1100)[:257]
    calls = {}
    for name, M in (("aligned", D), ("shifted", view)):
        calls["seurat_v3 " + name] = lambda M=M: hvg.highly_variable_genes(M, n_top_genes=n_top)
        calls["seurat " + name] = lambda M=M: hvg.highly_variable_genes(M, sc, n_top, "seurat")
    calls["select_genes"] = lambda: hvg.select_genes(gather, idx)
    calls["select_genes, a mask"] = lambda: hvg.select_genes(gather, np.arange(1100) % 3 == 0)
    return "hvg", calls


def test_hvg():
    _thrice(*calls_hvg())


def calls_markers(place=_identity):
    """``rank_genes_groups`` refuses a group of fewer than two cells (``markers.statistics``), so the empty group goes through
    ``group_moments``, the device pass of ``rank_genes_groups``, and the whole call gets three populated groups."""
    import test_gpu_markers as tm
    from prosstt_amd import markers
    shifted, aligned, s = _counts(place)
    sparse_labels = tm._labels(259, 3)                           # group 1 is empty, group 2 a single cell, some cells left out
    assert not (sparse_labels == 1).any() and (sparse_labels == 2).sum() == 1 and (sparse_labels == -1).any()
    labels = np.where(sparse_labels < 0, -1, np.arange(259) % 3)
    calls = {}
    for name, X in (("shifted", shifted), ("aligned", aligned)):
        calls["rank_genes_groups " + name] = lambda X=X: markers.rank_genes_groups(X, s, labels)
        calls["group_moments, an empty group, " + name] = lambda X=X: markers.group_moments(X, s, sparse_labels)
        calls["group_moments, an empty group, 64 rows per block, out=torch, " + name] = lambda X=X: markers.group_moments(
            X, s, sparse_labels, rows_per_block=64, out="torch")
    calls["rank_genes_groups wilcoxon"] = lambda: markers.rank_genes_groups(shifted[:, :130], s, labels, method="wilcoxon",
                                                                              tie_correct=True)
    return "markers", calls


def test_markers():
    _thrice(*calls_markers())


def calls_ranks(place=_identity):
    import test_gpu_ranks as tr
    from prosstt_amd import ranks
    K, G = 3, 1024 + 37                                          # a whole strip of the emit kernel and its remainder
    labels, N = tr._labels(65, K)
    s = tr._input("a", N, G)[1]
    calls = {}
    for view in tr.VIEWS:
        X = place(tr._view("a", N, G, view))
        calls["two passes, " + view] = lambda X=X: ranks.rank_sums(X, s, labels, genes_per_pass=1024)
        calls["reference 0, out=torch, " + view] = lambda X=X: ranks.rank_sums(X, s, labels, reference=0, out="torch")
    labels2, N2 = tr._labels(1025, 7)                            # more than one tile of the sort
    X2, s2 = place(tr._view("b", N2, 6, "shifted")), tr._input("b", N2, 6)[1]
    calls["two sort tiles, tied keys"] = lambda: ranks.rank_sums(X2, s2, labels2)
    return "ranks.rank_sums", calls


def test_ranks():
    _thrice(*calls_ranks())


def calls_fit(place=_identity):
    import test_gpu_fit as tf
    from prosstt_amd import fit
    calls = {}
    for shift in (0, 1):                                         # (257, 1025, 7, 9, 3, "big") of its suite, both alignments
        rng = np.random.default_rng(257 * 100003 + 1025 * 7 + 3 + 31 * 9 + 7)
        _, view = tf._matrix(257, 1025, 3, "big", shift, rng)
        sc, labels, means, alpha, beta = tf._inputs(257, 1025, 7, 9, rng)
        args = (place(view), sc, labels, means, alpha, beta)
        calls["loglik, shift %d" % shift] = lambda args=args: fit.loglik(*args)
        calls["loglik, shift %d, out=torch" % shift] = lambda args=args: fit.loglik(*args, out="torch")
    return "fit.loglik", calls


def test_fit():
    _thrice(*calls_fit())


def calls_autocorr(place=_identity):
    import test_gpu_autocorr as ta
    import test_gpu_markers as tm
    from prosstt_amd import autocorr
    N, G = 130, 300                                              # three blocks of 64 rows and five tiles of 64 genes, both ragged
    s = tm._host(N, G)[1]
    calls = {}
    for kind in ta.GRAPHS:
        g = place(ta._as_graph(ta._graph(N, kind)))
        for view in tm.VIEWS:
            X = place(tm._view(N, G, view))
            tag = "%s graph, %s" % (kind, view)
            calls["graph_sums, " + tag] = lambda X=X, g=g: autocorr.graph_sums(X, s, g, rows_per_block=64, gene_tile=64)
            calls["graph_sums by default, out=torch, " + tag] = lambda X=X, g=g: autocorr.graph_sums(X, s, g, out="torch")
            calls["smooth, " + tag] = lambda X=X, g=g: autocorr.smooth(X, s, g, gene_tile=64)
            calls["smooth, unnormalised, out=numpy, " + tag] = lambda X=X, g=g: autocorr.smooth(X, s, g, normalize=False,
                                                                                                  out="numpy")
    return "autocorr", calls


def test_autocorr():
    _thrice(*calls_autocorr())


# -------------------------------------------------------------------------------------------------------- cell graphs

def calls_knn(place=_identity):
    import knn_model
    import test_gpu_knn as tk
    from prosstt_amd import neighbors
    host = knn_model.gaussian(257, 2, 1000 * 257 + 20 + 255)
    P = knn_model.gaussian(257, 31, 1000 * 257 + 310 + 256)
    view = place(tk._input(P, (3, 1)))                           # rows that do not start on 16 bytes
    lattice = place(tk._input(knn_model.lattice(2049, 7), (0, 0)))      # ties across three segments of the select kernel
    return "neighbors.knn", {
        "a host array, chunks of 100": lambda: neighbors.knn(host, 255, chunk_rows=100),
        "an unaligned view, chunks of 7": lambda: neighbors.knn(view, 256, chunk_rows=7, out="torch"),
        "ties, chunks of 1000": lambda: neighbors.knn(lattice, 15, chunk_rows=1000)}


def test_neighbors_knn():
    _thrice(*calls_knn())


def calls_graph(place=_identity):
    import graph_model
    import test_gpu_graph as tg
    from prosstt_amd import graph
    nb = place(tg._neighbors(graph_model.case(257, 65)))         # rows longer than one group of 64 lanes
    small = graph_model.case(300, 5)
    nb_small = place(tg._neighbors(small))
    g = place(graph.connectivities(nb, out="torch"))
    return "graph", {
        "connectivities, out=torch": lambda: graph.connectivities(nb, out="torch"),
        "connectivities of host arrays": lambda: graph.connectivities((np.array(small["idx"]), np.array(small["d2"]))),
        "transitions of connectivities": lambda: graph.transitions(g),
        "transitions of neighbours": lambda: graph.transitions(nb_small),
        "diffmap": lambda: graph.diffmap(nb_small, 15),
        "diffmap, out=torch": lambda: graph.diffmap(nb, 5, out="torch")}


def test_graph():
    _thrice(*calls_graph())


def calls_layout(place=_identity):
    import graph_model
    import layout_model
    import test_gpu_layout as tl
    from prosstt_amd import layout
    calls = {}
    for name, c in (((1000, 14), 2), ((257, 65), 3)):
        conn = place(tl._conn_of(graph_model.case(*name)["W"]))
        Y = place(_cuda(np.random.default_rng(c).uniform(-10, 10, (name[0], c)).astype(np.float32)))
        kw = dict(n_epochs=50, a=layout_model.A, b=layout_model.B, seed=3)
        for lanes in tl.LANES:
            calls["%s, c = %d, %d lanes" % (name, c, lanes)] = lambda conn=conn, Y=Y, kw=kw, lanes=lanes: layout.optimize(
                conn, Y, 0, 3, lanes_per_row=lanes, **kw)
    return "layout.optimize", calls


def test_layout_optimize():
    _thrice(*calls_layout())


def calls_tsne(place=_identity):
    import tsne_model
    import test_gpu_tsne as tt
    from prosstt_amd import tsne
    calls = {}
    for case, slab_counts in (((65, 63, 20.0), (3,)), ((300, 90, 30.0), (3, 0))):       # one tile: slabs 2 and 3 are empty
        cs = tsne_model.case(*case)
        nb = place(tt._neighbors(cs["idx"], cs["d2"]))
        aff = place(tt._aff(case))
        calls["affinities %s, out=torch" % (case,)] = lambda nb=nb, case=case: tsne.affinities(nb, case[2], out="torch")
        calls["affinities %s of host arrays" % (case,)] = lambda cs=cs, case=case: tsne.affinities(
            (np.array(cs["idx"]), np.array(cs["d2"])), case[2])
        for c in (2, 3):
            Y = place(_cuda(tsne_model.pca_start(cs["P_panel"], c)))
            for slabs in slab_counts:
                tag = "%s, c = %d, slabs %d" % (case, c, slabs)
                calls["gradient " + tag] = lambda aff=aff, Y=Y, slabs=slabs: tsne.gradient(aff, Y, exaggeration=12.0, slabs=slabs,
                                                                                         _sums=True)
                calls["optimize " + tag] = lambda aff=aff, Y=Y, slabs=slabs: tsne.optimize(aff, Y, 0, 3, exploration=2,
                                                                                         learning_rate=50.0, slabs=slabs)
    return "tsne", calls


def test_tsne():
    _thrice(*calls_tsne())


def calls_dpt(place=_identity):
    import dpt_model
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    dm = place(td._device_run(300, 5)[0])
    root = dpt_model.truth(300, 5)[2]
    return "dpt.dpt", {
        "one branching, slabs 3": lambda: dpt.dpt(dm, root, n_branchings=1, slabs=3, _stages=True),
        "one branching, out=torch": lambda: dpt.dpt(dm, root, 15, n_branchings=1, min_group_size=40, out="torch"),
        "no branching": lambda: dpt.dpt(dm, root)}


def test_dpt():
    _thrice(*calls_dpt())


def calls_cluster(place=_identity):
    import test_gpu_cluster as tc
    from prosstt_amd import _native, cluster
    g = place(tc._connectivities(300, 5))                        # (host arrays: the wrapper moves them)

    def run(path):
        def call():
            try:
                return cluster.louvain(g, path=path)
            except _native.NativeError as exc:                   # (16 lanes may hold no level of the graph whole: the same
                assert "rows are longer" in str(exc)             # refusal in every run, after the same allocations)
                return str(exc)
        return call

    calls = {"path %d" % path: run(path) for path in tc.PATHS}
    calls["out=torch"] = lambda: cluster.louvain(g, 2.0, out="torch")
    return "cluster.louvain", calls


def test_cluster_louvain():
    _thrice(*calls_cluster())
