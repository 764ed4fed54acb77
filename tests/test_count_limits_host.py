"""No GPU: the host side of tests/test_gpu_count_limits.py.  Every generator of that module runs here together with its
model, each case is held to the condition that makes it reach the code it names (conditions, not measurements), every limit
the module names is read from its header under include/, and every model call is timed and printed (DESIGN section 32 has
the figures).  The census is one-directional: a limit the GPU module names must stand in its header with the module's
value; a header's other limits need no row here."""
import os
import re
import time

import numpy as np

import test_gpu_count_limits as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _timed(what, call):
    t0 = time.perf_counter()
    out = call()
    print("%-58s %6.2f s" % (what, time.perf_counter() - t0))
    return out


def _rounds(R):
    return -(-R // cl.TABLE_THREADS)


# ------------------------------------------------------------------------------------------------------------- census

def test_every_limit_the_module_names_stands_in_its_header():
    for name, (header, value) in cl.LIMITS.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        found = re.findall(r"^#define %s\s+(.+?)\s*(?:/\*.*)?$" % name, text, flags=re.M)
        assert len(found) == 1, name
        assert re.fullmatch(r"[0-9()*<+\- ]+", found[0]), (name, found[0])          # integer arithmetic alone
        assert eval(found[0], {"__builtins__": {}}) == value, name
    L = {name: value for name, (_, value) in cl.LIMITS.items()}
    assert cl.MAX_GROUPS == L["PROSSTT_AMD_MARKERS_MAX_GROUPS"] == L["PROSSTT_AMD_RANKS_MAX_GROUPS"] == cl.KS[-1]
    assert cl.TABLE_THREADS == cl.MAX_GROUPS                         # markers.hip: the table kernel's block is kMaxGroups threads
    assert (cl.MAX_NODES, cl.MAX_EDGES) == (L["PROSSTT_AMD_PTREE_MAX_NODES"], L["PROSSTT_AMD_PTREE_MAX_EDGES"])
    assert (cl.MAX_SOURCES, cl.MAX_BATCH, cl.MAX_SLABS) == (L["PROSSTT_AMD_DPT_MAX_SOURCES"], L["PROSSTT_AMD_DPT_MAX_BATCH"],
                                                           L["PROSSTT_AMD_DPT_MAX_SLABS"])
    assert cl.MAX_SLABS == L["PROSSTT_AMD_TSNE_MAX_SLABS"]
    assert max(R for R, _ in cl.MAPPING_CASES) < L["PROSSTT_AMD_MAPPING_MAX_NODES"]
    assert max(c[0] for c in cl.PTREE_HARD) == cl.MAX_NODES and max(c[1] for c in cl.PTREE_PROJECT) == cl.MAX_EDGES
    assert max(n for _, n in cl.DPT_ROWS) == cl.MAX_SOURCES and cl.DPT_BATCH[1] == cl.MAX_BATCH and cl.DPT_SLABS[2] == cl.MAX_SLABS
    assert max(cl.TSNE_SLABS) == cl.MAX_SLABS
    assert cl.KS == (63, 64, 65, 255, 256, 257, 1023, 1024)


# ------------------------------------------------------------------------------------------------------------ markers

def test_markers_cases_reach_the_table_kernels_scan_search_and_second_trip():
    import markers_model as mm
    import test_gpu_markers as tm
    for K in cl.KS:
        N = cl.markers_cells(K)
        assert 1100 <= N <= 2100
        for last in ("full", "empty"):
            codes = cl.group_codes(N, K, last)
            assert codes.shape == (N,) and codes.min() == -1 and codes.max() == (K - 1 if last == "full" else K - 2)
            n = np.bincount(codes[codes >= 0], minlength=K)
            assert (n == 0).sum() >= K // 5 - 1 and (n == 1).sum() >= K // 5 - 1 and n[1] == 0     # empty and single-cell groups
            assert n[0] == n.max() >= 3 * (N - N // 10) // 10 and (codes < 0).sum() == N // 10    # one large group, cells left out
            assert (n[K - 1] > 0) == (last == "full") and n[K - 2 if last == "empty" else K - 1] == 2
            for rpb in cl.markers_rows_per_block(K):
                r = rpb or mm.default_rows_per_block(int(n.sum()), cl.G_SMALL)
                blocks = cl.blocks_of(codes, K, r)
                assert blocks + K <= cl.MAX_GRID_Y
                if K >= 1023 and rpb == 1:                           # K = 1024 with one row per block: the block loop's second trip
                    assert blocks > cl.TABLE_THREADS
    # first_sh[K] is index 1024 only at K = 1024, and K = 1023 fills the offsets' segment to the byte
    assert cl.KS[-1] == cl.TABLE_THREADS and (cl.KS[-2] + 1) * 8 % 256 == 0
    assert int(np.ceil(np.log2(cl.KS[-1]))) == 10                    # the search's steps
    assert sum(K > 64 for K in cl.KS) == 6                           # above 64 groups the scan leaves the first wave
    N, K, labels, rpb = cl.second_trip_case()
    assert K == 3 and cl.TABLE_THREADS < cl.blocks_of(labels, K, rpb) <= cl.MAX_GRID_Y - K
    X, s = tm._host(N, cl.G_SMALL)
    S1, _, n = _timed("markers_model.sums, K = 3, one row per block", lambda: mm.sums(mm.dense(X, s).astype(np.float32), labels, rpb, K))
    assert n.tolist() == [cl.blocks_of(labels, K, rpb) - 1, 0, 1] and not S1[1].any()
    # the models, at the largest case
    K, N = 1024, cl.markers_cells(1024)
    X, s = tm._host(N, cl.G_SMALL)
    A = mm.dense(X, s).astype(np.float32)
    codes = cl.group_codes(N, K, "full")
    S1, S2, n = _timed("markers_model.sums, K = 1024, one row per block", lambda: mm.sums(A, codes, 1, K))
    assert S1.shape == (K, cl.G_SMALL) and n.sum() == N - N // 10
    nz, cs = _timed("test_gpu_markers._integers, K = 1024", lambda: tm._integers(X, codes, K))
    assert nz.shape == (K, cl.G_SMALL) and cs.sum() == X[codes >= 0].astype(np.int64).sum()


# -------------------------------------------------------------------------------------------------------------- ranks

def test_ranks_cases_reach_the_second_trip_of_the_group_loops():
    import markers_model as mm
    import ranks_model as rm
    import test_gpu_ranks as tr
    W = cl.LIMITS["PROSSTT_AMD_RANKS_SORT_TILE"][1]
    seen = set()
    for K in cl.KS:
        n_sel = cl.ranks_selected(K)
        seen.add(n_sel - W)
        labels, N = tr._labels(n_sel, K)
        n = np.bincount(labels[labels >= 0], minlength=K)
        assert n.sum() == n_sel and n[1] == 0 and n[K - 1] == 1 and labels.max() == K - 1
    assert seen == {-1, 0, 1}                                        # below, at and above one tile of the sort
    assert sum(K > 256 for K in cl.KS) >= 3                          # k += 256: a second trip, and four at K = 1024
    assert cl.KS[-1] - 1 > 255                                       # payloads that need the second byte of the uint16
    K = 1024
    labels, N = tr._labels(cl.ranks_selected(K), K)
    for kind in cl.RANKS_KINDS:
        X, s = tr._input(kind, N, cl.G_SMALL)
        A = mm.dense(X, s).astype(np.float32)
        for reference in (None, K - 1, 1):
            Q, T, n = _timed("ranks_model.rank_sums, K = 1024, input %s, reference %s" % (kind, reference),
                             lambda: rm.rank_sums(A, labels, K, reference=reference))
            assert Q.shape == (K, cl.G_SMALL) and (reference != 1 or not Q.any())
            assert reference is not None or Q.sum(0).tolist() == [int(n.sum()) ** 2] * cl.G_SMALL


# ------------------------------------------------------------------------------------------------------------- trends

def test_trends_cases_reach_the_carry_of_the_table_kernel():
    import test_gpu_trends as tt
    import trends_model
    assert [c[0] for c in cl.TRENDS_CASES] == [1023, 1024, 1025, 2047, 2049, 3000] and cl.TRENDS_N == 161
    assert {G for c in cl.TRENDS_CASES for G in c[3]} == {3, 257} and cl.TRENDS_EPB == (0, 1, 64)
    long_rounds = {}
    for R, long_at, empty_at, genes in cl.TRENDS_CASES:
        indptr, indices, weights = cl.trends_csr(R, long_at, empty_at)
        lengths = np.diff(indptr)
        assert len(lengths) == R and lengths[long_at] == cl.TRENDS_LONG and -(-cl.TRENDS_LONG // 64) == 5
        rest = np.delete(lengths, long_at)
        assert rest.max() == 5 and rest.min() == 0 and not lengths[list(empty_at)].any()
        assert indices.min() >= 0 and indices.max() < cl.TRENDS_N and weights.min() == 0 and weights.max() == 4096
        assert (R > cl.TABLE_THREADS) == (_rounds(R) >= 2)
        long_rounds[R] = (long_at // cl.TABLE_THREADS, long_at == R - 1)
        for node in empty_at:
            assert node == 0 or node % cl.TABLE_THREADS == 0 or node == R - 1
        # the library's rule for entries_per_block = 0 gives chunks of 64 here: the long row is cut in five
        nnz = int(indptr[-1])
        assert max(64, -(-nnz * -(-max(genes) // 1024) // 1024)) == 64
        for G in genes:
            X = np.array(cl.trends_counts(G))
            s1, s2 = _timed("trends_model.node_sums and words, R = %d, G = %d" % (R, G), lambda: tt._expected(X, (indptr, indices, weights)))
            assert s1.shape == (R, G) and s2.shape == (R, G, 2) and s2[..., 1].any()
    assert sum(_rounds(R) >= 2 for R in long_rounds) == 4 and _rounds(3000) == 3
    assert long_rounds[1025] == (1, True) and long_rounds[2049] == (1, False) and long_rounds[3000] == (2, True)
    assert any(1024 in c[2] for c in cl.TRENDS_CASES)                # an empty node first in a round
    assert (2047 + 1) * 8 % 256 == 0                                 # R + 1 offsets fill their segment to the byte
    assert trends_model.ONE == 4096


def _first_chunk(indptr, entries_per_block, before_takes_carry=True, carry_adds=True):
    """trends_table_kernel's first_chunk restated: rounds of 1024 nodes, an inclusive scan within a round, ``before = carry +
    scan[k] - nb`` and ``carry += scan[1023]``; the two switches break those two lines (no carry in ``before``; ``=`` for
    ``+=``)."""
    nb = -(-np.diff(indptr) // entries_per_block)
    R = len(nb)
    out, carry = np.zeros(R + 1, dtype=np.int64), 0
    for base in range(0, R, cl.TABLE_THREADS):
        part = nb[base:base + cl.TABLE_THREADS]
        scan = np.cumsum(part)
        out[base:base + len(part)] = (carry if before_takes_carry else 0) + scan - part
        carry = int(scan[-1]) + (carry if carry_adds else 0)
    out[R] = carry
    return out


def test_a_broken_carry_shows_at_these_node_counts_and_at_none_of_the_older_ones():
    """On a restatement, not on the device (a table that is wrong sends the pass to entries nobody wrote): with ``before``
    without the carry, or with ``carry =`` for ``carry +=``, the chunk table differs from the running sum of the chunks
    exactly where R > 1024 (the second break shows in first_chunk[R] after two rounds and in ``before`` from the third);
    test_gpu_trends' own RS = (1, 5, 40) cannot tell."""
    import test_gpu_trends as tt
    cases = [(cl.trends_csr(R, long_at, empty_at)[0], R) for R, long_at, empty_at, _ in cl.TRENDS_CASES]
    cases += [(tt._csr(R, 161, np.random.default_rng(R))[0], R) for R in tt.RS]
    for indptr, R in cases:
        for epb in (1, 64):
            truth = np.concatenate([[0], np.cumsum(-(-np.diff(indptr) // epb))])
            assert np.array_equal(_first_chunk(indptr, epb), truth)
            for broken in (dict(before_takes_carry=False), dict(carry_adds=False)):
                assert np.array_equal(_first_chunk(indptr, epb, **broken), truth) == (_rounds(R) == 1), (R, epb, broken)


# -------------------------------------------------------------------------------------------------------------- ptree

def test_ptree_cases_reach_many_tiles_of_centres_and_many_trips_over_the_edges():
    import ptree_model as pm
    assert sorted({c[0] for c in cl.PTREE_HARD}) == [1023, 1024, 1025, 4096]
    assert {c[1] for c in cl.PTREE_HARD} == {65, 257} and {c[2] for c in cl.PTREE_HARD} == {3, 33}
    assert sorted({c[1] for c in cl.PTREE_PROJECT}) == [4095, 8191, 8192]
    for R, N, d in cl.PTREE_HARD:
        Y, C = cl.ptree_hard_inputs(R, N, d)
        want = _timed("ptree_model.assign, hard, R = %d, N = %d, d = %d" % (R, N, d), lambda: pm.assign(Y, C, 0.0))
        assert np.array_equal(C[R - cl.PTREE_TIES:], C[:cl.PTREE_TIES]) and (R - cl.PTREE_TIES) // 64 > cl.PTREE_TIES // 64
        assert np.all(want.best[:30] < cl.PTREE_TIES) and np.all(want.sq_distance[:30] == 0)
        assert want.gamma.sum() == N and -(-R // 32) >= 32           # 32 to 128 blocks of nodes in the sums kernel
    for R, N, d in cl.PTREE_SOFT:
        assert R & (R - 1) == 0                                      # a power of two: 1 / R is exact
        rng = np.random.default_rng(R + d)
        Y = rng.standard_normal((N, d)).astype(np.float32)
        C = np.repeat(rng.standard_normal((1, d)).astype(np.float32), R, axis=0)
        want = _timed("ptree_model.assign, soft, R = %d, N = %d, d = %d" % (R, N, d), lambda: pm.assign(Y, C, 0.7))
        assert np.all(want.resp == 1.0 / R)
    for R, E, N, d in cl.PTREE_PROJECT:
        Y, C, edges = cl.ptree_project_inputs(R, E, N, d)
        assert edges.shape == (E, 2) and edges.min() >= 0 and edges.max() < R and -(-E // 64) >= 64
        assert edges[0, 0] == edges[0, 1] and np.array_equal(edges[E - 1], edges[2]) and np.array_equal(edges[E // 2], edges[3])
        want = _timed("ptree_model.project, R = %d, E = %d, N = %d, d = %d" % (R, E, N, d), lambda: pm.project(Y, C, edges))
        assert want.edge.max() >= 64 and not np.any(want.edge == E - 1)


# ------------------------------------------------------------------------------------------------------------ mapping

def test_mapping_cases_reach_many_node_tiles_and_a_best_node_in_each_part():
    import mapping_model as mm
    assert sorted({R for R, _ in cl.MAPPING_CASES}) == [1023, 1025, 2049] and {G for _, G in cl.MAPPING_CASES} == {33, 257}
    for R, G in cl.MAPPING_CASES:
        X, s, P, m, c, offsets = cl.mapping_inputs(R, G)
        assert X.shape == (cl.MAPPING_N, G) and P.shape == (R, G) and offsets[-1] == R and -(-R // 32) >= 32
        first, middle, last = cl.mapping_targets(R)
        assert first // 32 == 0 and last // 32 == (R - 1) // 32 and 0 < middle // 32 < (R - 1) // 32
        assert np.abs(mm.gene_sums(X, P)).max() < 2 ** 13 and np.abs(s[:, None] * m[None, :]).max() < 1e4
        for node in (first, middle, last):
            S = _timed("mapping_model.scores and best, R = %d, G = %d" % (R, G),
                       lambda: mm.scores(X, s, P, m, cl.with_best_node(c, node)))
            assert np.all(mm.best(S) == node)


# ---------------------------------------------------------------------------------------------------------------- dpt

def test_dpt_cases_reach_the_grid_limits():
    import dpt_model
    import test_gpu_dpt as td
    assert {N for N, _ in cl.DPT_ROWS} == {3, 5} and {n for _, n in cl.DPT_ROWS} == {1024, 65535}
    for N, n in cl.DPT_ROWS:
        dm = td._random_map(N, 2)
        src = cl.dpt_sources(N, n)
        assert src.shape == (n,) and src.min() == 0 and src.max() == N - 1
        for n_dcs in (1, 2):
            d = _timed("dpt_model.rows, %d cells, %d sources, n_dcs %d" % (N, n, n_dcs),
                       lambda: dpt_model.rows(dm.eigenvectors, dpt_model.weights(dm.eigenvalues, n_dcs), src))
            assert d.shape == (n, N) and np.all(d[np.arange(n), src] == 0)
    assert cl.DPT_BATCH == (257, 1024, 1) and cl.DPT_SLABS == (1000, 1, 1024)
    seq = _timed("dpt_model.concordance, 1024 pairs of 257, two kinds", cl.dpt_batch_sequences)
    for kind, (ru, rv, lower, upper) in seq.items():
        assert ru.shape == (1024, 257) and lower.shape == (1024, 257)
        assert len({ru[b].tobytes() for b in range(1024)}) == 1024                  # every pair its own
    N, batch, slabs = cl.DPT_SLABS
    assert -(-N // 256) == 4 and slabs - 4 == 1020                   # 1020 slabs without a tile
    _timed("test_gpu_dpt._sequences(1000, 1), five kinds", lambda: td._sequences(N, batch))
    assert 1024 * 1024 * 2 * 257 * 4 > 2 ** 31                       # the joint maximum's workspace: left out


# --------------------------------------------------------------------------------------------------------------- tsne

def test_tsne_case_leaves_all_but_two_slabs_empty():
    import tsne_model
    assert cl.TSNE_CASE == (300, 90, 30.0) and cl.TSNE_SLABS == (64, 1024) and -(-300 // tsne_model.TILE) == 2
    P = _timed("tsne_model.case(300, 90, 30.0)", lambda: tsne_model.case(*cl.TSNE_CASE))["P"]
    for c in (2, 3):
        for Y in cl.tsne_positions(c):
            want = _timed("tsne_model.gradient, c = %d" % c, lambda: tsne_model.gradient(P, Y, 12.0, sums=True))
            assert want.grad.shape == (300, c) and np.abs(want.grad).max() > 0
