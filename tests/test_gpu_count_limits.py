"""-m gpu: the dimension that COUNTS things, up to its declared limit.  Every library's suite sweeps cells and genes across the
wave, strip and tile boundaries; groups, nodes, edges, sources, batch entries and slabs stayed small.  Here they run at the
wave (63/64/65), the block (255/256/257) and the table kernel's width (1023/1024/1025) and at the limit each header declares,
over few cells and genes, against each library's own model by each library's own criterion (imported from its GPU test
module: nothing is restated).  tests/test_count_limits_host.py runs every generator and model below without a GPU, asserts
that each case reaches the code it names, and reads every limit below from its header.

The audit: every loop, scan, table and grid extent that depends on the count, and what bounds it (read in the sources before
anything ran; K, R, E, ... are at most the limit in every line, the wrappers refuse more: check_sizes of each library).

  markers   markers_table_kernel   one block of kMaxGroups = 1024 threads, thread k is group k.
                                   scan[1024], lo_sh[1024], hi_sh[1024]: indexed by threadIdx.x < 1024, written for k < K
                                   first_sh[1024 + 1]: [k] for k < K, [K] by thread K - 1; K <= 1024, so index 1024 at most
                                   the scan's 10 rounds read scan[k - off], k >= off
                                   first_block[K + 1]: geometry's pad((K + 1) * 8) at first_at
                                   for (b = k; b < total; b += kMaxGroups): total = first_sh[K] <= max_blocks, and
                                   table[b] has max_blocks entries (pad(max_blocks * 16)); the search keeps left in [0, K)
            markers_pass_kernel    grid.y = max_blocks = ceil(n_sel / r) + K <= 65535 (check_sizes); a block at or past
                                   *block_count returns; slabs [max_blocks][G] at (size_t)blockIdx.y * G
            markers_finish_kernel  grid.y = K <= 1024; first_block[k], [k + 1], k < K; outputs [K][G] at k * G + g
  ranks     ranks_emit_kernel      for (k = tid; k < K; k += 256) reads group_start[k], [k + 1]: K + 1 entries
                                   the search over group_start keeps left in [0, K): the payload is a group below K <= 1024
                                   and fits uint16; group_sh[16] by tid < nrows <= 16
            ranks_fold_kernel      q_sh[kMaxGroups = 1024]: for (k = tid; k < K; k += 256), and atomicAdd at
                                   group < K ? group : 0; Q[k * G + gene], k < K, int64 products
  trends    trends_table_kernel    one block of 1024 threads, rounds of 1024 nodes: scan[1024] by threadIdx.x;
                                   indptr[r], [r + 1] only for r < R; first_chunk[R + 1] (pad((R + 1) * 8)): [r] for r < R,
                                   [R] by thread 0 after the last round; carry += scan[1023] after every round;
                                   table[before + c] only while before + c < max_chunks = ceil(nnz / e) + R entries
            trends_pass_kernel     grid.x = max_chunks < 2^31; a block at or past first_chunk[R] returns; first_chunk[node + 1]
                                   with node < R; a node of one chunk stores to S1 / S2 at node * G, the others to slabs at
                                   (size_t)blockIdx.x * G, [max_chunks][G]
            trends_finish_kernel   grid.x = R < 2^31, first_chunk[r], [r + 1]
  ptree     ptree_distance_kernel  grid.y = ceil(R / 64) <= 64; centres past R are zeros in LDS, D[i * R + k] only for k < R
            ptree_cell_kernel      for (k = lane; k < R; k += 64) over the row D + cell * R (int64), the key holds k in 32
                                   bits; resp + cell * R the same
            ptree_sums_kernel      grid.y = ceil(R / 32) <= 128; a lane past R reads node R - 1 and stores nothing;
                                   part[(chunk * R + k) * (d + 1)] within layout()'s ceil(N / 128) * R * (d + 1) doubles
            ptree_fold_kernel      one thread per j < R * (d + 1)
            ptree_project_kernel   for (e = lane; e < E; e += 64) reads edges[2 e], [2 e + 1]; a node outside [0, R) is
                                   skipped and reported; no table, no LDS
  mapping   mapping_pass_kernel    grid.y = ceil(R / (32 NT)) <= 65535 since R <= 65535 * 32; panel rows, exposure,
                                   constant and S[row * R + node] only for node < R
            mapping_finish_kernel  for (r = lane; r < R; r += 64) over S + cell * R; the index is kept in an int: R < 2^31
  dpt       dpt_rows_kernel        grid.y = n_sources <= 65535; sources[blockIdx.y]; out[blockIdx.y * N + j] in int64
            dpt_concordance_kernel grid = (row blocks, slabs <= 1024, batch <= 1024); u, v at pair * N; a slab past the
                                   last tile has tile_begin >= tile_end = tiles and stores its zeros;
                                   part[((pair * slabs + slab) * 2 [+ 1]) * N + row] within batch * slabs * 2 * N int32
            dpt_reduce_kernel      grid.y = batch; for (s = 0; s < slabs; ++s) over the same layout
                                   (the joint maximum batch = slabs = 1024 needs a workspace of 2 GB at N = 257 and is left
                                   out: each extent runs at its limit with the other at 1)
  tsne      tsne_pair_kernel       grid.y = slabs <= 1024; an empty slab stores +0.0; zpart[slab * N + row],
                                   rpart[(slab * N + row) * C + c] within make_plan's slabs * N * 8 (* C) bytes
            tsne_zsum_kernel,      for (s = 0; s < slabs; ++s) over the same layouts.  A tile's binary32 sums are added
            tsne_row_kernel        to binary64 in ascending tile order from 0.0, within a slab or across slabs alike,
                                   and an empty slab adds +0.0: the bytes do not depend on the slab count

No index was found to leave its array at an admissible count, and no run found one.  Of the older suites only
tests/test_gpu_ranks.py::test_inputs_groups_and_references ran a count at its limit, K = 1024 (so the k += 256 loops and
payloads up to 1023 had run; the group counts between 7 and 1024, the last group and an empty group as reference at those
counts, and two passes had not); every other count stayed at 400 or below (DESIGN section 32 has the table).

Where a store one entry past a table lands.  first_block (K + 1 entries) and first_chunk (R + 1) are the FIRST segment of
one workspace, padded to 256 bytes: a store into entry K + 1 lies in that padding, not at a guard band, unless
(K + 1) * 8 is a multiple of 256.  K = 1023 and R = 2047 are such counts: there entry K + 1 is the first word of the next
segment, table[0], and block 0's sums show it.  Both are among the cases and the guarded calls for that reason.  The
outputs [K][G], [R][G] and the last slab of every workspace do end at a band."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# every limit the cases use -> (header under include/, value): tests/test_count_limits_host.py reads them from the headers
LIMITS = {
    "PROSSTT_AMD_MARKERS_MAX_GROUPS": ("prosstt_amd_markers.h", 1024),
    "PROSSTT_AMD_RANKS_MAX_GROUPS": ("prosstt_amd_ranks.h", 1024),
    "PROSSTT_AMD_RANKS_SORT_TILE": ("prosstt_amd_ranks.h", 1024),
    "PROSSTT_AMD_PTREE_MAX_NODES": ("prosstt_amd_ptree.h", 4096),
    "PROSSTT_AMD_PTREE_MAX_EDGES": ("prosstt_amd_ptree.h", 8192),
    "PROSSTT_AMD_MAPPING_MAX_NODES": ("prosstt_amd_mapping.h", 65535 * 32),
    "PROSSTT_AMD_DPT_MAX_SOURCES": ("prosstt_amd_dpt.h", 65535),
    "PROSSTT_AMD_DPT_MAX_BATCH": ("prosstt_amd_dpt.h", 1024),
    "PROSSTT_AMD_DPT_MAX_SLABS": ("prosstt_amd_dpt.h", 1024),
    "PROSSTT_AMD_TSNE_MAX_SLABS": ("prosstt_amd_tsne.h", 1024),
}
MAX_GROUPS, MAX_NODES, MAX_EDGES = 1024, 4096, 8192
MAX_SOURCES, MAX_BATCH, MAX_SLABS = 65535, 1024, 1024
TABLE_THREADS = 1024                        # the one block of markers_table_kernel and of trends_table_kernel
MAX_GRID_Y = 65535

KS = (63, 64, 65, 255, 256, 257, 1023, 1024)
G_SMALL = 5


def _same_bytes(a, b, what):
    from test_gpu_stale_memory import _flatten
    a, b = _flatten(a), _flatten(b)
    assert sorted(a) == sorted(b) and len(a) > 0, what
    for path in a:
        assert a[path] == b[path], "%s: %s differs" % (what, path)


# ------------------------------------------------------------------------------------------------------------ markers

def markers_cells(K):
    return 1100 if K < 1023 else 2100


def group_codes(N, K, last):
    """One code in [-1, K) per cell: a tenth of the cells left out, group 0 large (three tenths of the rest and more), the
    groups k = 1 mod 5 empty, the groups k = 2 mod 5 a single cell, the others a few cells each; ``last`` = "full": group
    K - 1 has two cells, "empty": group K - 1 has none and group K - 2 has two."""
    rng = np.random.default_rng(7 * N + K + (last == "empty"))
    top = K - 1 if last == "full" else K - 2
    singles = [k for k in range(1, top) if k % 5 == 2]
    few = [k for k in range(1, top) if k % 5 not in (1, 2)]
    pool = rng.permutation(N)[N // 10:]
    assert len(singles) + 2 + len(few) < len(pool) // 2
    codes = np.full(N, -1, dtype=np.int64)
    at = 0
    codes[pool[:len(singles)]] = singles
    at += len(singles)
    codes[pool[at:at + 2]] = top
    at += 2
    big = 3 * len(pool) // 10
    codes[pool[at:at + big]] = 0
    at += big
    codes[pool[at:at + len(few)]] = few                              # every such group has a cell
    at += len(few)
    codes[pool[at:]] = np.asarray(few + [0])[rng.integers(0, len(few) + 1, size=len(pool) - at)]
    return codes


def markers_rows_per_block(K):
    """0 (the library's rule) and a small block: 1 at the table's width, where the blocks then exceed the table's threads."""
    return (0, 1) if K >= 1023 else (0, 7)


def blocks_of(codes, K, rows_per_block):
    """The blocks of the grouped pass: sum over the groups of ceil(n_k / rows_per_block)."""
    n = np.bincount(codes[codes >= 0], minlength=K)
    return int((-(-n // rows_per_block)).sum())


def second_trip_case():
    """(N, K, labels, rows_per_block): test_gpu_markers' labels of three groups over 2100 cells, one row per block."""
    import test_gpu_markers as tm
    return 2100, 3, tm._labels(2100, 3), 1


def _markers_abi(X, s, codes, K, rows_per_block):
    """The grouped pass through the C ABI, with K given (the wrapper takes K from the largest label: its last group is never
    empty): (nonzero, count_sum, s1, s2) as host arrays, the row list and the offsets by the wrapper's own helper."""
    import torch
    from prosstt_amd import _native, embed, markers
    from prosstt_amd.device import _ptr
    op = embed.LogNormalized(X, s)
    N, G = op.shape
    L = _native.load("markers")
    n, rows, start = markers._row_list(codes, K, None, op.device)
    n_sel = int(n.sum())
    need = ctypes.c_uint64(0)
    _native.check(L.prosstt_amd_markers_workspace_bytes(n_sel, G, K, rows_per_block, ctypes.byref(need)), "markers")
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    out = [torch.empty((K, G), dtype=t, device="cuda") for t in (torch.int64, torch.int64, torch.float64, torch.float64)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.check(L.prosstt_amd_markers_group_moments(None, _ptr(op.counts), N, G, op.ld, _ptr(op.inv_size), _ptr(rows), n_sel,
                                                      _ptr(start), K, rows_per_block, _ptr(ws), need.value,
                                                      *[_ptr(o) for o in out], _ptr(status)), "markers")
    assert int(status.item()) == 0
    return [o.cpu().numpy() for o in out]


def _check_markers(got, X, A, codes, K, rpb, G, what):
    import markers_model as mm
    import test_gpu_markers as tm
    nz, cs, s1, s2 = got
    want_nz, want_cs = tm._integers(X, codes, K)
    assert np.array_equal(nz, want_nz) and np.array_equal(cs, want_cs), what
    S1, S2, _ = mm.sums(A, codes, rpb or mm.default_rows_per_block(int((codes >= 0).sum()), G), K)
    assert tm._same_bits(s1, S1) and tm._same_bits(s2, S2), what


@pytest.mark.parametrize("last", ["full", "empty"])
@pytest.mark.parametrize("K", KS)
def test_markers_group_moments(K, last):
    import test_gpu_markers as tm
    from prosstt_amd import markers
    N, G = markers_cells(K), G_SMALL
    X, s = tm._host(N, G)
    A = tm._a32(N, G)
    codes = group_codes(N, K, last)
    for view in tm.VIEWS:
        for rpb in markers_rows_per_block(K):
            what = (K, last, view, rpb)
            if last == "full":                                       # through the wrapper: K is the largest label + 1
                gm = markers.group_moments(tm._view(N, G, view), s, codes, rows_per_block=rpb)
                assert len(gm.groups) == K and np.array_equal(gm.n, np.bincount(codes[codes >= 0], minlength=K))
                got = (gm.nonzero, gm.count_sum, gm.s1, gm.s2)
            else:
                got = _markers_abi(tm._view(N, G, view), s, codes, K, rpb)
                assert not got[0][K - 1].any() and not got[2][K - 1].any()           # the empty last group gives zeros
            _check_markers(got, X, A, codes, K, rpb, G, what)
            assert not got[1][1].any() and not got[3][1].any()       # group 1 is empty


def test_markers_table_takes_a_second_trip_over_its_blocks():
    """More blocks than the table kernel has threads, with three groups: thread k also writes table[k + 1024]."""
    import test_gpu_markers as tm
    from prosstt_amd import markers
    N, K, labels, rpb = second_trip_case()
    assert TABLE_THREADS < blocks_of(labels, K, rpb) <= MAX_GRID_Y - K
    X, s = tm._host(N, G_SMALL)
    for view in tm.VIEWS:
        gm = markers.group_moments(tm._view(N, G_SMALL, view), s, labels, rows_per_block=rpb)
        _check_markers((gm.nonzero, gm.count_sum, gm.s1, gm.s2), X, tm._a32(N, G_SMALL), labels, K, rpb, G_SMALL, view)


# -------------------------------------------------------------------------------------------------------------- ranks

RANKS_KINDS = ("a", "b")                    # test_gpu_ranks' inputs: distinct keys, and long runs of ties


def ranks_selected(K):
    """n_sel around the sort's tile of 1024 positions."""
    return (1023, 1024, 1025)[KS.index(K) % 3] if K < 1023 else 1025


@pytest.mark.parametrize("K", KS)
def test_ranks_rank_sums(K):
    import test_gpu_ranks as tr
    from prosstt_amd import ranks
    assert tr._w() == LIMITS["PROSSTT_AMD_RANKS_SORT_TILE"][1]
    G = G_SMALL
    labels, N = tr._labels(ranks_selected(K), K)
    for kind in RANKS_KINDS:
        s = tr._input(kind, N, G)[1]
        for view in tr.VIEWS:
            X = tr._view(kind, N, G, view)
            # every labelled cell, the last group (a single cell) and the empty group 1 as the counting set
            for index, reference in ((None, "rest"), (K - 1, K - 1), (1, 1)):
                rs = ranks.rank_sums(X, s, labels, reference=reference)
                tr._check(rs, tr._want(kind, N, G, labels, K, index), K)
                if index == 1:
                    assert rs.n[1] == 0 and not rs.q.any()
                two = ranks.rank_sums(X, s, labels, reference=reference, genes_per_pass=3)
                _same_bytes((two.q, two.ties), (rs.q, rs.ties), (K, kind, view, reference, "two passes"))


# ------------------------------------------------------------------------------------------------------------- trends

TRENDS_N, TRENDS_LONG = 161, 300
# (R, the node of the long row, nodes emptied, the gene counts): the long row as the last node of the only round (1023,
# 1024), as the first node of the second round and the last node (1025), inside the second round behind an empty first node
# of that round (2047, 2049), as the last node of the third round (3000)
TRENDS_G = (3, 257)
TRENDS_CASES = ((1023, 1022, (0,), TRENDS_G), (1024, 1023, (), TRENDS_G), (1025, 1024, (), TRENDS_G),
                (2047, 1500, (1024, 2046), TRENDS_G), (2049, 1500, (1024, 2048), TRENDS_G), (3000, 2999, (1024, 2048), TRENDS_G))
TRENDS_EPB = (0, 1, 64)


def trends_csr(R, long_at, empty_at):
    """Rows of 0 to 5 entries and one of TRENDS_LONG (five chunks of 64); cells and weights as test_gpu_trends._csr draws
    them: repeated cells, weights 0 .. 4096 with zeros and 4096 among them."""
    rng = np.random.default_rng(31 * R + long_at)
    lengths = rng.integers(0, 6, size=R)
    lengths[long_at] = TRENDS_LONG
    lengths[list(empty_at)] = 0
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, TRENDS_N, nnz).astype(np.int32)
    weights = rng.integers(0, 4097, nnz).astype(np.int32)
    weights[rng.random(nnz) < 0.1] = 0
    weights[rng.random(nnz) < 0.1] = 4096
    return indptr, indices, weights


@functools.lru_cache(maxsize=None)
def trends_counts(G):
    import test_gpu_trends as tt
    X = tt._counts(TRENDS_N, G, "big", np.random.default_rng(161 * G))
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("R,long_at,empty_at,genes", TRENDS_CASES)
def test_trends_node_sums(R, long_at, empty_at, genes):
    import test_gpu_trends as tt
    from prosstt_amd import trends
    csr = trends_csr(R, long_at, empty_at)
    w = tt._weights(csr, TRENDS_N)
    for G in genes:
        X = np.array(trends_counts(G))
        s1, s2 = tt._expected(X, csr)
        base = None
        for turn, epb in enumerate(TRENDS_EPB):
            got = trends.node_sums(tt._view(X, tt.LAYOUTS[(turn + G) % 3]), w, entries_per_block=epb)
            assert np.array_equal(got.s1, s1) and np.array_equal(got.s2_words, s2), (R, G, epb)
            base = got if base is None else base
            assert tt._bytes(got) == tt._bytes(base), (R, G, epb)
        assert not s1[list(empty_at)].any() and s1[long_at].any()


# -------------------------------------------------------------------------------------------------------------- ptree

# (R, N, d) of the hard pass; at R = 4096 on the three layouts
PTREE_HARD = ((1023, 65, 3), (1024, 257, 33), (1025, 65, 33), (4096, 257, 3), (4096, 65, 33))
PTREE_SOFT = ((1024, 257, 33), (4096, 65, 3))                       # powers of two: r = 1 / R and every r * y are exact
# (R, E, N, d) of the projection
PTREE_PROJECT = ((1023, 4095, 65, 33), (1025, 8191, 257, 3), (4096, 8192, 257, 3), (4096, 8192, 65, 33))
PTREE_TIES = 40


def ptree_hard_inputs(R, N, d):
    """Coordinates in eighths (every sum exact); the last PTREE_TIES centres repeat the first, 64-wide tiles apart, and the
    first 30 cells lie on such a centre: the lower index must win."""
    import ptree_model as pm
    Y, C = pm.eighths(N, d, 100 * R + d, span=16), pm.eighths(R, d, 100 * R + d + 1, span=16)
    C[R - PTREE_TIES:] = C[:PTREE_TIES]
    Y[:30] = C[R - PTREE_TIES + np.arange(30)]
    return Y, C


def ptree_edges(R, E):
    """Random edges with a zero-length edge, repeated edges and an edge between the first and the last node."""
    rng = np.random.default_rng(R + E)
    edges = np.stack([rng.integers(0, R, size=E), rng.integers(0, R, size=E)], axis=1).astype(np.int32)
    edges[0] = (1, 1)
    edges[E - 1] = edges[2]
    edges[E // 2] = edges[3]
    edges[E - 2] = (0, R - 1)
    return edges


def ptree_project_inputs(R, E, N, d):
    rng = np.random.default_rng(R * 7 + E + d)
    return (rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((R, d)).astype(np.float32), ptree_edges(R, E))


@pytest.mark.parametrize("R,N,d", PTREE_HARD)
def test_ptree_hard_pass(R, N, d):
    import ptree_model as pm
    import test_gpu_ptree as tp
    from prosstt_amd import ptree
    Y, C = ptree_hard_inputs(R, N, d)
    want = pm.assign(Y, C, 0.0)
    assert np.all(want.best[:30] < PTREE_TIES) and (R - PTREE_TIES) // 64 > PTREE_TIES // 64
    for turn, layout in enumerate(tp.LAYOUTS if R == MAX_NODES else tp.LAYOUTS[R % 3:R % 3 + 1]):
        got = ptree.assign(tp._view(Y, layout), tp._view(C, tp.LAYOUTS[(turn + 1) % 3]), 0.0, responsibilities=True)
        tp._assert_hard(got, want, (R, N, d, layout))
        assert tp._same_bits(got.resp, want.resp)
        assert np.array_equal(got.gamma, np.bincount(want.best, minlength=R).astype(np.float64))


@pytest.mark.parametrize("R,N,d", PTREE_SOFT)
def test_ptree_soft_pass_where_it_is_exact(R, N, d):
    """Every centre is the same point (test_gpu_ptree's construction): w = 1, Z = R, r = 1 / R exactly."""
    import ptree_model as pm
    import test_gpu_ptree as tp
    from prosstt_amd import ptree
    rng = np.random.default_rng(R + d)
    Y = rng.standard_normal((N, d)).astype(np.float32)
    C = np.repeat(rng.standard_normal((1, d)).astype(np.float32), R, axis=0)
    want, got = pm.assign(Y, C, 0.7), ptree.assign(tp._view(Y, "shifted"), C, 0.7, responsibilities=True)
    assert np.all(got.resp == 1.0 / R) and not got.best.any()
    assert tp._same_bits(got.resp, want.resp) and tp._same_bits(got.gamma, want.gamma) and tp._same_bits(got.sums, want.sums)
    assert np.all(got.gamma == N / R)
    assert np.all(np.abs(got.free_energy - want.free_energy) <= pm.soft_bound(Y, C, 0.7, want)[0])


@pytest.mark.parametrize("R,E,N,d", PTREE_PROJECT)
def test_ptree_projection(R, E, N, d):
    import ptree_model as pm
    import test_gpu_ptree as tp
    from prosstt_amd import ptree
    Y, C, edges = ptree_project_inputs(R, E, N, d)
    want = pm.project(Y, C, edges)
    for layout in (tp.LAYOUTS if R == MAX_NODES else tp.LAYOUTS[E % 3:E % 3 + 1]):
        got = ptree.project(tp._view(Y, layout), tp._view(C, layout), edges)
        assert got.edge.dtype == np.int32 and np.array_equal(got.edge, want.edge), (R, E, layout)
        assert tp._same_bits(got.t, want.t) and tp._same_bits(got.sq_distance, want.sq_distance), (R, E, layout)
    assert not np.any(got.edge == E - 1) and not np.any(got.edge == E // 2)                   # a repeat never beats the original


# ------------------------------------------------------------------------------------------------------------ mapping

MAPPING_N = 33
MAPPING_CASES = ((1023, 33), (1025, 257), (2049, 33), (2049, 257))  # (R, G)


def mapping_inputs(R, G):
    import test_gpu_mapping as tg
    rng = np.random.default_rng(9000 + R + G)
    X, s, P, m, c = tg._exact_inputs(MAPPING_N, G, R, rng)
    return X, s, P, m, c, tg._offsets(R, rng)


def mapping_targets(R):
    """The node that is made the best of every cell: in the first tile of 32 nodes, in a middle tile, in the last tile."""
    return (3, 32 * (R // 64) + 17, R - 1)


def with_best_node(c, node):
    """The constants with ``node`` raised above every other score (|D| < 2^13 and |s m| stays far below 10^6 here)."""
    out = np.array(c)
    out[node] += 1.0e6
    return out


@pytest.mark.parametrize("R,G", MAPPING_CASES)
def test_mapping_node_scores(R, G):
    import test_gpu_mapping as tg
    from prosstt_amd import mapping
    X, s, P, m, c, offsets = mapping_inputs(R, G)
    views = {layout: tg._view(X, layout) for layout in tg.LAYOUTS}
    for turn, node in enumerate(mapping_targets(R)):
        cn = with_best_node(c, node)
        base = mapping.node_scores(views["aligned"], s, P, m, cn, offsets, scores=True)
        tg._assert_against_model(base, X, s, P, m, cn, offsets, 256, (R, G, node), exact=True)
        assert np.all(base.best == node)
        for tile in (1, 2, 3, 4):                                    # the tiled entry point: 32, 64, 96 and 128 nodes a block
            other = mapping.node_scores(views[tg.LAYOUTS[(tile + turn) % 3]], s, P, m, cn, offsets, scores=True, node_tile=tile,
                                        genes_per_chain=32)
            assert tg._bytes(other) == tg._bytes(base), (R, G, node, tile)
    plain = mapping.node_scores(views["shifted"], s, P, m, c, offsets, scores=True)          # and no planted node
    tg._assert_against_model(plain, X, s, P, m, c, offsets, 256, (R, G), exact=True)


# ---------------------------------------------------------------------------------------------------------------- dpt

DPT_ROWS = ((3, 1024), (5, 1024), (3, MAX_SOURCES), (5, MAX_SOURCES))           # (cells, sources)
DPT_BATCH, DPT_SLABS = (257, MAX_BATCH, 1), (1000, 1, MAX_SLABS)               # (N, batch, slabs)


def dpt_sources(N, n):
    src = np.random.default_rng(N + n).integers(0, N, size=n)
    src[[0, n - 1]] = (N - 1, 0)
    return src


@functools.lru_cache(maxsize=None)
def dpt_batch_sequences():
    """{kind: (ru, rv, lower, upper)} of 1024 sequence pairs, every pair its own: permutations, and four values (ties)."""
    import dpt_model
    N, batch, _ = DPT_BATCH
    rng = np.random.default_rng(N + batch)
    perm = [np.stack([rng.permutation(N) for _ in range(batch)]).astype(np.int32) for _ in range(2)]
    pairs = {"permutations": tuple(perm), "four values": tuple(rng.integers(0, 4, (batch, N)).astype(np.int32) for _ in range(2))}
    return {kind: (ru, rv) + dpt_model.concordance(ru, rv) for kind, (ru, rv) in pairs.items()}


@pytest.mark.parametrize("N,n_sources", DPT_ROWS)
def test_dpt_rows_of_many_sources(N, n_sources):
    import dpt_model
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    dm = td._random_map(N, 2)
    src = dpt_sources(N, n_sources)
    for n_dcs in (1, 2):
        want = dpt_model.rows(dm.eigenvectors, dpt_model.weights(dm.eigenvalues, n_dcs), src)
        got = dpt.distances(dm, src, n_dcs)
        assert got.shape == (n_sources, N) and got.dtype == np.float64
        print("(%d cells, %d sources), n_dcs %d: largest error %.3g ulp" % (N, n_sources, n_dcs,
                                                                            dpt_model.ulp_distance(got, want).max()))
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
        assert np.all(got[np.arange(n_sources), src] == 0)


def test_dpt_concordance_of_1024_pairs():
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    for kind, (ru, rv, lower, upper) in dpt_batch_sequences().items():
        got_lower, got_upper = dpt.concordance(td._cuda(ru), td._cuda(rv), DPT_BATCH[2])
        assert np.array_equal(got_lower.cpu().numpy(), lower) and np.array_equal(got_upper.cpu().numpy(), upper), kind


def test_dpt_concordance_over_1024_slabs():
    """Four tiles of columns: 1020 slabs are empty and add their zeros."""
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    N, batch, slabs = DPT_SLABS
    for kind in td.KINDS:
        ru, rv, lower, upper = td._sequences(N, batch)[kind]
        got_lower, got_upper = dpt.concordance(td._cuda(ru), td._cuda(rv), slabs)
        assert np.array_equal(got_lower.cpu().numpy(), lower) and np.array_equal(got_upper.cpu().numpy(), upper), kind


# --------------------------------------------------------------------------------------------------------------- tsne

TSNE_CASE, TSNE_SLABS = (300, 90, 30.0), (64, MAX_SLABS)


def tsne_positions(c):
    """Two tiles of columns: positions spread over a few units, and the same with half of the rows on one point."""
    Y = np.random.default_rng(300 + c).normal(0.0, 3.0, (TSNE_CASE[0], c)).astype(np.float32)
    packed = Y.copy()
    packed[150:] = packed[3]
    return Y, packed


@pytest.mark.parametrize("c", [2, 3])
def test_tsne_gradient_over_many_slabs(c):
    """The sums are order-free over the slabs (the module docstring): the bytes of slabs = 1, which the library's own
    criterion holds against the model."""
    import test_gpu_tsne as tt
    from prosstt_amd import tsne
    for Y in tsne_positions(c):
        tt._check_gradient(TSNE_CASE, Y, 12.0, [0.0, 0.0])           # slabs 1, 2, 3 and the library's choice, by the model
        Yd = tt._cuda(Y)
        one = tsne.gradient(tt._aff(TSNE_CASE), Yd, exaggeration=12.0, slabs=1, _sums=True)
        for slabs in TSNE_SLABS:
            many = tsne.gradient(tt._aff(TSNE_CASE), Yd, exaggeration=12.0, slabs=slabs, _sums=True)
            _same_bytes(many, one, (c, slabs))


# -------------------------------------------------------------------------------------- one past the limit, by the ABI

SENTINEL = 0x5A


def _sentinels(*shapes_and_types):
    import torch
    return [torch.full(shape, SENTINEL, dtype=torch.uint8, device="cuda").view(dtype) for shape, dtype in shapes_and_types]


def _untouched(tensors):
    import torch
    torch.cuda.synchronize()
    return all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in tensors)


def test_one_past_the_limit_is_refused_and_writes_nothing():
    """R = 4097, E = 8193, 65536 sources, batch and slabs of 1025 through the C ABI: EINVAL with the limit in the message, and
    outputs that hold their sentinel after a synchronize.  (K = 1025 of markers and ranks and tsne's slabs = 1025 are refused
    in tests/test_gpu_markers.py, test_gpu_ranks.py and test_gpu_tsne.py.)"""
    import torch
    from prosstt_amd import _native
    from prosstt_amd.device import _ptr
    N, d = 3, 2
    Y = torch.zeros((N, d), dtype=torch.float32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    # ptree: one node and one edge too many
    L = _native.load("ptree")
    R = MAX_NODES + 1
    C = torch.zeros((R, d), dtype=torch.float32, device="cuda")
    need = ctypes.c_uint64(0)
    with pytest.raises(_native.NativeError, match="R <= %d nodes" % MAX_NODES):
        _native.check(L.prosstt_amd_ptree_workspace_bytes(N, d, R, 0, ctypes.byref(need)), "ptree")
    outs = _sentinels(((4 * N,), torch.int32), ((4 * N,), torch.float32), ((8 * N,), torch.float64), ((8 * R,), torch.float64),
                      ((8 * R * d,), torch.float64))
    with pytest.raises(_native.NativeError, match="R <= %d nodes" % MAX_NODES):
        _native.check(L.prosstt_amd_ptree_assign(None, _ptr(Y), N, d, d, _ptr(C), R, d, 0.0, _ptr(ws), ws.numel(),
                                                 *[_ptr(o) for o in outs], None, _ptr(status)), "ptree")
    edges = torch.zeros((MAX_EDGES + 1, 2), dtype=torch.int32, device="cuda")
    pouts = _sentinels(((4 * N,), torch.int32), ((8 * N,), torch.float64), ((8 * N,), torch.float64))
    with pytest.raises(_native.NativeError, match="R <= %d nodes" % MAX_NODES):
        _native.check(L.prosstt_amd_ptree_project(None, _ptr(Y), N, d, d, _ptr(C), R, d, _ptr(edges), 1,
                                                  *[_ptr(o) for o in pouts], _ptr(status)), "ptree")
    with pytest.raises(_native.NativeError, match="E <= %d edges" % MAX_EDGES):
        _native.check(L.prosstt_amd_ptree_project(None, _ptr(Y), N, d, d, _ptr(C), MAX_NODES, d, _ptr(edges), MAX_EDGES + 1,
                                                  *[_ptr(o) for o in pouts], _ptr(status)), "ptree")
    assert _untouched(outs + pouts)
    # dpt: one source, one sequence pair and one slab too many
    L = _native.load("dpt")
    vectors = torch.zeros((N, 2), dtype=torch.float64, device="cuda")
    weights = torch.ones(2, dtype=torch.float64, device="cuda")
    sources = torch.zeros(MAX_SOURCES + 1, dtype=torch.int64, device="cuda")
    rows = _sentinels(((8 * (MAX_SOURCES + 1) * N,), torch.float64))
    with pytest.raises(_native.NativeError, match="n_sources <= %d" % MAX_SOURCES):
        _native.check(L.prosstt_amd_dpt_rows(None, _ptr(vectors), 2, _ptr(weights), N, 2, _ptr(sources), MAX_SOURCES + 1,
                                             _ptr(rows[0])), "dpt")
    ranks = torch.zeros((MAX_BATCH + 1, N), dtype=torch.int32, device="cuda")
    sums = _sentinels(((8 * (MAX_BATCH + 1) * N,), torch.int64), ((8 * (MAX_BATCH + 1) * N,), torch.int64))
    for batch, slabs, text in ((MAX_BATCH + 1, 1, "batch <= %d" % MAX_BATCH), (1, MAX_SLABS + 1, "slabs <= %d" % MAX_SLABS)):
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_dpt_workspace_bytes(N, batch, slabs, ctypes.byref(need)), "dpt")
        with pytest.raises(_native.NativeError, match=text):
            _native.check(L.prosstt_amd_dpt_concordance(None, _ptr(ranks), _ptr(ranks), N, batch, slabs, _ptr(ws), ws.numel(),
                                                        _ptr(sums[0]), _ptr(sums[1])), "dpt")
    assert _untouched(rows + sums) and int(status.item()) == 0


# ------------------------------------------------------------------------- bands and stale memory at the limit

def calls_markers(place=lambda value: value):
    """K = 1024 with one row per block (1 890 blocks) and the library's rule, and K = 1023, whose K + 1 offsets fill their
    segment of the workspace to the byte."""
    import test_gpu_markers as tm
    from prosstt_amd import markers
    N, G = markers_cells(MAX_GROUPS), G_SMALL
    s = tm._host(N, G)[1]
    shifted, aligned = place(tm._view(N, G, "shifted")), place(tm._view(N, G, "aligned"))
    at, below = group_codes(N, MAX_GROUPS, "full"), group_codes(N, MAX_GROUPS - 1, "full")
    return "markers at K = 1024", {
        "K = 1024, one row per block, shifted": lambda: markers.group_moments(shifted, s, at, rows_per_block=1),
        "K = 1024, aligned, out=torch": lambda: markers.group_moments(aligned, s, at, out="torch"),
        "K = 1023, one row per block, aligned": lambda: markers.group_moments(aligned, s, below, rows_per_block=1)}


def calls_ranks(place=lambda value: value):
    import test_gpu_ranks as tr
    from prosstt_amd import ranks
    labels, N = tr._labels(ranks_selected(MAX_GROUPS), MAX_GROUPS)
    s = tr._input("b", N, G_SMALL)[1]
    shifted, aligned = place(tr._view("b", N, G_SMALL, "shifted")), place(tr._view("b", N, G_SMALL, "aligned"))
    return "ranks at K = 1024", {
        "rest, shifted": lambda: ranks.rank_sums(shifted, s, labels),
        "the last group, two passes, aligned, out=torch": lambda: ranks.rank_sums(aligned, s, labels, reference=MAX_GROUPS - 1,
                                                                                 genes_per_pass=3, out="torch")}


def calls_trends(place=lambda value: value):
    """R = 2049 (three rounds of the table) and R = 2047, whose R + 1 offsets fill their segment to the byte."""
    import test_gpu_trends as tt
    from prosstt_amd import trends
    X = np.array(trends_counts(3))
    shifted, aligned = place(tt._view(X, "shifted")), place(tt._view(X, "aligned"))
    w = {R: tt._weights(trends_csr(R, long_at, empty_at), TRENDS_N) for R, long_at, empty_at, _ in TRENDS_CASES if R in (2047, 2049)}
    return "trends at R = 2049", {
        "R = 2049, shifted": lambda: trends.node_sums(shifted, w[2049]),
        "R = 2049, chunks of 1, aligned, out=torch": lambda: trends.node_sums(aligned, w[2049], entries_per_block=1, out="torch"),
        "R = 2047, chunks of 64, aligned": lambda: trends.node_sums(aligned, w[2047], entries_per_block=64)}


def calls_ptree(place=lambda value: value):
    import test_gpu_ptree as tp
    from prosstt_amd import ptree
    R, N, d = PTREE_HARD[-1]
    Y, C = ptree_hard_inputs(R, N, d)
    Yv, Cv = place(tp._view(Y, "shifted")), place(tp._view(C, "wide"))
    Rp, E, Np, dp = PTREE_PROJECT[-1]
    Yp, Cp, edges = ptree_project_inputs(Rp, E, Np, dp)
    Ypv, Cpv = place(tp._view(Yp, "wide")), place(tp._view(Cp, "shifted"))
    assert R == Rp == MAX_NODES and E == MAX_EDGES
    return "ptree at R = 4096 and E = 8192", {
        "assign, hard": lambda: ptree.assign(Yv, Cv, 0.0, responsibilities=True),
        "assign, soft, out=torch": lambda: ptree.assign(Yv, Cv, 2.0, responsibilities=True, out="torch"),
        "project": lambda: ptree.project(Ypv, Cpv, edges)}


def calls_dpt(place=lambda value: value):
    import test_gpu_dpt as td
    from prosstt_amd import dpt
    ru, rv = dpt_batch_sequences()["four values"][:2]
    ru, rv = place(td._cuda(ru)), place(td._cuda(rv))
    return "dpt at batch 1024", {"concordance, slabs 1": lambda: dpt.concordance(ru, rv, 1),
                                 "concordance, slabs 3": lambda: dpt.concordance(ru, rv, 3)}


AT_THE_LIMIT = {"markers": calls_markers, "ranks": calls_ranks, "trends": calls_trends, "ptree": calls_ptree, "dpt": calls_dpt}


@pytest.mark.parametrize("library", list(AT_THE_LIMIT))
def test_no_access_outside_a_buffer_at_the_limit(library):
    """tests/test_gpu_guard_bands.py's checks: no band damaged, no input written, equal bytes under the three bytes."""
    import test_gpu_guard_bands as bands
    bands._guarded_runs(library, AT_THE_LIMIT[library], "at the limit")


@pytest.mark.parametrize("library", list(AT_THE_LIMIT))
def test_no_result_depends_on_stale_memory_at_the_limit(library):
    from test_gpu_stale_memory import _thrice
    _thrice(*AT_THE_LIMIT[library]())
