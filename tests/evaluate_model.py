"""The numpy model of libprosstt_amd_evaluate.so, written from include/prosstt_amd_evaluate.h alone: brute force over all pairs
by broadcasting, Python integers for the moment sums.  It takes the cells as the header does (sorted by class, with offsets),
and ``by_class`` does the stable sort for callers that hold a class per cell.  ``plan`` mirrors the two block tables and the
kinds of block of the pass, for the host tests that show which path a GPU case reaches.  A helper: nothing here is
collected."""
import numpy as np

MAX_DEPTH = 65535
TILE, BLOCK_ROWS, MAX_TILES = 256, 512, 4096


def by_class(classes, K):
    """(order, offsets): the stable sort of the cells by class and the K + 1 offsets of the header."""
    classes = np.asarray(classes, dtype=np.int64)
    order = np.argsort(classes, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(classes, minlength=K))]).astype(np.int64)
    return order, offsets


def _pair_sets(offsets):
    """Per class pair p <= q: (p, q, rows, columns, the (rows, columns) boolean matrix of the pairs of its set)."""
    K = len(offsets) - 1
    for p in range(K):
        for q in range(p, K):
            i = np.arange(offsets[p], offsets[p + 1])
            j = np.arange(offsets[q], offsets[q + 1])
            inside = np.ones((len(i), len(j)), dtype=bool) if p < q else i[:, None] < j[None, :]
            yield p, q, i, j, inside


def pairs(offsets):
    K = len(offsets) - 1
    out = np.zeros((K, K), dtype=np.int64)
    for p, q, _, _, inside in _pair_sets(offsets):
        out[p, q] = inside.sum()
    return out


def pair_counts(a, b, offsets):
    """(K, K, 4) int64: S, P, A2, B2 of the header for sequences sorted by class."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    K = len(offsets) - 1
    out = np.zeros((K, K, 4), dtype=np.int64)
    for p, q, i, j, inside in _pair_sets(offsets):
        sa = np.sign(a[i][:, None] - a[j][None, :]) * inside
        sb = np.sign(b[i][:, None] - b[j][None, :]) * inside
        out[p, q] = ((sa * sb).sum(), ((sa * sb) ** 2).sum(), (sa ** 2).sum(), (sb ** 2).sum())
    return out


def junction_entry(v):
    return min(max(int(v), 0), MAX_DEPTH)


def distances(h, c, J, i, j):
    """d of the header between the cells i (rows) and j (columns): an int64 matrix."""
    Jc = np.vectorize(junction_entry)(np.asarray(J)).astype(np.int64).reshape(np.asarray(J).shape)
    hi, hj = h[i][:, None], h[j][None, :]
    m = np.minimum(np.minimum(hi, hj), Jc[c[i][:, None], c[j][None, :]])
    return hi + hj - 2 * m


def pair_moments(h, offsets, J, h2, c2, J2):
    """(K, K, 5) object array of Python integers: sum d, d2, d^2, d2^2, d d2 of the header for cells sorted by class."""
    h, h2, c2 = (np.asarray(v, dtype=np.int64) for v in (h, h2, c2))
    K = len(offsets) - 1
    c = np.repeat(np.arange(K), np.diff(offsets))
    out = np.zeros((K, K, 5), dtype=object)
    for p, q, i, j, inside in _pair_sets(offsets):
        d = distances(h, c, J, i, j)[inside]
        e = distances(h2, c2, J2, i, j)[inside]
        if len(d) < 1 << 29:                 # a term is below 2^34: the int64 sums are exact
            out[p, q] = tuple(int(v.sum()) for v in (d, e, d * d, e * e, d * e))
        else:
            d, e = d.tolist(), e.tolist()
            out[p, q] = (sum(d), sum(e), sum(x * x for x in d), sum(y * y for y in e), sum(x * y for x, y in zip(d, e)))
    return out


def words(sums):
    """The (K, K, 5, 2) uint64 words (low, high) of ``pair_moments``' sums."""
    K = sums.shape[0]
    out = np.zeros((K, K, 5, 2), dtype=np.uint64)
    for p in range(K):
        for q in range(K):
            for i in range(5):
                v = int(sums[p, q, i])
                out[p, q, i] = (v & 0xFFFFFFFFFFFFFFFF, v >> 64)
    return out


# ------------------------------------------------------------------------------------------------------ statistics

def gamma(a, b):
    """Goodman-Kruskal's gamma of two sequences by a direct count of the concordant and discordant pairs."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    i, j = np.triu_indices(len(a), 1)
    s = np.sign(a[i] - a[j]) * np.sign(b[i] - b[j])
    C, D = int((s > 0).sum()), int((s < 0).sum())
    return (C - D) / (C + D) if C + D else float("nan")


def tree_arrays(topology, time, branches, ticks=1):
    """(first, last, J) of a tree given as the package's ``Tree`` takes it: per branch (in ``branches`` order) the absolute
    time of its first and last node, and the junction table of the header at ``ticks`` steps per unit of time."""
    parent = {child: par for par, child in topology}
    first = {}
    for b in branches:
        chain, at = [], b
        while at in parent:
            at = parent[at]
            chain.append(at)
        first[b] = sum(time[x] for x in chain)
    last = {b: first[b] + time[b] - 1 for b in branches}

    def ancestors(b):
        out = [b]
        while out[-1] in parent:
            out.append(parent[out[-1]])
        return out

    B = len(branches)
    J = np.full((B, B), MAX_DEPTH, dtype=np.int64)
    for x, p in enumerate(branches):
        for y, q in enumerate(branches):
            ap, aq = ancestors(p), ancestors(q)
            if p in aq or q in ap:
                continue
            common = next(z for z in ap if z in aq)
            J[x, y] = last[common] * ticks
    return np.array([first[b] for b in branches]), np.array([last[b] for b in branches]), J


# ---------------------------------------------------------------------------------------------------- the block plan

def default_tiles(N, K):
    """tiles_per_block = 0 of the header."""
    tiles, row_blocks = -(-N // TILE), -(-N // BLOCK_ROWS)
    t = min(max(row_blocks * tiles // 4096, 1), MAX_TILES)
    return max(t, -(-tiles // (65535 - K)))


def tables(offsets, tiles_per_block):
    """(row blocks, chunks): lists of (first, class, count), class after class, as evaluate_table_kernel writes them."""
    rows, chunks = [], []
    for p in range(len(offsets) - 1):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        for span, out in ((BLOCK_ROWS, rows), (TILE * tiles_per_block, chunks)):
            for first in range(lo, hi, span):
                out.append((first, p, min(span, hi - first)))
    return rows, chunks


def plan(offsets, tiles_per_block):
    """What the blocks of the pass do.  Returns a dict of counters: ``blocks``; ``below`` (p > q: exits), ``skipped`` (p = q,
    the chunk wholly before the rows: zeros), ``off_diagonal`` and ``diagonal`` working blocks; per tile of a working block
    ``tiles_fast`` (no index compare), ``tiles_masked`` (a tile of a diagonal block that meets its rows), ``tiles_before``
    (passed over); ``ragged_tiles`` (fewer than 256 columns), ``ragged_rows`` (row blocks of fewer than 512 rows),
    ``split_classes`` (classes of more than one chunk) and ``empty_classes``."""
    rows, chunks = tables(offsets, tiles_per_block)
    sizes = np.diff(offsets)
    out = dict(blocks=len(rows) * len(chunks), below=0, skipped=0, off_diagonal=0, diagonal=0, tiles_fast=0, tiles_masked=0,
               tiles_before=0, ragged_tiles=0, ragged_rows=sum(1 for r in rows if r[2] < BLOCK_ROWS),
               split_classes=int(sum(1 for n in sizes if n > TILE * tiles_per_block)), empty_classes=int((sizes == 0).sum()))
    for r_first, p, r_count in rows:
        for c_first, q, c_count in chunks:
            if p > q:
                out["below"] += 1
                continue
            if p == q and c_first + c_count <= r_first:
                out["skipped"] += 1
                continue
            out["diagonal" if p == q else "off_diagonal"] += 1
            for col0 in range(c_first, c_first + c_count, TILE):
                cnt = min(TILE, c_first + c_count - col0)
                if p == q and col0 + cnt <= r_first:
                    out["tiles_before"] += 1
                    continue
                out["ragged_tiles"] += cnt < TILE
                out["tiles_masked" if p == q and col0 < r_first + BLOCK_ROWS else "tiles_fast"] += 1
    return out
