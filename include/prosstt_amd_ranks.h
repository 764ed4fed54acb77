/*
 * prosstt_amd_ranks.h -- rank sums over the log-normalised count matrix on the device (libprosstt_amd_ranks.so): what a
 * Wilcoxon rank-sum (Mann-Whitney) ranking of marker genes per group of cells (scanpy's tl.rank_genes_groups with
 * method="wilcoxon") is computed from.  prosstt_amd/ranks.py drives it and holds the statistics.
 *
 * Definition.
 *
 *   Input, as for the grouped pass of prosstt_amd_markers.h.  X: N cells x G genes, int32, and inv_size: N floats (row r,
 *   gene g at X[r*ld + g], ld >= G, any base alignment; inv_size[i] = fl32(1 / s[i]) in [2^-126, 2^94]).  rows: the n_sel <= N
 *   selected row indices, int32, sorted by group.  group_start: K + 1 int64 offsets into rows, ascending from 0 to n_sel:
 *   group k is rows[group_start[k] .. group_start[k + 1]).  reference: -1, the counting set C is all selected rows; r >= 0,
 *   C is group r.
 *
 *   For gene j let a_q be the float32 entry log1p(X[rows[q]][j] * inv_size[rows[q]]) of prosstt_amd_embed.h, bit for bit that
 *   library's (one definition in the source, csrc/log1p_entry.h).  Output:
 *       Q[k][j] = sum over the positions q of group k of ( #{c in C : a_c < a_q} + #{c in C : a_c <= a_q} )    int64 [K][G]
 *       T[j]    = sum over the maximal runs of equal a among all selected rows of (t^3 - t), t the run's length  int64 [G]
 *   Both are exact integers: they depend on no order of evaluation, not on genes_per_pass and not on the stream.  An empty
 *   group, or an empty C, gives zeros.
 *
 *   What follows from them (n = n_sel, n_k the cells of group k; checked against scipy in tests/test_ranks_model.py):
 *       against the rest (reference = -1): the rank sum of group k with midranks is (Q[k] + n_k) / 2, and the tie correction
 *       1 - T / (n^3 - n) is scipy.stats.tiecorrect;
 *       against group r: Q[k] / 2 is the Mann-Whitney U of k against r with half counts for ties, and the rank sum of k
 *       within k and r together is U + n_k (n_k + 1) / 2.
 *
 * Kernels (256 threads, 64-bit offsets, no scratch, no floating-point arithmetic after the entry is formed).  The genes are
 * taken in chunks of genes_per_pass; the workspace holds one chunk, a segment of n_sel entries per gene, as two ping-pong
 * copies of a 32-bit key and a 16-bit payload per entry: 12 bytes per entry.
 *   ranks_emit_kernel   reads the matrix once in the strip order of the markers pass (a block owns 1024 genes over 16
 *                       positions of rows; row index and inv_size[row] are block-uniform; one 16-byte load per lane and row
 *                       when rows are 16-byte aligned, a scalar path otherwise), forms the entries, transposes the tile
 *                       through LDS and writes every gene's segment in runs of 16 positions.  Key: the bit pattern of a (a
 *                       is finite and >= +0, so unsigned order is numeric order).  Payload: the group of position q, from
 *                       group_start alone.  Zeros are entries like all others.
 *   ranks_sort_kernel   one launch per digit of a least-significant-digit radix sort of the key: four passes of 8 bits.
 *                       One block owns one gene's segment and walks it in tiles of PROSSTT_AMD_RANKS_SORT_TILE positions:
 *                       a histogram in LDS, an exclusive scan, and a stable scatter in position order (wave ballots per
 *                       digit bit, a scan across the block's waves).  A scatter offset comes from the histogram of the very
 *                       data being scattered and from nothing the caller passed.
 *   ranks_fold_kernel   one block per gene over the sorted segment.  Run boundaries are key[p] != key[p - 1]; every
 *                       position gets its run's start and end from two segmented scans (one walk up, one walk down the
 *                       segment, a carry across tiles; no thread walks a run).  With P[p] = the members of C among the
 *                       sorted positions [0, p), a position of group k adds P[start] + P[end] into an LDS table of K int64
 *                       (integer LDS atomics), the first position of a run adds t^3 - t; then Q[.][j] and T[j] are stored.
 *
 * Conventions (as in prosstt_amd_markers.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_RANKS_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_ranks_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers (group_start too).  All work is enqueued on the caller's stream (NULL: the default
 *    stream of the current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    _workspace_bytes(n_sel, G, genes_per_pass) bytes, 16-byte aligned.
 *  - Deterministic: equal inputs give equal outputs on any stream and for any genes_per_pass.
 *  - *status (the caller zeroes it; bits are only ever set) and, when it is not zero, meaningless outputs:
 *      PROSSTT_AMD_RANKS_NEGATIVE      a negative count among the selected rows
 *      PROSSTT_AMD_RANKS_ROW_RANGE     an entry of rows outside [0, N); that row is not read
 *      PROSSTT_AMD_RANKS_GROUP_RANGE   group_start is not ascending from 0 to n_sel; every position still gets a group in
 *                                      [0, K), nothing is read or written out of bounds
 *  - genes_per_pass: 0 for the library's rule, as many genes as keep the workspace at or below 1 GiB:
 *        clamp(floor((2^30 - 1024) / (12 max(n_sel, 1))), 1, G);
 *    any positive value is taken as given (above G it means G).
 *  - Limits, refused with PROSSTT_AMD_RANKS_EINVAL: 1 <= N < 2^31, 1 <= G, ld >= G, 0 <= n_sel <= min(N,
 *    PROSSTT_AMD_RANKS_MAX_ROWS) (so that T < 2^60), 1 <= K <= PROSSTT_AMD_RANKS_MAX_GROUPS, -1 <= reference < K,
 *    genes_per_pass >= 0 and at most 65535 * 1024 genes in a chunk (the emit grid's y extent), a workspace at least the
 *    query's.
 */
#ifndef PROSSTT_AMD_RANKS_H
#define PROSSTT_AMD_RANKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_RANKS_OK = 0,
    PROSSTT_AMD_RANKS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_RANKS_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_RANKS_MAX_GROUPS 1024
#define PROSSTT_AMD_RANKS_MAX_ROWS (1 << 20)
#define PROSSTT_AMD_RANKS_SORT_TILE 1024
#define PROSSTT_AMD_RANKS_NEGATIVE 1u
#define PROSSTT_AMD_RANKS_ROW_RANGE 2u
#define PROSSTT_AMD_RANKS_GROUP_RANGE 4u

const char* prosstt_amd_ranks_last_error(void);

/* Device workspace (bytes) of _rank_sums for these sizes.  genes_per_pass as there.  Pure. */
int prosstt_amd_ranks_workspace_bytes(int64_t n_sel, int64_t G, int64_t genes_per_pass, uint64_t* bytes);

/* The two outputs of the definition. */
int prosstt_amd_ranks_rank_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                const float* inv_size, const int32_t* rows, int64_t n_sel,
                                const int64_t* group_start /* K + 1 */, int64_t K, int64_t reference,
                                int64_t genes_per_pass, void* ws, uint64_t ws_bytes, int64_t* Q /* [K][G] */,
                                int64_t* T /* [G] */, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
