/*
 * prosstt_amd_evaluate.h -- scores of an inferred trajectory against the simulated truth on the device
 * (libprosstt_amd_evaluate.so): exact integer sums over all N (N - 1) / 2 pairs of cells, binned by the pair of true classes.
 *
 * Two passes.  The pair counts are what Goodman-Kruskal's gamma and Kendall's tau-a and tau-b are ratios of (MERLoT's
 * benchmark of PROSSTT simulations takes them over the pairs of cells on a common lineage); the pair moments are what the
 * Pearson correlation of the geodesic distances on two trees is a ratio of (dynverse's main metric, there over sampled
 * waypoints).  The ratios are the caller's; everything here is an integer.
 *
 * Definition.
 *
 *   Cells and classes.  N cells, 2 <= N < 2^31, presented SORTED by their true class c_i, 0 <= c_i < K, 1 <= K <=
 *   PROSSTT_AMD_EVALUATE_MAX_CLASSES.  The classes are given as `offsets`, K + 1 int64 values: class p holds the cells
 *   [offsets[p], offsets[p + 1]); non-decreasing, offsets[0] = 0, offsets[K] = N.  A class may be empty.
 *
 *   Pair sets.  For a class pair p <= q: all (i, j) with i in p and j in q when p < q; all i < j in p when p = q.  Every
 *   unordered pair of cells lies in exactly one set.  Outputs of a class pair p > q are written as 0.
 *
 *   Pair counts.  Two int32 sequences a and b of length N; any values whose differences fit int32.  With sa = sgn(a_i - a_j)
 *   and sb = sgn(b_i - b_j), per class pair four int64 values in this order:
 *       S = sum sa sb,   P = sum (sa sb)^2,   A2 = sum sa^2,   B2 = sum sb^2.
 *   From these: concordant pairs C = (P + S) / 2, discordant D = (P - S) / 2, pairs tied in a = pairs - A2, tied in b = pairs
 *   - B2; gamma = S / P, tau-a = S / pairs, tau-b = S / sqrt(A2 B2), over one class pair or over the sums of several.
 *
 *   Pair moments.  Two trees.  The true tree: per cell a depth h_i, 0 <= h_i <= PROSSTT_AMD_EVALUATE_MAX_DEPTH, its branch is
 *   its class, and a junction table J, K x K int32.  The second tree: per cell a depth h2_i in the same range and a branch
 *   c2_i, 0 <= c2_i < K2, 1 <= K2 <= PROSSTT_AMD_EVALUATE_MAX_CLASSES, and a junction table J2, K2 x K2 int32.  A junction
 *   table is symmetric: J[p][q] is the depth of the last node of the deepest common ancestor branch of p and q when neither
 *   is the other or its ancestor, and any value >= PROSSTT_AMD_EVALUATE_MAX_DEPTH otherwise (p = q included).  An entry is
 *   read as min(max(entry, 0), MAX_DEPTH).  The distance of two cells on a tree is
 *       d(i, j) = h_i + h_j - 2 min(h_i, h_j, J[c_i][c_j]),
 *   the graph distance on the tree of nodes whose junction is the parent's last node: |h_i - h_j| along a lineage, (h_i - e)
 *   + (h_j - e) across a junction of depth e.  0 <= d <= 2 MAX_DEPTH.  With d on the true tree and d2 on the second, per
 *   class pair five exact sums in this order, each as two uint64 words (low, high):
 *       sum d,   sum d2,   sum d^2,   sum d2^2,   sum d d2.
 *
 *   Status.  `status` is one uint32 word that the CALLER zeroes.  A bit is set (atomicOr, the library's only atomic) for
 *     PROSSTT_AMD_EVALUATE_OFFSETS_RANGE  offsets that do not ascend from 0 to N.  They are clamped into [0, N] and the tables
 *                                         to their bounds: nothing is read out of bounds.
 *     PROSSTT_AMD_EVALUATE_DEPTH_RANGE    a depth outside 0 .. MAX_DEPTH: the cell contributes to no sum.
 *     PROSSTT_AMD_EVALUATE_BRANCH_RANGE   a second-tree branch outside [0, K2): the cell contributes to no sum.
 *   The outputs are written only while the word is 0 after the passes: a flagged call leaves them as they were.
 *
 * Kernels.  No floating point anywhere.
 *   evaluate_table_kernel  one block.  From `offsets` two tables in the workspace: ROW BLOCKS of at most
 *                          PROSSTT_AMD_EVALUATE_BLOCK_ROWS cells and COLUMN CHUNKS of at most tiles_per_block tiles of
 *                          PROSSTT_AMD_EVALUATE_TILE cells; neither crosses a class boundary, so the host never reads
 *                          `offsets`.  Class p of n_p cells has ceil(n_p / 512) row blocks and ceil(n_p / (256 tiles_per_block))
 *                          chunks: at most ceil(N / 512) + K and ceil(N / (256 tiles_per_block)) + K in all, which is what the
 *                          workspace and the grid are sized by.
 *   evaluate_pass_kernel   <counts> and <moments>, one body.  Block (x, y) takes row block x and chunk y; its class pair (p, q)
 *                          is block-uniform.  A block with p > q exits at once (the fold reads nothing of it); a block with
 *                          p = q whose chunk lies wholly before its rows stores zeros and exits.  256 threads, two rows
 *                          per thread 256 apart; a tile's columns are staged in LDS and read as a broadcast, 16 columns to a group.  Only a tile of a p = q block that
 *                          meets the block's rows (and a tile that holds an inadmissible cell) compares indices.  Counts: two
 *                          subtractions, two medians of three, 24-bit multiply-adds, int32 sums.  Moments: J[p][q] is a
 *                          scalar; J2 lies in LDS as 64 x 64 words at c2_j 64 + c2_i, so that the lanes of a read differ in
 *                          the row cell's branch alone (distinct branches on distinct banks modulo 32, equal ones a
 *                          broadcast); a column's (h2, 64 c2) is one word; sum d and sum d2 are 32-bit within a tile, the
 *                          three products 64-bit multiply-adds.  The block's sums: wave reductions, then the four waves
 *                          through LDS, then one store per sum to the workspace.
 *   evaluate_fold_kernel   one block per class pair: the partial sums of its blocks, added with carry.
 *   Integer sums do not depend on their order: equal results for every tiles_per_block, stream and run.
 *
 * The 64-bit bound.  A block's partial sum is one unsigned 64-bit word.  A block holds at most 512 rows x 256 T columns, T =
 * tiles_per_block, and a term is at most (2 MAX_DEPTH)^2 = 131 070^2 < 2^34: the partial is below 2^9 2^8 T 2^34 = 2^51 T, which
 * is at most 2^63 for T <= PROSSTT_AMD_EVALUATE_MAX_TILES_PER_BLOCK = 4096.  A thread's int32 sums of the counts are at most
 * 2 x 256 T = 2^21 in size.  Within a tile a thread's sum of d over one row is at most 256 x 131 070 < 2^25.
 *
 * tiles_per_block = 0 is the library's choice: floor(row blocks x tiles / 4096) for ceil(N / 512) row blocks and ceil(N / 256)
 * tiles, at least 1 and at most 4096 (half of the blocks lie below the diagonal and exit: about 8 working blocks per CU of
 * the MI355X's 256), raised where needed so that the chunks fit the grid's second dimension (65 535).
 *
 * Conventions (as in prosstt_amd_dpt.h and prosstt_amd_trends.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_EVALUATE_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_evaluate_last_error.  Bad sizes and pointers are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory.
 *  - Kernels use 64-bit offsets and no scratch.
 */
#ifndef PROSSTT_AMD_EVALUATE_H
#define PROSSTT_AMD_EVALUATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_EVALUATE_OK = 0,
    PROSSTT_AMD_EVALUATE_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_EVALUATE_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_EVALUATE_MAX_CLASSES 64
#define PROSSTT_AMD_EVALUATE_MAX_DEPTH 65535
#define PROSSTT_AMD_EVALUATE_TILE 256                   /* columns of a tile */
#define PROSSTT_AMD_EVALUATE_BLOCK_ROWS 512             /* rows of a block */
#define PROSSTT_AMD_EVALUATE_MAX_TILES_PER_BLOCK 4096
#define PROSSTT_AMD_EVALUATE_COUNT_WORDS 4              /* S, P, A2, B2 */
#define PROSSTT_AMD_EVALUATE_MOMENT_SUMS 5              /* d, d2, d^2, d2^2, d d2: two words each */

/* the bits of the status word */
#define PROSSTT_AMD_EVALUATE_OFFSETS_RANGE 1u
#define PROSSTT_AMD_EVALUATE_DEPTH_RANGE 2u
#define PROSSTT_AMD_EVALUATE_BRANCH_RANGE 4u

const char* prosstt_amd_evaluate_last_error(void);

/* Device workspace (bytes) of either pass for these sizes; tiles_per_block as there.  Pure: the tables are bounded from N, K
 * and tiles_per_block alone.  It grows as (N / 512 + K) (N / (256 tiles_per_block) + K) x 40 bytes. */
int prosstt_amd_evaluate_workspace_bytes(int64_t N, int32_t K, int32_t tiles_per_block, uint64_t* bytes);

/* counts[(p K + q) 4 + w], w = S, P, A2, B2 of the definition.  0 <= tiles_per_block <= MAX_TILES_PER_BLOCK; workspace:
 * _workspace_bytes(N, K, tiles_per_block) bytes, 16-byte aligned; status: one zeroed word. */
int prosstt_amd_evaluate_pair_counts(void* stream, const int32_t* a /* N */, const int32_t* b /* N */,
                                     const int64_t* offsets /* K + 1 */, int64_t N, int32_t K, int32_t tiles_per_block,
                                     void* workspace, uint64_t bytes, int64_t* counts /* K x K x 4 */, uint32_t* status);

/* moments[((p K + q) 5 + w) 2 + (0: low, 1: high)], w = the five sums of the definition. */
int prosstt_amd_evaluate_pair_moments(void* stream, const int32_t* h /* N */, const int32_t* h2 /* N */,
                                      const int32_t* c2 /* N */, const int64_t* offsets /* K + 1 */, const int32_t* J /* K x K */,
                                      const int32_t* J2 /* K2 x K2 */, int64_t N, int32_t K, int32_t K2, int32_t tiles_per_block,
                                      void* workspace, uint64_t bytes, uint64_t* moments /* K x K x 5 x 2 */, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
