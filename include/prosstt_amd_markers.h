/*
 * prosstt_amd_markers.h -- per-group sums over the log-normalised count matrix on the device
 * (libprosstt_amd_markers.so): what a ranking of marker genes per group of cells (scanpy's tl.rank_genes_groups with a t-test)
 * and a per-group pseudo-bulk are computed from.  prosstt_amd/markers.py drives it and holds the statistics.
 *
 * Definition.
 *
 *   Input.  X: N cells x G genes, int32, and inv_size: N floats, both exactly as in prosstt_amd_embed.h (row r, gene g at
 *   X[r*ld + g], ld >= G, any base alignment; inv_size[i] = fl32(1 / s[i]) in [2^-126, 2^94]).  rows: the n_sel <= N selected
 *   row indices, int32, sorted by group and in the caller's order within a group.  group_start: K + 1 int64 offsets into rows,
 *   ascending from 0 to n_sel: group k is rows[group_start[k] .. group_start[k + 1]).
 *
 *   Output, each [K][G], per group k and gene j over the group's rows r:
 *       nz[k][j] = the number of r with X[r][j] > 0                  int64
 *       cs[k][j] = sum of X[r][j]                                    int64, exact
 *       S1[k][j] = sum of a,   S2[k][j] = sum of a a                 binary64
 *   with a = (double) of the float32 entry log1p(X[r][j] * inv_size[r]) of prosstt_amd_embed.h, bit for bit that library's
 *   (one definition in the source, csrc/log1p_entry.h).  An empty group gives zeros.
 *
 *   Order of the floating-point sums (part of the definition).  Group k's rows are cut into ceil(n_k / rows_per_block)
 *   blocks of rows_per_block consecutive positions of `rows` (the last one shorter); no block spans two groups.  Within a
 *   block, in `rows` order: s1 = s1 + a, s2 = fma(a, a, s2) (a a is exact in binary64, so this is s2 + a a rounded once),
 *   both from 0.  Then the group's blocks are added in ascending order, from 0.  The integers do not depend on the order, so
 *   they are the same for every rows_per_block; the floats are the same for equal rows_per_block.
 *
 * Kernels (256 threads, 64-bit offsets, no scratch, no floating-point atomic).
 *   markers_table_kernel   one block: the blocks per group, their prefix sum first_block[0 .. K], and the block table
 *                          (group, first, last) of every block, from group_start on the device: nothing synchronises.
 *   markers_pass_kernel    embed_moments_kernel's layout: a block owns a strip of 1024 genes (one 16-byte load per lane and
 *                          row when rows are 16-byte aligned; a scalar path otherwise) over one entry of the block table.
 *                          The grid's y extent is the bound ceil(n_sel / rows_per_block) + K; blocks past the table's end
 *                          exit.  The row index and inv_size[row] are block-uniform loads.  Partials go to slabs [blocks][G].
 *   markers_finish_kernel  one thread per (group, gene) adds the group's blocks in ascending order.
 *
 * Conventions (as in prosstt_amd_embed.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_MARKERS_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_markers_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers (group_start too).  All work is enqueued on the caller's stream (NULL: the default
 *    stream of the current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    _workspace_bytes(n_sel, G, K, rows_per_block) bytes, 16-byte aligned.
 *  - Deterministic: equal inputs give bit-identical outputs on any stream.
 *  - *status (the caller zeroes it; bits are only ever set) and, when it is not zero, meaningless outputs:
 *      PROSSTT_AMD_MARKERS_NEGATIVE      a negative count among the selected rows
 *      PROSSTT_AMD_MARKERS_ROW_RANGE     an entry of rows outside [0, N); that row is not read
 *      PROSSTT_AMD_MARKERS_GROUP_RANGE   group_start is not ascending from 0 to n_sel; offsets are clamped, nothing is read
 *                                        or written out of bounds
 *  - Limits, refused with PROSSTT_AMD_MARKERS_EINVAL: 1 <= N < 2^31, 1 <= G, ld >= G, 0 <= n_sel <= N, 1 <= K <=
 *    PROSSTT_AMD_MARKERS_MAX_GROUPS, rows_per_block >= 0, ceil(n_sel / rows_per_block) + K <= 65535 (the grid's y extent), a
 *    workspace at least the query's.
 */
#ifndef PROSSTT_AMD_MARKERS_H
#define PROSSTT_AMD_MARKERS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_MARKERS_OK = 0,
    PROSSTT_AMD_MARKERS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_MARKERS_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_MARKERS_MAX_GROUPS 1024
#define PROSSTT_AMD_MARKERS_NEGATIVE 1u
#define PROSSTT_AMD_MARKERS_ROW_RANGE 2u
#define PROSSTT_AMD_MARKERS_GROUP_RANGE 4u

const char* prosstt_amd_markers_last_error(void);

/* Device workspace (bytes) of _group_moments for these sizes.  rows_per_block as there.  Pure. */
int prosstt_amd_markers_workspace_bytes(int64_t n_sel, int64_t G, int64_t K, int64_t rows_per_block, uint64_t* bytes);

/* The four outputs of the definition.  rows_per_block: 0 for the library's rule (that of the strip kernels for an n_sel x G
 * matrix: about 1024 blocks, at least 64 rows each), or any positive value. */
int prosstt_amd_markers_group_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                      const float* inv_size, const int32_t* rows, int64_t n_sel,
                                      const int64_t* group_start /* K + 1 */, int64_t K, int64_t rows_per_block,
                                      void* ws, uint64_t ws_bytes, int64_t* nz, int64_t* cs, double* S1, double* S2,
                                      uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
