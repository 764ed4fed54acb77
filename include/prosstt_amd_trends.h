/*
 * prosstt_amd_trends.h -- weighted sums of the cells of a count matrix around the nodes of a lineage tree on the device
 * (libprosstt_amd_trends.so): what the mean expression and the variance of every gene at every node are computed from.
 * prosstt_amd/trends.py builds the weights, drives the pass and holds the results.
 *
 * Definition.
 *
 *   Nodes.  The integer time steps of every branch of a tree, in the row order of its mean tensor: R = sum_b T_b rows; node
 *   (b, j) has the absolute pseudotime first_b + j.  A cell has a branch and a binary64 absolute pseudotime inside its
 *   branch's [first, last].
 *
 *   Tree distance of the positions (b, t) and (b', t'), binary64, every operation rounded on its own:
 *       b an ancestor of b', b' one of b, or b = b':   d = |t - t'|
 *       otherwise:                                     d = (t - e) + (t' - e), e the last absolute time of the deepest
 *                                                      common ancestor branch
 *   (the graph distance on the node tree, whose junction is the parent's last node).
 *
 *   Weight (tricube, bandwidth h > 0 in units of pseudotime):  u = d / h; no entry when u >= 1; c = (u * u) * u; v = 1 - c;
 *   w = (v * v) * v; q = floor(w * 4096 + 0.5), an integer in 0 .. 4096 = PROSSTT_AMD_TRENDS_ONE; q = 0 is dropped.
 *   Nearest: the cell's only entry is q = 4096 at node j = floor((t - first_b) + 0.5), clipped to 0 .. T_b - 1, of its own
 *   branch.  The weights are built on the host; this library takes them as they come.
 *
 *   Input.  X: N rows x G genes, int32, row r and gene g at X[r*ld + g], ld >= G, any base alignment, read in place.
 *   A CSR matrix of R nodes x N matrix rows: indptr R + 1 int64 ascending from 0 to nnz; indices nnz int32 in [0, N), the
 *   MATRIX ROW of the entry's cell, in any order, repeats allowed; weights nnz int32 in [0, 4096].
 *
 *   Sums, exact integers (no floating point on the device), over the entries e of node r's row:
 *       S1[r][g] = sum_e q_e * x[c_e][g]                       int64, at S1[r*G + g]
 *       S2[r][g] = sum_e q_e * x[c_e][g]^2                     128 bits as (low, high) uint64 words at S2[2*(r*G + g)],
 *                                                              the format of prosstt_amd_stats.h's gene_sumsq
 *   A node without entries gives zeros.  A row of the CSR matrix holds at most 2^20 - 1 entries (the caller checks it:
 *   indptr is device memory): then S1 < 2^63 for counts up to 2^31 - 1, and no accumulator below wraps.
 *
 * Kernels (256 threads, 64-bit offsets, no scratch, no floating point, no atomic but the status word's OR).
 *   trends_table_kernel   one block of 1024 threads walks indptr, 1024 nodes at a time: chunks per node
 *                         ceil(n_r / entries_per_block), their running sum, and the table (first entry, node, entries) of
 *                         every chunk, so that the host never reads indptr
 *   trends_pass_kernel    a strip kernel: a block owns 1024 genes, four per lane (one 16-byte load per lane and row when rows
 *                         are 16-byte aligned, four 4-byte loads otherwise), and one chunk.  An entry's index and weight are
 *                         block-uniform loads; four indexed rows are in flight before the arithmetic.  Per gene three 64-bit
 *                         accumulators: S1 += q x, A += q lo32(x^2), B += q hi32(x^2), each below 2^64 over 2^20 - 1 entries;
 *                         S2 = A + B 2^32 is put together in 128 bits once per chunk.  A node of one chunk is written to S1
 *                         and S2 directly, the others to slabs [chunks][G] of the workspace.
 *   trends_finish_kernel  one thread per (node, gene): adds a node's chunks with carry; zeros for a node without entries.
 *
 * Conventions (as in prosstt_amd_autocorr.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_TRENDS_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_trends_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of the queried
 *    size, 16-byte aligned.
 *  - Deterministic: integer sums have no order, so equal inputs give identical outputs on any stream and for any
 *    entries_per_block.
 *  - The CSR arrays are the caller's to check.  As a guard nothing is read or written out of bounds whatever they hold;
 *    what is wrong sets a bit of *status (the caller zeroes it; bits are only ever set, with an atomic OR) and leaves the
 *    outputs meaningless:
 *      PROSSTT_AMD_TRENDS_NEGATIVE      a negative count
 *      PROSSTT_AMD_TRENDS_INDEX_RANGE   an index outside [0, N): the entry is skipped
 *      PROSSTT_AMD_TRENDS_WEIGHT_RANGE  a weight outside [0, 4096]: the entry is skipped
 *      PROSSTT_AMD_TRENDS_ROW_RANGE     indptr does not ascend from 0 to nnz, or a row holds 2^20 entries or more: the
 *                                       offsets are clamped into [0, nnz]
 *  - Limits, refused with PROSSTT_AMD_TRENDS_EINVAL: 1 <= N < 2^31, 1 <= G <= 65535 * 256, ld >= G, 1 <= R < 2^31,
 *    0 <= nnz, entries_per_block >= 0, ceil(nnz / entries_per_block) + R < 2^31, NULL or misaligned pointers (int64 and
 *    uint64 arrays on 8 bytes, the workspace on 16; indices and weights may be NULL when nnz = 0), a workspace below the
 *    query's.
 */
#ifndef PROSSTT_AMD_TRENDS_H
#define PROSSTT_AMD_TRENDS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_TRENDS_OK = 0,
    PROSSTT_AMD_TRENDS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_TRENDS_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_TRENDS_ONE 4096
#define PROSSTT_AMD_TRENDS_MAX_ROW_ENTRIES ((1 << 20) - 1)

#define PROSSTT_AMD_TRENDS_NEGATIVE 1u
#define PROSSTT_AMD_TRENDS_INDEX_RANGE 2u
#define PROSSTT_AMD_TRENDS_WEIGHT_RANGE 4u
#define PROSSTT_AMD_TRENDS_ROW_RANGE 8u

const char* prosstt_amd_trends_last_error(void);

/* Device workspace (bytes) of _node_sums for these sizes.  entries_per_block as there.  Pure. */
int prosstt_amd_trends_workspace_bytes(int64_t R, int64_t G, int64_t nnz, int64_t entries_per_block, uint64_t* bytes);

/* The sums of the definition.  entries_per_block: the entries of one node that a block takes, 0 for the library's rule
 * clamp(ceil(nnz * ceil(G / 1024) / 1024), 64, 2^20) (about 1024 blocks), or any positive value; the results do not depend
 * on it. */
int prosstt_amd_trends_node_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const int64_t* indptr,
                                 const int32_t* indices, const int32_t* weights, int64_t R, int64_t nnz,
                                 int64_t entries_per_block, void* ws, uint64_t ws_bytes, int64_t* S1, uint64_t* S2,
                                 uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
