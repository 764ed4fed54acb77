/*
 * prosstt_amd_mapping.h -- the score of every cell of a count matrix at every node of a lineage tree on the device
 * (libprosstt_amd_mapping.so): the best node, its posterior and the posterior of every branch, from the Poisson
 * log-likelihood of the raw counts.  prosstt_amd/mapping.py builds the panel, drives the pass and holds the results.
 *
 * Definition.
 *
 *   Input.  X: N rows x G genes, int32, row i and gene g at X[i*ld + g], ld >= G, any base alignment, read in place.
 *   s: N binary64, the size factor of every row.  A panel P: R nodes x G genes, binary32, node r and gene g at
 *   P[r*ldp + g], ldp >= G (node-major, the row order of the tree's mean tensor).  m: R binary64, the exposure of every
 *   node.  c: R binary64, a constant of every node.  branch_offsets: B + 1 int64 ascending from 0 to R: the nodes of branch
 *   b are the rows branch_offsets[b] .. branch_offsets[b + 1] - 1.
 *
 *   The gene sum D[i][r].  The genes are cut into consecutive chains of genes_per_chain genes from gene 0 (a multiple of
 *   32 in 32 .. 4096; the last chain may be shorter).  Within a chain, sum_g float(x_ig) * P[r][g] is accumulated in
 *   binary32 by the fused multiply-adds of v_mfma_f32_32x32x2_f32, starting from +0: the chain's steps of 32 genes in
 *   ascending order, within a step the 16 instructions s = 0 .. 15, of which instruction s adds the products of the genes
 *   s and 16 + s of the step; float(x) is v_cvt_f32_i32 (a count of 2^24 or more rounds once, to nearest even).  The chain
 *   sums are converted to binary64 and added in ascending chain order from +0.  D[i][r] is a function of row i, row r of
 *   the panel and genes_per_chain only: it does not depend on the grid, the node tile, the stream, the other rows, ld, ldp or
 *   an alignment.
 *
 *   The score.  S[i][r] = (D[i][r] - s_i * m_r) + c_r in binary64, every operation rounded on its own (nothing is
 *   contracted).  With P[r][g] = log mean_rg and m_r = sum_g mean_rg this is the Poisson log-likelihood of row i at node
 *   r up to a constant of the row.
 *
 *   Per row:
 *     best        int32: the node of the largest S; of equal scores the lowest node; a NaN never wins.  If every score of
 *                 the row is NaN: node 0, and best_score is NaN.
 *     best_score  S[i][best].
 *     lse         log(sum_r exp(S[i][r] - best_score)) + best_score.  The sum: lane k of a wave adds the terms of the nodes
 *                 k, k + 64, ... in ascending order from 0, then the 64 partial sums are added by wave_reduce.h's butterfly.
 *     branch_lse  (optional, N x B at branch_lse[i*B + b]) the same over the nodes of branch b, around the largest score of
 *                 the branch (NaNs skipped in that maximum); -inf for a branch without nodes or whose scores are all -inf.
 *     scores      (optional, N x R binary64 at scores[i*R + r]) the whole of S.  NULL: S is kept in the workspace only.
 *
 * Kernels (256 threads, 64-bit offsets, no scratch, no floating-point atomic, no atomic but the status word's OR).
 *   mapping_pass_kernel<NT, VEC>   a block owns 128 rows (32 per wave) and a tile of 32 NT nodes, NT = 1 .. 4 (at most 2 by
 *                                  the library's rule), and loops over all genes.  Per step of 32 genes a lane loads 16 consecutive counts of its row (four 16-byte
 *                                  loads when VEC: rows 16-byte aligned), the block stages the 32 genes x 32 NT nodes slice of
 *                                  the panel in LDS (read along the genes, stored transposed), and every wave runs 16 matrix
 *                                  instructions per 32-node tile.  At a chain's end the 16 NT accumulators are added into
 *                                  binary64 registers and cleared.  The epilogue applies s_i m_r and c_r and stores S.
 *                                  Grid: (ceil(N / 128), ceil(R / (32 NT))).
 *   mapping_finish_kernel          one wave per row: the argmax, lse and branch_lse of the row of S.
 *
 * Conventions (as in prosstt_amd_trends.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_MAPPING_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_mapping_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of the queried
 *    size, 16-byte aligned.
 *  - Deterministic: equal inputs give identical outputs on any stream, for any node tile, and for a row alone or among
 *    others.
 *  - Nothing is read or written out of bounds whatever the arrays hold; what is wrong sets a bit of *status (the caller
 *    zeroes it; bits are only ever set, with an atomic OR):
 *      PROSSTT_AMD_MAPPING_NEGATIVE      a negative count (it is converted and multiplied as it is; the outputs are
 *                                        meaningless)
 *      PROSSTT_AMD_MAPPING_BRANCH_RANGE  branch_offsets do not ascend from 0 to R: the offsets are clamped into [0, R] and
 *                                        a branch that ends before it begins is empty
 *  - Limits, refused with PROSSTT_AMD_MAPPING_EINVAL: 1 <= N < 2^31, 1 <= G < 2^31, ld >= G, ldp >= G,
 *    1 <= R <= 65535 * 32 (the node tiles are the grid's second dimension, and a tile holds at least 32 nodes),
 *    genes_per_chain a multiple of 32 in 32 .. 4096, 1 <= B < 2^31 when branch_lse is given (B and branch_offsets are not
 *    looked at otherwise), NULL or misaligned pointers (binary64 and int64 arrays on 8 bytes, P and best on 4, the workspace
 *    on 16), a workspace below the query's.
 */
#ifndef PROSSTT_AMD_MAPPING_H
#define PROSSTT_AMD_MAPPING_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_MAPPING_OK = 0,
    PROSSTT_AMD_MAPPING_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_MAPPING_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_MAPPING_NEGATIVE 1u
#define PROSSTT_AMD_MAPPING_BRANCH_RANGE 2u

#define PROSSTT_AMD_MAPPING_MAX_NODES (65535 * 32)
#define PROSSTT_AMD_MAPPING_MAX_CHAIN 4096

const char* prosstt_amd_mapping_last_error(void);

/* Device workspace (bytes) of _node_scores for these sizes: the N x R scores.  Pure. */
int prosstt_amd_mapping_workspace_bytes(int64_t N, int64_t G, int64_t R, int64_t B, uint64_t* bytes);

/* The scores of the definition.  branch_lse and scores may be NULL; branch_offsets may be NULL when branch_lse is. */
int prosstt_amd_mapping_node_scores(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const double* s,
                                    const float* P, int64_t ldp, int64_t R, const double* m, const double* c,
                                    const int64_t* branch_offsets, int64_t B, int64_t genes_per_chain, void* ws,
                                    uint64_t ws_bytes, int32_t* best, double* best_score, double* lse, double* branch_lse,
                                    double* scores, uint32_t* status);

/* The same with the node tile chosen by the caller: node_tile = 1 .. 4 tiles of 32 nodes per block, 0 for the library's rule
 * min(2, ceil(R / 32)).  The results do not depend on it. */
int prosstt_amd_mapping_node_scores_tiled(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const double* s,
                                          const float* P, int64_t ldp, int64_t R, const double* m, const double* c,
                                          const int64_t* branch_offsets, int64_t B, int64_t genes_per_chain,
                                          int32_t node_tile, void* ws, uint64_t ws_bytes, int32_t* best, double* best_score,
                                          double* lse, double* branch_lse, double* scores, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
