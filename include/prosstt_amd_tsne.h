/*
 * prosstt_amd_tsne.h -- exact t-SNE of the cells on the device (libprosstt_amd_tsne.so): the affinities of a kNN graph,
 * the gradient over all N^2 pairs, scikit-learn's gradient descent on it, and the objective.
 *
 * The reference's example notebooks draw their branch pictures from scanpy.tl.tsne.  CPU libraries approximate the
 * repulsion (Barnes-Hut); here every pair is evaluated, in a fixed order, so equal calls give equal bits.
 *
 * Definition.  Affinities are binary64.  Positions, gradient, update and gains are binary32.  The normaliser Z and the
 * sums across tiles and slabs are binary64.
 *
 *   Conditional affinities (N x k, one wave per row).  The input is that of prosstt_amd_graph_memberships: index[i*k + r]
 *   and sqdist[i*k + r] (binary32, widened to binary64: d2).  3 <= N < 2^31, 2 <= k <= min(N - 1, 1024), 1 < perplexity <
 *   k.  For row i: g_j = d2_j - min_j d2_j, target = log(perplexity).  For a given beta: p_j = exp(-beta g_j), S = sum p_j,
 *   H(beta) = log S + beta (sum g_j p_j) / S.  beta_i comes from exactly this bisection, 64 steps, no early exit:
 *       lo = 0; hi = inf; beta = 1
 *       repeat 64 times:
 *           if H(beta) > target:  lo = beta;  beta = (hi == inf) ? 2 beta : (lo + hi) / 2
 *           else:                 hi = beta;  beta = (lo + hi) / 2
 *   and p_{j|i} = p_j / S at the last beta.  (scikit-learn's _binary_search_perplexity with the root found to full
 *   precision instead of its 1e-5 early exit, and with the shift by the row minimum, which cancels in p_j / S.)  A row
 *   whose distances are all equal ends with beta = 2^64 and p = 1 / k exactly.
 *
 *   Joint affinities.  P = (A + A^T) / (2 N), A the N x N matrix of the p_{j|i}, in CSR as the graph library holds W:
 *   indptr int64 (N + 1), indices int32 ascending within a row, data binary64, no diagonal.  Each value is (a + b) / (2 N):
 *   one IEEE addition (b = 0 where only one direction is listed: a + 0 = a) and one IEEE division, so P is symmetric to
 *   the bit.  The transpose is the graph library's keyed emit, the caller's sort, and _symmetrize_fold below, which adds
 *   where the graph library's fold takes the fuzzy union.
 *
 *   Gradient at positions Y (N x c row-major, c = 2 or 3) and exaggeration x (rounded to binary32 once).
 *     q of a pair (i, j): delta = y_i - y_j per coordinate, d2 = delta_0 delta_0, then d2 = fmaf(delta_c, delta_c, d2) for c
 *     = 1 .., w = 1 + d2, q = the hardware reciprocal of w (v_rcp_f32: within 1 ulp).
 *     Repulsion, over ALL pairs, j = i included: z_i += q, r_i += (q q) delta by fmaf.  The self term adds exactly 1 to z_i
 *     and 0 to r_i.  The columns are cut into global tiles of PROSSTT_AMD_TSNE_TILE columns; within a tile a row's sums
 *     are binary32 chains in ascending column order, and after each tile they are added to binary64 accumulators.  The
 *     tiles are dealt to `slabs` consecutive runs of ceil(tiles / slabs) whole tiles (trailing slabs may be empty), one
 *     block column each; slab partials are binary64 in the workspace and are added in ascending slab order: z_i and R_i.
 *     Z = (sum_i z_i) - N, a binary64 reduction of fixed order: a thread adds every 256th row of its block's run of rows
 *     in ascending order, a fixed tree adds the threads, and a fixed tree adds the blocks.  There is no atomic: equal
 *     inputs and equal `slabs` give equal bits on every run and stream.  slabs = 0 lets the library choose the smallest
 *     count that gives 4 blocks per CU of the MI355X's 256 (at most one tile per slab).
 *     Attraction, one wave per row: for entry e = (i, j) of P, term = ((float)P_e q_e) delta.  Lane l takes entries l, l +
 *     64, .. of the row and adds its terms in ascending order; a fixed xor shuffle tree adds the lanes: att_i, binary32.
 *     Combination: rep_i = (float)(R_i / Z), a binary64 division; grad_i = 4 (x att_i - rep_i) in binary32, each
 *     operation rounded.
 *
 *   Iteration n (scikit-learn's _gradient_descent without its early stops), synchronous: Y^n is read, Y^(n+1) written.
 *   Per coordinate, binary32, every operation rounded on its own:
 *       gain = (update grad < 0) ? gain + 0.2f : gain 0.8f;  gain = max(gain, 0.01f)
 *       update = mu update - (eta gain) grad;  y += update
 *   Iterations n < exploration use x = early_exaggeration and mu = 0.5, later ones x = 1 and mu = 0.8; eta is the learning
 *   rate; early_exaggeration and eta are rounded to binary32 once.
 *
 *   Objective.  row_i = sum_e P_e (log P_e + log1p(d2_e)) over the row's entries, binary64 (d2_e the binary32 value above,
 *   widened); an entry with P_e = 0 adds nothing; lanes as in the attraction.  KL = sum_i row_i + (sum P) log Z.
 *
 * Conventions (as in prosstt_amd_graph.h and prosstt_amd_layout.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_TSNE_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_tsne_last_error.  Bad sizes, aliases and parameters are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers, rows contiguous.  All work is enqueued on the caller's stream (NULL: the default
 *    stream of the current device); nothing synchronises, nothing allocates device memory.
 *  - _affinities checks its values on the device: a wave that meets a bad one sets the condition's byte of *status (a
 *    device word the caller zeroes and reads back; a plain one-byte store of the constant 1, so no atomic is needed) and
 *    stays within bounds.  PROSSTT_AMD_TSNE_BAD_* name the bits.  The other entries trust indptr and indices (0 =
 *    indptr[0] <= .. <= indptr[N] = nnz, 0 <= indices < N).
 *  - Kernels use 256-thread blocks, 64-bit offsets, no scratch and no atomic.
 */
#ifndef PROSSTT_AMD_TSNE_H
#define PROSSTT_AMD_TSNE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_TSNE_OK = 0,
    PROSSTT_AMD_TSNE_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_TSNE_EHIP = -3    /* HIP runtime error */
};

/* bits of *status: one byte of the word each */
enum {
    PROSSTT_AMD_TSNE_BAD_INDEX = 1,          /* an index outside [0, N) */
    PROSSTT_AMD_TSNE_BAD_SELF = 1 << 8,      /* an index equal to its row */
    PROSSTT_AMD_TSNE_BAD_DISTANCE = 1 << 16  /* a squared distance that is negative, infinite or NaN */
};

#define PROSSTT_AMD_TSNE_TILE 256       /* T: columns of a tile of the repulsion */
#define PROSSTT_AMD_TSNE_MAX_SLABS 1024

const char* prosstt_amd_tsne_last_error(void);

/* Device workspace (bytes) of _gradient and _iterations for these sizes; slabs as there (0: the library's choice).  Pure. */
int prosstt_amd_tsne_workspace_bytes(int64_t N, int32_t c, int32_t slabs, uint64_t* bytes);

/* cond[i*k + r] = p_{j|i} and beta[i] of the definition; the value checks of index and sqdist go to *status. */
int prosstt_amd_tsne_affinities(void* stream, const int32_t* index /* N x k */, const float* sqdist /* N x k */, int64_t N,
                                int64_t k, double perplexity, double* cond /* N x k */, double* beta /* N */,
                                uint32_t* status);

/* Step 3 of the graph library's symmetrisation with this library's fold: the run of a key folds to (sum of its values) /
 * (2 N).  sorted_keys, perm, pos: M = 2 N k int64 each; ws: the graph library's workspace for (N, k), which still holds
 * the values of its emit step; nnz = pos[M - 1]. */
int prosstt_amd_tsne_symmetrize_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm, const int64_t* pos,
                                     int64_t N, int64_t k, int64_t nnz, const void* ws, uint64_t ws_bytes,
                                     int64_t* indptr /* N + 1 */, int32_t* indices /* nnz */, double* data /* nnz */);

/* grad and *z = Z of the definition at y.  1 <= slabs <= PROSSTT_AMD_TSNE_MAX_SLABS, or 0; ws: _workspace_bytes(N, c, slabs)
 * bytes, 16-byte aligned.  rep_abs: NULL, or N x c sums of |q q delta| in the repulsion's order (what an error bound is
 * scaled by: for tests).  exaggeration finite and > 0.  grad must not alias y. */
int prosstt_amd_tsne_gradient(void* stream, const int64_t* indptr, const int32_t* indices, const double* P /* nnz */,
                              int64_t N, int64_t nnz, int32_t c, const float* y /* N x c */, double exaggeration,
                              int32_t slabs, void* ws, uint64_t ws_bytes, float* grad /* N x c */, double* z /* 1 */,
                              double* rep_abs /* N x c, or NULL */);

/* Iterations it_begin .. it_end - 1 of the definition, back to back: the first reads y0 and writes y1, the next reads y1
 * and writes y0, and so on; the result lies in y1 if it_end - it_begin is odd and in y0 otherwise.  update and gains (N x c
 * each) are read and written in place.  0 <= it_begin <= it_end <= 2^30, exploration >= 0; early_exaggeration and
 * learning_rate finite and > 0.  y0, y1, update and gains must not alias each other. */
int prosstt_amd_tsne_iterations(void* stream, const int64_t* indptr, const int32_t* indices, const double* P, int64_t N,
                                int64_t nnz, int32_t c, float* y0, float* y1, float* update, float* gains,
                                int32_t it_begin, int32_t it_end, int32_t exploration, double early_exaggeration,
                                double learning_rate, int32_t slabs, void* ws, uint64_t ws_bytes);

/* rows[i] = row_i of the objective at y. */
int prosstt_amd_tsne_objective(void* stream, const int64_t* indptr, const int32_t* indices, const double* P, int64_t N,
                               int64_t nnz, int32_t c, const float* y, double* rows /* N */);

#ifdef __cplusplus
}
#endif
#endif
