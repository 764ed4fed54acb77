/*
 * prosstt_amd_dpt.h -- diffusion pseudotime of the cells and its first branching on the device (libprosstt_amd_dpt.so):
 * the distance rows of a diffusion map, and the concordance sums over all N^2 pairs that the branching is read from.
 *
 * Diffusion pseudotime (DPT, Haghverdi et al. 2016; scanpy.tl.dpt) is the step that a diffusion map is computed for: a
 * pseudotime and a branch per cell.  The rule for the distance weights is from memory of scanpy's _get_dpt_row, not from a
 * run of it.  The branching is defined here in full: it follows the 2016 paper and the outline of scanpy's "haghverdi16"
 * flavour and is a copy of neither (tau-a where scanpy takes scipy's tau-b once and approximate updates after it, an exact
 * scan of every split point, and no special treatment of connected components).
 *
 * Definition.
 *
 *   Input.  The eigenvalues lambda (n_comps, descending) and unit eigenvectors Psi (N x n_comps, binary64) of a diffusion
 *   map; 3 <= N < 2^31, 1 <= n_dcs <= n_comps.  The weights w_l, l < n_dcs, are computed by the CALLER on the host, in
 *   binary64: w_l = lambda_l / (1 - lambda_l) where lambda_l < 0.9994, and w_l = 1 otherwise (the division is not
 *   evaluated where it is not selected: lambda_0 is 1).
 *
 *   Distance row of a source cell s.  For cell j: acc = 0; for l = 0 .. n_dcs - 1 ascending: t = w_l (psi_sl - psi_jl),
 *   acc = acc + t t.  Every operation is a binary64 operation rounded on its own (nothing is fused).  d(s, j) = sqrt(acc).
 *
 *   Pseudotime.  d(root, .) / max_j d(root, j).  A cell that the root's component does not reach gets whatever the
 *   eigenvectors give it (scanpy sets infinity): a disconnected graph is the caller's problem, as in the graph library.
 *
 *   Branching.  Every argmax takes the lowest index among equals.
 *     Tips.  t0 = argmax d(root, .), t1 = argmax d(t0, .), t2 = argmax (d(t0, .) + d(t1, .)).
 *     Per rotation (a, b, c) of (t0, t1, t2), that is (t0, t1, t2), (t1, t2, t0) and (t2, t0, t1): `order` is the stable
 *     ascending sort of d(a, .); ru and rv are the dense int32 ranks of d(b, .)[order] and d(c, .)[order] (equal values get
 *     equal ranks, the smallest value rank 0: unique with return_inverse).  For positions p, q:
 *         s_pq = sgn(ru_p - ru_q) sgn(rv_p - rv_q), a value in {-1, 0, 1}, symmetric in (p, q),
 *     and the concordance sums, exact integers (what _concordance computes):
 *         lower_r = sum_{p < r} s_pr,   upper_r = sum_{q > r} s_rq.
 *     Split scan (the caller's, on int64, exact): H(n) = sum_{r < n} lower_r is the sum over the pairs inside the first n
 *     positions, T(n) = sum_{r >= n} upper_r the sum over the pairs inside the rest.  H(n), T(n) and the pair counts n (n -
 *     1) / 2 and (N - n)(N - n - 1) / 2 (int64) are each rounded to binary64, and
 *         diff(n) = H(n) / (n (n - 1) / 2) - T(n) / ((N - n)(N - n - 1) / 2)
 *     is two divisions and a subtraction.  n* = argmax of diff(n) over m <= n <= N - m, m = the smallest group, 2 <= m, 2 m
 *     <= N.  Near tip a the distances to b and c move together (Kendall's tau-a of the head near +1) and past the
 *     branching against each other (tau-a of the tail near -1), so the head order[:n*] is tip a's arm.
 *     Groups.  A cell in exactly one of the three heads gets 1, 2 or 3 (for t0, t1, t2); a cell in none or in several
 *     gets 0, the branching region.
 *
 * Kernels.
 *   dpt_rows_kernel         one thread per (source, cell); the weights and the source's coordinates are uniform across the
 *                           block.  A source outside [0, N) gives a row of NaN and reads nothing out of bounds.
 *   dpt_concordance_kernel  pure integer.  A block owns PROSSTT_AMD_DPT_BLOCK_ROWS rows (two per thread, 256 apart), one slab
 *                           of column tiles of PROSSTT_AMD_DPT_TILE columns and one sequence pair of the batch.  A tile's (ru,
 *                           rv) pairs are staged in LDS and read as a broadcast.  A tile wholly below or above the block's
 *                           rows adds to lower or upper without an index compare; only the tiles that meet the block's rows
 *                           compare the column with the row.  The tiles are dealt to `slabs` consecutive runs of ceil(tiles /
 *                           slabs) whole tiles (trailing slabs may be empty); a slab's partial sums are int32 in the
 *                           workspace, exact since |sum| < N < 2^31.
 *   dpt_reduce_kernel       adds the slabs' partial sums into int64.
 *   Integer sums do not depend on their order: the results are the same for every `slabs`, run and stream.
 *
 * Conventions (as in prosstt_amd_graph.h and prosstt_amd_tsne.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_DPT_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_dpt_last_error.  Bad sizes and pointers are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory.
 *  - _concordance trusts nothing about the ranks' values: any int32 values give the sums of the formula above, as long as
 *    their differences fit int32 (ranks in [0, N) do).
 *  - Kernels use 256-thread blocks, 64-bit offsets, no scratch and no atomic.
 */
#ifndef PROSSTT_AMD_DPT_H
#define PROSSTT_AMD_DPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_DPT_OK = 0,
    PROSSTT_AMD_DPT_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_DPT_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_DPT_TILE 256        /* columns of a tile of the concordance sums */
#define PROSSTT_AMD_DPT_BLOCK_ROWS 512  /* rows of a block of the concordance sums */
#define PROSSTT_AMD_DPT_MAX_SLABS 1024
#define PROSSTT_AMD_DPT_MAX_BATCH 1024
#define PROSSTT_AMD_DPT_MAX_SOURCES 65535

const char* prosstt_amd_dpt_last_error(void);

/* Device workspace (bytes) of _concordance for these sizes; slabs as there (0: the library's choice).  Pure. */
int prosstt_amd_dpt_workspace_bytes(int64_t N, int32_t batch, int32_t slabs, uint64_t* bytes);

/* out[i*N + j] = d(sources[i], j) of the definition.  vectors: N rows of row_stride >= n_dcs binary64 values each, of
 * which the first n_dcs are read; weights: n_dcs; sources: n_sources cell indices, 1 <= n_sources <=
 * PROSSTT_AMD_DPT_MAX_SOURCES.  out must not alias vectors. */
int prosstt_amd_dpt_rows(void* stream, const double* vectors, int64_t row_stride, const double* weights, int64_t N,
                         int64_t n_dcs, const int64_t* sources, int64_t n_sources, double* out /* n_sources x N */);

/* lower[b*N + r] and upper[b*N + r] of the definition for the sequence pairs (ru[b*N + .], rv[b*N + .]), b < batch.  1 <=
 * batch <= PROSSTT_AMD_DPT_MAX_BATCH; 1 <= slabs <= PROSSTT_AMD_DPT_MAX_SLABS, or 0: the smallest count that gives 4 blocks
 * per CU of the MI355X's 256 (at most one tile per slab); workspace: _workspace_bytes(N, batch, slabs) bytes, 16-byte
 * aligned. */
int prosstt_amd_dpt_concordance(void* stream, const int32_t* ru /* batch x N */, const int32_t* rv /* batch x N */, int64_t N,
                                int32_t batch, int32_t slabs, void* workspace, uint64_t bytes, int64_t* lower /* batch x N */,
                                int64_t* upper /* batch x N */);

#ifdef __cplusplus
}
#endif
#endif
