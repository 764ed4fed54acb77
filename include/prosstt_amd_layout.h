/*
 * prosstt_amd_layout.h -- UMAP layouts of the connectivity graph of cells, on the device (libprosstt_amd_layout.so).
 *
 * The reference's example notebooks call scanpy.tl.umap on the neighbour graph and plot obsm["X_umap"].  The matrix W of
 * prosstt_amd_graph.h is the fuzzy simplicial set such a layout starts from; this library is the optimiser: the epochs of
 * the stochastic layout in their SYNCHRONOUS form.  umap-learn's optimiser is an in-place SGD whose threads race; here
 * every epoch reads the positions the previous epoch wrote and writes new ones, so that every sum has a fixed order, no
 * atomic is needed, and an epoch can be checked against a binary64 model.  (The correspondences with umap-learn below are
 * from reading it, not from a run.)
 *
 * Definition.  Coordinates are binary32, schedules binary64.
 *
 *   Input.  W in CSR as prosstt_amd_graph.h leaves it: N rows, symmetric, indptr int64 (N + 1), indices int32, 3 <= N <
 *   2^31; p[e] = W[e] / max(W) (binary64, one IEEE division, the caller's) for CSR position e, 0 <= p <= 1.  Positions Y
 *   are N x c, row-major binary32, c = 2 or 3.
 *
 *   Parameters.  E = n_epochs, 1 <= E <= 4096.  a, b, gamma, alpha0: binary64, finite, a > 0, b > 0, gamma >= 0, alpha0 >
 *   0; a, b and gamma are rounded to binary32 once, and those rounded values are the ones meant below.  r =
 *   negative_sample_rate, 0 <= r <= 31.  seed: any uint64.
 *
 *   Epoch n (0-based), for every row i independently, every read from Y^n:
 *     - Entry e = (i, j) is ACTIVE iff floor((n + 1) p_e) > floor(n p_e), a binary64 product and floor.  The rule has no
 *       state; over E epochs an edge is sampled floor(E p_e) times, so an edge with p < 1 / E never is (umap-learn's
 *       epochs_per_sample schedule and its pruning of weak edges).
 *     - Attraction, per active entry: delta = y_i - y_j, d2 = sum delta^2, coef = -2 a b d2^(b - 1) / (a d2^b + 1) if d2 >
 *       0, else 0; term = 2 clip(coef delta, -4, 4) per coordinate.  (The factor 2: W stores the pair in both directions
 *       with equal p, and umap-learn moves both ends on each sample.)
 *     - Repulsion, per active entry and s = 0 .. r - 1: k = ((h >> 32) N) >> 32 with h = mix(base_n ^ (32 e + s)), base_n =
 *       mix(seed + 0x9E3779B97F4A7C15 (n + 1)), e the CSR position as uint64, all arithmetic modulo 2^64, and
 *           mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31.
 *       If k = i there is no term.  Otherwise delta = y_i - y_k, coef = 2 gamma b / ((0.001 + d2) (a d2^b + 1)) if d2 > 0,
 *       else 0; term = clip(coef delta, -4, 4).
 *     - alpha_n = alpha0 (1 - n / E), computed in binary64 and rounded to binary32.
 *     - y_i^(n+1) = y_i^n + alpha_n sum(terms).
 *
 *   Evaluation.  delta, d2 (coordinates added in ascending order), the coefficients and the terms are binary32 with every
 *   operation rounded on its own (-ffp-contract=off).  d2^b is the device library's powf(d2, b); d2^(b - 1) is that value
 *   divided by d2 (an IEEE division), so there is one powf per pair; -2 a b and 2 gamma b are formed in binary64 from the
 *   rounded a, b, gamma and rounded once.  The caller keeps d2^b within binary32's range (|y| below 1e12 does for b <= 1.5).
 *   A group of lanes_per_row lanes owns a row.  The row's items -- item t = (entry t / (1 + r), slot t % (1 + r)), slot 0
 *   the attraction and slot s + 1 the negative sample s -- are dealt round-robin: lane l takes items l, l + lanes_per_row,
 *   ...  A lane adds its terms in ascending item order; the lanes' sums are added with a fixed xor shuffle tree; then one
 *   multiplication by alpha_n and one addition to y_i.  Equal inputs and an equal lanes_per_row give equal bits on every
 *   run and every stream.  There is no floating-point atomic.
 *
 * Conventions (as in prosstt_amd_graph.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_LAYOUT_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_layout_last_error().  Bad arguments are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory.
 *  - The kernels trust indptr and indices (0 = indptr[0] <= indptr[1] <= .. <= indptr[N] = nnz, 0 <= indices < N) and
 *    stay within Y for every p; a p outside [0, 1] or a NaN only changes which entries are active.
 *  - Kernels use 256-thread blocks, 64-bit offsets and no scratch.
 */
#ifndef PROSSTT_AMD_LAYOUT_H
#define PROSSTT_AMD_LAYOUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_LAYOUT_OK = 0,
    PROSSTT_AMD_LAYOUT_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_LAYOUT_EHIP = -3    /* HIP runtime error */
};

const char* prosstt_amd_layout_last_error(void);

/* Epochs epoch_begin .. epoch_end - 1 of the definition, one launch each, back to back: the first reads y0 and writes y1,
 * the next reads y1 and writes y0, and so on; the result lies in y1 if epoch_end - epoch_begin is odd and in y0 otherwise
 * (y0 is untouched when the range is empty or holds one epoch).  0 <= epoch_begin <= epoch_end <= n_epochs.  lanes_per_row:
 * 4, 16 or 64; 0: the library chooses (64, or 16 below 16 items per mean row).  y1 must not alias y0; c must be 2 or 3. */
int prosstt_amd_layout_epochs(void* stream, const int64_t* indptr, const int32_t* indices, const double* p /* nnz */,
                              int64_t N, int64_t nnz, int32_t c, float* y0 /* N x c */, float* y1 /* N x c */,
                              int32_t epoch_begin, int32_t epoch_end, int32_t n_epochs, double a, double b, double gamma,
                              double alpha0, int32_t negative_sample_rate, uint64_t seed, int32_t lanes_per_row);

/* The probe of the hash: out[(e - e_begin) rate + s] = the k of the definition for entry e, sample s and this epoch and
 * N, for e_begin <= e < e_begin + count and 0 <= s < rate.  0 <= epoch < 4096, 0 <= rate <= 31, 3 <= N < 2^31, e_begin >=
 * 0, count >= 0.  Nothing is enqueued when count rate = 0. */
int prosstt_amd_layout_negatives(void* stream, uint64_t seed, int32_t epoch, int64_t e_begin, int64_t count, int32_t rate,
                                 int64_t N, int32_t* out /* count x rate */);

#ifdef __cplusplus
}
#endif
#endif
