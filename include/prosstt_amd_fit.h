/*
 * prosstt_amd_fit.h -- the log-likelihood of the count model over a device count matrix, for several candidate
 * parameter pairs per gene at once (libprosstt_amd_fit.so; prosstt_amd/fit.py drives it and holds the optimiser).
 *
 * The count model (count_model.get_pr_umi): X[i][g] is negative binomial with mean mu = s_i m[k][g] and variance
 * alpha mu^2 + beta mu.  For cell i with label k = labels[i] >= 0 (a negative label leaves the cell out), gene g and
 * candidate c with a = alpha[c][g], b = beta[c][g], everything in binary64:
 *
 *     mu = s_i m[k][g]
 *     mu = 0:  the entry contributes 0; if x > 0 it is counted in bad[g]   (the sampler draws 0 from a mean of 0)
 *     theta = a mu + (b - 1)      r = mu / theta      L1 = log1p(theta)
 *     term = lgd(r, x) - r L1 + x (log theta - L1)      lgd(r, x) = lgamma(r + x) - lgamma(r),  lgd(r, 0) = 0
 *     ll[c][g] = sum_i term       base[g] = sum_i lgamma(x + 1)      (ll - base is the full log-likelihood)
 *
 * Admissible parameters are finite with a >= 0, b >= 1 and a + b - 1 > 0; then theta > 0 for every entry that is
 * evaluated.  b = 1 is the textbook negative binomial with dispersion a, a = 0 the quasi-Poisson end.
 *
 * How the term is formed (tests/fit_model.py is the same in numpy)
 *     inv = 1 / theta;  r = mu inv;  log theta - L1 = -log1p(inv)   (no cancellation at large theta)
 *     x = 0:        term = -(r L1)
 *     1 <= x <= 12: lgd = log(prod_{j < x} (r + j)), or x log r when r > 1e17 (the product would near overflow)
 *     x > 12:       k = ceil(16 - r) for r < 16, else 0;  P = prod_{j < k} (r + j);  z = r + k;  n = x - k;  t = z + n
 *                   lgd = n log t + ((z - 1/2) log1p(n / z) - n) + (S(t) - S(z)) + log P
 *                   S(t) = u (1/12 - u^2 (1/360 - u^2 (1/1260 - u^2 (1/1680 - u^2 / 1188)))),  u = 1 / t
 *     lgamma(x + 1) is lgd(1, x).  Every operation is rounded on its own (no contraction).
 *
 * Conventions (as in prosstt_amd_hvg.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_FIT_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_fit_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    prosstt_amd_fit_workspace_bytes bytes for (N, G, C).
 *  - Deterministic: a gene's terms are added in ascending row order within a block of rows, and a finishing kernel adds
 *    the blocks' partial sums in ascending order (no floating-point atomics).  The blocking of the rows is a function of
 *    (N, ceil(G / 256)) alone: equal inputs give equal bits on any stream, for any row stride and base alignment, for
 *    any C and position of a candidate among the C, and for a slice of the genes with the same row blocking.
 *  - X: row i, gene g at X[i*ld + g] (unit column stride, row stride ld >= G; any base alignment -- rows that start on 16
 *    bytes are read with 16-byte loads).
 *  - *status is only ever set (the caller zeroes it); with a bit set the outputs of that call are meaningless.  A row
 *    with a label >= K or a bad size factor is skipped (nothing is read outside the arrays).  Every candidate is judged
 *    before anything is computed with it: an inadmissible or non-finite pair sets its bit and the arithmetic runs on
 *    (a, b) = (0, 2) in its place, so the running time of a call does not depend on what the parameters are.  Size
 *    factors and means above 1e150 count as not finite (bits 8 and 16), so that mu = s m never overflows.
 *  - Limits, refused with PROSSTT_AMD_FIT_EINVAL: 1 <= N < 2^31, 1 <= G <= (2^31 - 1) 256 / 17, 1 <= K < 2^31, 1 <= C <= 16, ld >= G,
 *    ldm >= G, a workspace at least the query's.
 */
#ifndef PROSSTT_AMD_FIT_H
#define PROSSTT_AMD_FIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_FIT_OK = 0,
    PROSSTT_AMD_FIT_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_FIT_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_FIT_MAX_CANDIDATES 16

#define PROSSTT_AMD_FIT_NEGATIVE 1u   /* status: a negative entry of X */
#define PROSSTT_AMD_FIT_LABEL 2u      /* status: a label >= K */
#define PROSSTT_AMD_FIT_PARAMETER 4u  /* status: an inadmissible or non-finite alpha or beta */
#define PROSSTT_AMD_FIT_SIZE 8u       /* status: a size factor that is not in (0, 1e150] (of a cell with a label >= 0) */
#define PROSSTT_AMD_FIT_MEAN 16u      /* status: a mean that is not in [0, 1e150] (in a row of means that a label names) */

const char* prosstt_amd_fit_last_error(void);

/* Device workspace (bytes) of prosstt_amd_fit_loglik for an N x G matrix and C candidates.  A pure function of (N, G, C). */
int prosstt_amd_fit_workspace_bytes(int64_t N, int64_t G, int64_t C, uint64_t* bytes);

/*
 * ll[c*G + g], base[g], bad[g] of the definition above.
 *   size    N binary64 size factors       labels  N int32 (row of means per cell; negative: the cell is left out)
 *   means   K x G binary64, row stride ldm: the means at unit size
 *   alpha, beta   C x G binary64 (contiguous)
 *   ll      C x G binary64     base   G binary64     bad   G uint64
 */
int prosstt_amd_fit_loglik(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const double* size,
                           const int32_t* labels, int64_t K, const double* means, int64_t ldm, const double* alpha,
                           const double* beta, int64_t C, void* ws, uint64_t ws_bytes, double* ll, double* base,
                           uint64_t* bad, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
