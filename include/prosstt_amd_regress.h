/*
 * prosstt_amd_regress.h -- the normal equations of a per-gene regression of a device count matrix on a design, under the
 * count model's variance law (libprosstt_amd_regress.so; prosstt_amd/regress.py drives it and holds the Fisher scoring).
 *
 * The count model (count_model.get_pr_umi): X[i][g] has mean mu and variance a mu^2 + b mu, a = alpha[g], b = beta[g].
 * The regression puts log(mu / s_i) = sum_j D[l_i][j] C[g][j]: s_i the cell's size factor, l_i = labels[i] its row of the
 * design D (K x p), C the coefficients.  K is the number of nodes for a tree, the number of groups for a one-hot design,
 * and N with labels = 0 .. N - 1 for covariates per cell.  Everything is binary64 and every operation is rounded on its
 * own (no contraction).  For a cell i with 0 <= l = l_i < K (a negative label leaves the cell out, one >= K sets
 * PROSSTT_AMD_REGRESS_LABEL and leaves it out) and a gene g, with x = X[i][g] >= 0 and s = s_i:
 *
 *     eta = sum_j D[l][j] C[g][j]           j ascending, from +0: the product is rounded, then added
 *     |eta| > 700 or not finite:            PROSSTT_AMD_REGRESS_ETA, the entry is skipped
 *     mu = s exp(eta)     d = a mu + b      (d not finite -- mu overflowed: PROSSTT_AMD_REGRESS_ETA, skipped)
 *     w = mu / d          u = (x - mu) / d
 *     U[j][g]    += D[l][j] u                                      the quasi-score
 *     I[jk][g]   += (D[l][j] D[l][k]) w        j <= k              the information; the two design entries are multiplied first
 *     M[jk][g]   += (D[l][j] D[l][k]) (u u)    j <= k              the "meat", in I's place when `meat` is not 0
 *                                                                  (u u not finite: PROSSTT_AMD_REGRESS_ETA, no sum takes the entry)
 *     L1 = log1p((a mu) / b)     T = a > 0 ? L1 / a : mu / b
 *     Q[g]       += x = 0 ? -T : (x / b) ((eta + log s) - (log b + L1)) - T
 *     used[g]    += 1
 *
 * jk = j p - j (j - 1) / 2 + (k - j): the upper triangle packed by rows, P2 = p (p + 1) / 2 entries.
 * Q is the quasi-log-likelihood, the integral of (x - t) / (a t^2 + b t) dt from a constant of the entry up to mu: U is
 * its gradient in C and I the expectation of its negated Hessian; d2Q / d eta2 = -mu (b + a x) / d^2 < 0 for every
 * x >= 0, so Q is concave in C.  With b = 1 the equation U = 0 is the likelihood equation of the negative binomial
 * with known dispersion a; with a = 0 and b = 1 it is the Poisson regression.
 *
 * Admissible parameters are finite with a >= 0 and b >= 1: the rule of prosstt_amd_fit.h without its third clause
 * (a + b - 1 > 0), because the corner a = 0, b = 1 that has no likelihood there is the Poisson case here (d = 1).
 *
 * Conventions (as in prosstt_amd_fit.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_REGRESS_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_regress_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    prosstt_amd_regress_workspace_bytes bytes for (N, G, p).
 *  - Deterministic: a gene's terms are added in ascending row order within a block of rows, and a finishing kernel adds
 *    the blocks' partial sums in ascending order.  No floating-point atomic; the only atomic is the OR of the status
 *    word.  The blocking of the rows is a function of (N, ceil(G / 256)) alone: equal inputs give equal bits on any
 *    stream, for any row stride and base alignment, for a slice of the genes with the same row blocking, and for every
 *    `split`.
 *  - split: how many of the p + P2 sums of (U, I) one block keeps in registers, 8, 16 or 32; 0 is the library's choice
 *    (16 for up to PROSSTT_AMD_REGRESS_SPLIT_16_MAX_SUMS sums, that is p <= 8, and 32 above).  The blocks of one strip
 *    of genes and one range of rows that differ in their slice of the sums each form eta, mu, w and u again, by the same
 *    operations; Q and used come from a pass of their own over the same blocks of rows.
 *  - X: row i, gene g at X[i*ld + g] (unit column stride, row stride ld >= G; any base alignment -- rows that start on 16
 *    bytes are read with 16-byte loads).
 *  - *status is only ever set (the caller zeroes it); with a bit set the outputs of that call are meaningless.  A row
 *    with a label >= K or a bad size factor is skipped (nothing is read outside the arrays).  Every (a, b) and every
 *    coefficient is judged before anything is computed with it: an inadmissible or non-finite pair sets its bit and the
 *    arithmetic runs on (0, 2) in its place, a non-finite coefficient sets its bit and counts as 0, so the running time
 *    of a call does not depend on what the values are.  A negative entry of X sets its bit and is skipped.
 *  - Limits, refused with PROSSTT_AMD_REGRESS_EINVAL: 1 <= N < 2^31, 1 <= G <= (2^31 - 1) 256 / 154, 1 <= K < 2^31,
 *    1 <= p <= 16, ld >= G, ldd >= p, split one of 0, 8, 16, 32, a workspace at least the query's.
 */
#ifndef PROSSTT_AMD_REGRESS_H
#define PROSSTT_AMD_REGRESS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_REGRESS_OK = 0,
    PROSSTT_AMD_REGRESS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_REGRESS_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_REGRESS_MAX_P 16
#define PROSSTT_AMD_REGRESS_SPLIT_16_MAX_SUMS 48

#define PROSSTT_AMD_REGRESS_NEGATIVE 1u     /* status: a negative entry of X */
#define PROSSTT_AMD_REGRESS_LABEL 2u        /* status: a label >= K */
#define PROSSTT_AMD_REGRESS_PARAMETER 4u    /* status: an inadmissible or non-finite alpha or beta */
#define PROSSTT_AMD_REGRESS_SIZE 8u         /* status: a size factor that is not in (0, 1e150] (of a cell with a label >= 0) */
#define PROSSTT_AMD_REGRESS_COEFFICIENT 16u /* status: a coefficient that is not finite */
#define PROSSTT_AMD_REGRESS_ETA 32u         /* status: |eta| > 700 or not finite, or a mean or a squared residual that overflowed */

const char* prosstt_amd_regress_last_error(void);

/* Device workspace (bytes) of prosstt_amd_regress_normal_equations for an N x G matrix and p coefficients.  A pure
 * function of (N, G, p): it does not depend on the split. */
int prosstt_amd_regress_workspace_bytes(int64_t N, int64_t G, int64_t p, uint64_t* bytes);

/*
 * U[j*G + g], I_or_M[jk*G + g], Q[g], used[g] of the definition above.
 *   size     N binary64 size factors      labels  N int32 (row of the design per cell; negative: the cell is left out)
 *   design   K x p binary64, row stride ldd
 *   coef     p x G binary64 (contiguous): coef[j*G + g] is C[g][j]
 *   alpha, beta   G binary64
 *   meat     0: the information I; otherwise the meat M in its place
 *   U        p x G binary64     I_or_M   P2 x G binary64     Q   G binary64     used   G uint64
 */
int prosstt_amd_regress_normal_equations(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                         const double* size, const int32_t* labels, int64_t K, const double* design,
                                         int64_t ldd, int64_t p, const double* coef, const double* alpha,
                                         const double* beta, int32_t meat, int32_t split, void* ws, uint64_t ws_bytes,
                                         double* U, double* I_or_M, double* Q, uint64_t* used, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
