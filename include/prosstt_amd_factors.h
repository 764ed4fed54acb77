/*
 * prosstt_amd_factors.h -- the normal equations of a per-cell regression of a device count matrix on gene loadings, under
 * the count model's variance law (libprosstt_amd_factors.so; prosstt_amd/factors.py drives it and holds the GLM-PCA loop).
 *
 * It is prosstt_amd_regress.h with the roles swapped: there a gene has coefficients and a cell a design row, here a cell
 * has coefficients and a gene a row of loadings.  The count model (count_model.get_pr_umi): X[i][g] has mean mu and
 * variance a mu^2 + b mu, a = alpha[g], b = beta[g].  The regression puts log(mu / s_i) = sum_j L[g][j] C[i][j]: s_i the
 * cell's size factor, L (G x p) the loadings, C the cell's coefficients.  Everything is binary64 and every operation is
 * rounded on its own (no contraction).  For a cell i with a good size factor and a gene g with use == NULL or
 * use[g] >= 0, with x = X[i][g] >= 0 and s = s_i:
 *
 *     eta = sum_j L[g][j] C[i][j]           j ascending, from +0: the product is rounded, then added
 *     |eta| > 700 or not finite:            PROSSTT_AMD_FACTORS_ETA, the entry is skipped
 *     mu = s exp(eta)     d = a mu + b      (d not finite -- mu overflowed: PROSSTT_AMD_FACTORS_ETA, skipped)
 *     w = mu / d          u = (x - mu) / d
 *     U[j][i]    += L[g][j] u                                      the quasi-score
 *     I[jk][i]   += (L[g][j] L[g][k]) w        j <= k              the information; the two loadings are multiplied first
 *     L1 = log1p((a mu) / b)     T = a > 0 ? L1 / a : mu / b
 *     Q[i]       += x = 0 ? -T : (x / b) ((eta + log s) - (log b + L1)) - T
 *     used[i]    += 1
 *
 * jk = j p - j (j - 1) / 2 + (k - j): the upper triangle packed by rows, P2 = p (p + 1) / 2 entries.  Q is the
 * quasi-log-likelihood of prosstt_amd_regress.h, U its gradient in C and I the expectation of its negated Hessian; Q is
 * concave in a cell's coefficients.  Admissible parameters are finite with a >= 0 and b >= 1, as there.
 *
 * Conventions (as in prosstt_amd_regress.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_FACTORS_E* code otherwise; the message is in the thread-local
 *    last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of at least
 *    the bytes that the workspace query names for (N, G, p, genes_per_block).
 *  - Deterministic: a cell's terms are added in ascending gene order within a block of genes_per_block genes, and a
 *    finishing kernel adds the blocks' partial sums in ascending order.  No floating-point atomic; the only atomic is the
 *    OR of the status word.  Equal inputs and equal genes_per_block give equal bits on any stream, for any row stride and
 *    base alignment, for every `split`, and for a cell alone or among others: the rows are independent, so a matrix in
 *    chunks of cells is one call per chunk with the same genes_per_block.
 *  - genes_per_block: 0 is the library's choice for (N, G), what the gene-blocking query returns; otherwise a multiple of
 *    PROSSTT_AMD_FACTORS_TILE_GENES (one above 2^30 counts as 2^30).  At most 65535 blocks of genes.
 *  - split: how many of the p + P2 sums of (U, I) one block keeps in registers, 8, 16 or 32; 0 is the library's choice
 *    (16 for up to PROSSTT_AMD_FACTORS_SPLIT_16_MAX_SUMS sums, that is p <= 8, and 32 above).  The blocks of 256 cells
 *    and one range of genes that differ in their slice of the sums each form eta, mu, w and u again, by the same
 *    operations; Q and used come from a pass of their own over the same blocks.
 *  - X: row i, gene g at X[i*ld + g] (unit column stride, row stride ld >= G; any base alignment -- rows that start on 16
 *    bytes are read with 16-byte loads).
 *  - *status is only ever set (the caller zeroes it); with a bit set the outputs of that call are meaningless.  A cell
 *    with a bad size factor is skipped, and so is a gene with use[g] < 0, whose loadings and parameters are not judged.
 *    Every (a, b), every loading and every coefficient is judged before anything is computed with it: an inadmissible or
 *    non-finite pair sets its bit and the arithmetic runs on (0, 2) in its place, a non-finite coefficient or loading sets
 *    its bit and counts as 0.  A negative entry of X sets its bit and is skipped.
 *  - Limits, refused with PROSSTT_AMD_FACTORS_EINVAL: 1 <= N < 2^31, 1 <= G < 2^31, 1 <= p <= 16, ld >= G, ldl >= p,
 *    split one of 0, 8, 16, 32, genes_per_block >= 0 and a multiple of the gene tile, a workspace at least the query's.
 */
#ifndef PROSSTT_AMD_FACTORS_H
#define PROSSTT_AMD_FACTORS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_FACTORS_OK = 0,
    PROSSTT_AMD_FACTORS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_FACTORS_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_FACTORS_MAX_P 16
#define PROSSTT_AMD_FACTORS_SPLIT_16_MAX_SUMS 48
#define PROSSTT_AMD_FACTORS_TILE_GENES 32   /* genes of the LDS tile that transposes the matrix; genes_per_block is a multiple */
#define PROSSTT_AMD_FACTORS_MAX_GENE_BLOCKS 65535

/* (the bits keep regress's values; 2, its label bit, has no meaning here) */
#define PROSSTT_AMD_FACTORS_NEGATIVE 1u     /* status: a negative entry of X */
#define PROSSTT_AMD_FACTORS_PARAMETER 4u    /* status: an inadmissible or non-finite alpha or beta */
#define PROSSTT_AMD_FACTORS_SIZE 8u         /* status: a size factor that is not in (0, 1e150] */
#define PROSSTT_AMD_FACTORS_COEFFICIENT 16u /* status: a coefficient or a loading that is not finite */
#define PROSSTT_AMD_FACTORS_ETA 32u         /* status: |eta| > 700 or not finite, or a mean that overflowed */

const char* prosstt_amd_factors_last_error(void);

/* The library's choice of genes_per_block for an N x G matrix: a pure function of (N, G), a multiple of the gene tile. */
int prosstt_amd_factors_gene_blocking(int64_t N, int64_t G, int64_t* genes_per_block);

/* Device workspace (bytes) of the cell equations for an N x G matrix, p coefficients and genes_per_block (0: the
 * library's choice).  It does not depend on the split. */
int prosstt_amd_factors_workspace_bytes(int64_t N, int64_t G, int64_t p, int64_t genes_per_block, uint64_t* bytes);

/*
 * U[j*N + i], I[jk*N + i], Q[i], used[i] of the definition above.
 *   size       N binary64 size factors      use   G int32 (negative: the gene is left out), or NULL for every gene
 *   loadings   G x p binary64, row stride ldl
 *   coef       p x N binary64 (contiguous): coef[j*N + i] is C[i][j]
 *   alpha, beta   G binary64
 *   U          p x N binary64     I   P2 x N binary64     Q   N binary64     used   N uint64
 */
int prosstt_amd_factors_cell_equations(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                       const double* size, const int32_t* use, const double* loadings, int64_t ldl,
                                       int64_t p, const double* coef, const double* alpha, const double* beta,
                                       int32_t split, int64_t genes_per_block, void* ws, uint64_t ws_bytes, double* U,
                                       double* I, double* Q, uint64_t* used, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
