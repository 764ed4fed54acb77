/*
 * prosstt_amd_hvg.h -- the passes over a device count matrix that choosing highly variable genes needs
 * (libprosstt_amd_hvg.so; prosstt_amd/hvg.py drives them).
 *
 * Between normalisation and PCA the single-cell toolchains keep the few thousand genes whose variance stands out
 * against the trend of variance over mean (scanpy's pp.highly_variable_genes).  Two definitions are in use:
 *   seurat_v3  works on the counts: a loess of log10(variance) on log10(mean) gives every gene a regularised standard
 *              deviation; the counts of a gene are clipped at clip[j] = reg_std[j] * sqrt(N) + mean[j], and the variance of
 *              the clipped, standardised counts ranks the genes.  Mean and variance come from the exact sums of
 *              prosstt_amd_stats_count_summary; the clipped sums need the matrix again, once the clip values are known:
 *              prosstt_amd_hvg_clipped_sums.
 *   seurat     works on y = x / s (what expm1 of the log-normalised entry stands for): the dispersion variance / mean of y,
 *              standardised within bins of the mean.  It needs per gene the sums of y and y^2:
 *              prosstt_amd_hvg_normalized_moments.
 * Everything downstream then reads the chosen genes only: prosstt_amd_hvg_gather_columns writes them as a new matrix.
 *
 * Conventions (as in prosstt_amd_stats.h and prosstt_amd_embed.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_HVG_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_hvg_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    prosstt_amd_hvg_workspace_bytes bytes for (N, G) (enough for each of the two reductions; the gather needs none).
 *  - Deterministic: reductions go through partial slabs in the workspace that a finishing kernel sums in a fixed order
 *    (no floating-point atomics).  The integer results are exact, so they depend on no launch geometry at all; the
 *    binary64 sums are equal to the bit for equal inputs on any stream.
 *  - X: row r, gene g at X[r*ld + g] (unit column stride, row stride ld >= G; any base alignment -- rows that start on 16
 *    bytes are read with 16-byte loads).
 *  - *status is only ever set (the caller zeroes it): bit 0 (value 1) for a negative entry of X, bit 1 (value 2) for a
 *    negative threshold or a column outside the matrix.  With a bit set the outputs of that call are meaningless, except
 *    where stated.
 *  - Limits, refused with PROSSTT_AMD_HVG_EINVAL: 1 <= N < 2^31, 1 <= G, ld >= G, 1 <= n_sel < 2^31, ldy >= n_sel, a
 *    workspace at least the query's.
 */
#ifndef PROSSTT_AMD_HVG_H
#define PROSSTT_AMD_HVG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_HVG_OK = 0,
    PROSSTT_AMD_HVG_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_HVG_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_HVG_NEGATIVE 1u /* status: a negative entry of X */
#define PROSSTT_AMD_HVG_RANGE 2u    /* status: a negative threshold, or a column outside [0, G) */

const char* prosstt_amd_hvg_last_error(void);

/* Device workspace (bytes) that each of the two reductions below needs for an N x G matrix.  A pure function of (N, G). */
int prosstt_amd_hvg_workspace_bytes(int64_t N, int64_t G, uint64_t* bytes);

/*
 * Exact sums of the counts of every gene on either side of its own threshold (threshold: G int32 on the device, each >= 0):
 *   n_over[j]             = #{i : X[i][j] > threshold[j]}                              u64
 *   sum_le[j]             = sum over {i : X[i][j] <= threshold[j]} of X[i][j]          u64
 *   sumsq_le[2j, 2j + 1]  = the same sum of X[i][j]^2, as (low, high) words            128 bits
 * Counts are integers, so min(x, c) for a real clip value c >= 0 is x when x <= floor(c) and c otherwise: with
 * threshold = floor(c) the host forms  sum_i min(x, c) = sum_le + n_over * c  and  sum_i min(x, c)^2 = sumsq_le + n_over * c^2.
 */
int prosstt_amd_hvg_clipped_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                 const int32_t* threshold, void* ws, uint64_t ws_bytes,
                                 uint64_t* n_over, uint64_t* sum_le, uint64_t* sumsq_le, uint32_t* status);

/*
 * per gene: S1[j] = sum_i y, S2[j] = sum_i y^2 in binary64, with y = (float)X[i][j] * inv_size[i] the float32 product that
 * the log-normalised entry of prosstt_amd_embed.h starts from (y^2 is exact in binary64).  inv_size: N floats, within the
 * limits of prosstt_amd_embed.h; rows are added in ascending order within a block of rows, the blocks in ascending order
 * (the geometry and order of prosstt_amd_embed_gene_moments).
 */
int prosstt_amd_hvg_normalized_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                       const float* inv_size, void* ws, uint64_t ws_bytes,
                                       double* S1, double* S2, uint32_t* status);

/*
 * Y[r][c] = X[r][cols[c]] for r < N, c < n_sel (Y: row stride ldy >= n_sel).  cols: n_sel int32 on the device, in any
 * order, repeats allowed.  A column outside [0, G) sets status bit 1, writes 0 in its place and reads nothing; the other
 * columns of Y are still right.  Entries are copied as they are (a negative one too).
 */
int prosstt_amd_hvg_gather_columns(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                   const int32_t* cols, int64_t n_sel, int32_t* Y, int64_t ldy, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
