/*
 * prosstt_amd_embed.h -- products with the log-normalised count matrix on the device (libprosstt_amd_embed.so).
 *
 * Every example notebook of the reference embeds the sampled cells the same way: divide each cell by its size factor,
 * take log1p, then neighbours / diffusion maps / UMAP on the leading principal components.  This library provides the
 * passes over the int32 count matrix that a randomized PCA of
 *
 *     A[i][j] = log1p(X[i][j] / s[i])                 (natural log; X: N cells x G genes; s: size factors)
 *
 * needs (prosstt_amd/embed.py drives them): the per-gene moments of A and the products A.W and A^T.Q with thin f32
 * panels.  A is never stored: each pass reads X once and forms A[i][j] in registers, in float32 with a relative error of
 * at most 2^-20 against binary64 (x / s through inv_size[i] = fl32(1 / s[i]), then log1p through v_log_f32 and the
 * identity log1p(y) = log(u) * y / (u - 1), u = fl(1 + y)).
 *
 * Conventions (as in prosstt_amd_stats.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_EMBED_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_embed_last_error().  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    prosstt_amd_embed_workspace_bytes(N, G, l) bytes (enough for each of the three entry points).
 *  - Deterministic: reductions go through partial slabs in the workspace that a finishing kernel sums in a fixed order
 *    (no floating-point atomics), so equal inputs give bit-identical outputs on any stream.
 *  - X: row r, gene g at X[r*ld + g] (unit column stride, row stride ld >= G; any base alignment).  Every entry must be
 *    >= 0; a negative entry sets *status to 1 (the caller zeroes it; it is only ever set) and leaves the outputs
 *    meaningless.
 *  - inv_size[i] = fl32(1 / s[i]) must lie in [2^-126, 2^94] (2^-94 <= s <= 2^126); the caller checks it (embed.py
 *    refuses other size factors), the library does not read it on the host.  Below 2^-126 it is a denormal; above
 *    2^94 the product x * inv_size of a large count overflows (a NaN entry) or exceeds 2^126, where v_rcp_f32 returns 0
 *    for a denormal reciprocal.  Inside the range every entry is 0 (x = 0) or a normal float32 within 2^-20.
 *  - Limits, refused with PROSSTT_AMD_EMBED_EINVAL: 1 <= N < 2^31, 1 <= G, ld >= G, 1 <= l <= 128, a workspace at least
 *    the query's.
 */
#ifndef PROSSTT_AMD_EMBED_H
#define PROSSTT_AMD_EMBED_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_EMBED_OK = 0,
    PROSSTT_AMD_EMBED_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_EMBED_EHIP = -3    /* HIP runtime error */
};

const char* prosstt_amd_embed_last_error(void);

/* Device workspace (bytes) that each entry point below needs for an N x G matrix and panels of width l.  Pure. */
int prosstt_amd_embed_workspace_bytes(int64_t N, int64_t G, int64_t l, uint64_t* bytes);

/* per gene: S1[j] = sum_i A[i][j], S2[j] = sum_i A[i][j]^2, binary64 accumulation.  inv_size: N floats. */
int prosstt_amd_embed_gene_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                   const float* inv_size, void* ws, uint64_t ws_bytes,
                                   double* S1, double* S2, uint32_t* status);

/* Y (N x l, row-major f32) = A . W,   W: G x l row-major f32 */
int prosstt_amd_embed_matmul(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                             const float* inv_size, const float* W, int64_t l, float* Y,
                             void* ws, uint64_t ws_bytes, uint32_t* status);

/* Z (G x l, row-major f32) = A^T . Q,  Q: N x l row-major f32 */
int prosstt_amd_embed_rmatmul(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                              const float* inv_size, const float* Q, int64_t l, float* Z,
                              void* ws, uint64_t ws_bytes, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
