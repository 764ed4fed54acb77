/*
 * prosstt_amd_knn.h -- exact k-nearest-neighbour search of cells on the device (libprosstt_amd_knn.so).
 *
 * Every example notebook of the reference goes from the (reduced) expression matrix to pp.neighbors and from there to
 * diffusion maps or UMAP.  This library is that neighbour search for an N x d panel of coordinates (the PCA scores of
 * prosstt_amd/embed.py, d <= 128), exact and defined to the bit.
 *
 * Definition.  P is an N x d panel of binary32 coordinates.  For the pair (i, j)
 *
 *     d2(i, j) = acc_d,   acc_0 = 0,   acc_{c+1} = fl32(acc_c + fl32(t_c * t_c)),   t_c = fl32(P[i][c] - P[j][c]),
 *                c = 0 .. d-1
 *
 * a separate binary32 subtract, multiply and add per coordinate in ascending c; nothing is fused and subnormals are kept.
 * Hence d2(i, j) and d2(j, i) are the same bits.  The neighbours of cell i are the k cells j != i with the smallest key
 * (bits(d2(i, j)), j), listed in ascending key; bits is the value's 32-bit pattern read as unsigned (numeric order for
 * the non-negative finite values in play), so ties go to the lower index.  All keys of a row are distinct: the result
 * is unique and does not depend on the grid, the chunking or the stream.  The Gram form |a|^2 + |b|^2 - 2 a.b is NOT
 * the definition (it cancels for exactly the pairs that matter).
 *
 * Conventions (as in prosstt_amd_embed.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_KNN_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_knn_last_error().  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    prosstt_amd_knn_workspace_bytes(N, d, k, chunk_rows) bytes, 16-byte aligned.
 *  - P: cell i, coordinate c at P[i*ld + c] (unit column stride, row stride ld >= d; any base alignment: rows that do
 *    not all start on 16 bytes are read with 4-byte loads).  Coordinates should be finite and below 2^59 in magnitude
 *    (then no d2 overflows); for ANY bit pattern the kernels stay within bounds and order the row by the key above.
 *  - The search runs over chunks of chunk_rows query cells: their distances to all N cells go to a slab in the workspace,
 *    then each row of the slab is selected.  chunk_rows = 0 is the library's choice, a pure function of N: the slab is
 *    kept near 192 MiB so that the selection's re-reads of a row stay in the 256 MiB last-level cache.  The result does
 *    not depend on chunk_rows.
 *  - Limits, refused with PROSSTT_AMD_KNN_EINVAL: 2 <= N < 2^31, 1 <= d <= 128, ld >= d, 1 <= k <= min(N - 1, 1024),
 *    0 <= chunk_rows <= N, a slab of at most 2^40 distances, a workspace at least the query's.
 */
#ifndef PROSSTT_AMD_KNN_H
#define PROSSTT_AMD_KNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_KNN_OK = 0,
    PROSSTT_AMD_KNN_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_KNN_EHIP = -3    /* HIP runtime error */
};

const char* prosstt_amd_knn_last_error(void);

/* Device workspace (bytes) that prosstt_amd_knn_search needs for these sizes.  Pure. */
int prosstt_amd_knn_workspace_bytes(int64_t N, int64_t d, int64_t k, int64_t chunk_rows, uint64_t* bytes);

/* index[i*k + r], sqdist[i*k + r]: the r-th neighbour of cell i and its d2, r = 0 .. k-1 in ascending key. */
int prosstt_amd_knn_search(void* stream, const float* P, int64_t N, int64_t d, int64_t ld, int64_t k,
                           int64_t chunk_rows, int32_t* index /* N x k */, float* sqdist /* N x k */,
                           void* ws, uint64_t ws_bytes);

#ifdef __cplusplus
}
#endif
#endif
