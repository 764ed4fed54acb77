/*
 * prosstt_amd_graph.h -- fuzzy connectivities of a kNN graph of cells and the density-normalised diffusion operator on
 * it, on the device (libprosstt_amd_graph.so).
 *
 * The reference's example notebooks go from pp.neighbors to scanpy.tl.diffmap.  This library is the graph half of that
 * step for the output of prosstt_amd_knn.h: memberships, their symmetrisation into a CSR matrix W, the normalisation of W
 * into the symmetric transition matrix T, and y = T x, which a Lanczos solver (prosstt_amd/graph.py) calls once per step.
 *
 * Definitions (all binary64).  The input is N rows of k other cells each: index[i*k + r] and sqdist[i*k + r] (binary32),
 * d_ij = sqrt((double)sqdist).  3 <= N < 2^31, 2 <= k <= min(N - 1, 1024); every index lies in [0, N) and differs from
 * its row; every sqdist is finite and >= 0.
 *
 *   Memberships (directed, N x k).  For row i: rho_i = min{d_ij : d_ij > 0} (0 if there is none), g_ij = max(d_ij - rho_i,
 *   0), f(s) = sum_j exp(-g_ij / s), target = log2(k + 1).  sigma_i comes from exactly this bisection, 64 steps, no early
 *   exit:
 *       lo = 0; hi = inf; mid = 1
 *       repeat 64 times:
 *           if f(mid) > target:  hi = mid;  mid = (lo + hi) / 2
 *           else:                lo = mid;  mid = (hi == inf) ? 2 mid : (lo + hi) / 2
 *       sigma_i = max(mid, 1e-3 * mean_j d_ij)
 *   a_ij = 1 where g_ij = 0, exp(-g_ij / sigma_i) otherwise.  (umap-learn's smooth_knn_dist as scanpy calls it with
 *   local_connectivity 1 and n_neighbors = k + 1, the self column skipped; but the root is found to full precision, and
 *   the floor uses the row's own mean also when rho = 0.)
 *
 *   Connectivities.  W = A + A^T - A o A^T, A the N x N matrix of the a_ij, computed as (a + b) - a b: symmetric in a and
 *   b, so W is symmetric to the bit.  CSR: indptr int64 (N + 1), indices int32 ascending within a row, data binary64;
 *   every stored pair once per direction, no diagonal, no explicit zeros beyond what a itself yields (an exp that
 *   underflows).  Rows have between k and N - 1 entries.
 *
 *   Operator.  q = W 1, K_ij = W_ij / (q_i q_j), z_i = sqrt((K 1)_i), T_ij = K_ij / (z_i z_j): symmetric to the bit, the
 *   sparsity of W.  On a connected graph T z = z.
 *
 * Conventions (as in prosstt_amd_knn.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_GRAPH_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_graph_last_error().  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers, rows contiguous.  All work is enqueued on the caller's stream (NULL: the default
 *    stream of the current device); nothing synchronises, nothing allocates device memory.
 *  - Values are checked on the device: a kernel that meets a bad one ORs a bit into *status (a device word the caller
 *    zeroes and reads back) and stays within bounds.  PROSSTT_AMD_GRAPH_BAD_* name the bits.  A caller that finds a bit
 *    set must not pass the arrays on: _normalize and _spmv trust indptr and indices (0 = indptr[0] <= indptr[1] <= .. <=
 *    indptr[N] = nnz, 0 <= indices < N).
 *  - Kernels use 256-thread blocks and 64-bit offsets and no floating-point atomic: every sum has a fixed order, so equal
 *    inputs give equal bits on every run and every stream.
 *
 * The symmetrisation has a sort in the middle, which is the caller's (any sort of int64 keys will do; prosstt_amd/graph.py
 * uses torch.sort on the same stream):
 *    1. _symmetrize_emit writes M = 2 N k keyed entries into the workspace: keys (int64) at offset 0, key[2e] =
 *       i << 32 | j and key[2e + 1] = j << 32 | i for entry e = i k + r with j = index[e]; values (binary64) at offset
 *       prosstt_amd_graph_workspace_bytes / 2, value[2e] = value[2e + 1] = a[e].
 *    2. the caller sorts the keys ascending and keeps the permutation: sorted[p] = key[perm[p]]; and computes pos[p] = the
 *       number of p' <= p with p' = 0 or sorted[p'] != sorted[p' - 1] (an inclusive prefix sum of the run heads), nnz =
 *       pos[M - 1].
 *    3. _symmetrize_fold walks the sorted run: the head of each run of equal keys folds the run's values (two at most
 *       when the indices of a row are distinct) with w <- (w + b) - w b and writes entry pos - 1 of indices and data;
 *       the first head of each row writes indptr.
 */
#ifndef PROSSTT_AMD_GRAPH_H
#define PROSSTT_AMD_GRAPH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_GRAPH_OK = 0,
    PROSSTT_AMD_GRAPH_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_GRAPH_EHIP = -3    /* HIP runtime error */
};

/* bits of *status */
enum {
    PROSSTT_AMD_GRAPH_BAD_INDEX = 1,    /* _memberships: an index outside [0, N) */
    PROSSTT_AMD_GRAPH_BAD_SELF = 2,     /* _memberships: an index equal to its row */
    PROSSTT_AMD_GRAPH_BAD_DISTANCE = 4, /* _memberships: a squared distance that is negative, infinite or NaN */
    PROSSTT_AMD_GRAPH_BAD_DEGREE = 8    /* _normalize: a row of W or K whose sum is not a positive finite number */
};

const char* prosstt_amd_graph_last_error(void);

/* Device workspace (bytes) of the symmetrisation for these sizes: keys in the first half, values in the second.  Pure. */
int prosstt_amd_graph_workspace_bytes(int64_t N, int64_t k, uint64_t* bytes);

/* a[i*k + r], rho[i], sigma[i] of the definition; the value checks of index and sqdist go to *status. */
int prosstt_amd_graph_memberships(void* stream, const int32_t* index /* N x k */, const float* sqdist /* N x k */,
                                  int64_t N, int64_t k, double* a /* N x k */, double* rho /* N */,
                                  double* sigma /* N */, uint32_t* status);

/* Step 1 above.  ws: prosstt_amd_graph_workspace_bytes(N, k) bytes, 16-byte aligned. */
int prosstt_amd_graph_symmetrize_emit(void* stream, const int32_t* index, const double* a, int64_t N, int64_t k,
                                      void* ws, uint64_t ws_bytes);

/* Step 3 above.  sorted_keys, perm, pos: M = 2 N k int64 each; ws still holds the values of step 1; nnz = pos[M - 1]. */
int prosstt_amd_graph_symmetrize_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm, const int64_t* pos,
                                      int64_t N, int64_t k, int64_t nnz, const void* ws, uint64_t ws_bytes,
                                      int64_t* indptr /* N + 1 */, int32_t* indices /* nnz */, double* data /* nnz */);

/* T (nnz values, the sparsity of W), q and z (N each) of the definition from W's values.  T must not alias W. */
int prosstt_amd_graph_normalize(void* stream, const int64_t* indptr, const int32_t* indices, const double* W, int64_t N,
                                int64_t nnz, double* T, double* q, double* z, uint32_t* status);

/* y = T x.  A group of lanes_per_row lanes (4, 16 or 64; 0: the library chooses from nnz / N) owns a row and adds its
 * products with a fixed shuffle tree: equal inputs give equal bits for a given lanes_per_row.  y must not alias x. */
int prosstt_amd_graph_spmv(void* stream, const int64_t* indptr, const int32_t* indices, const double* T, int64_t N,
                           int64_t nnz, const double* x, double* y, int32_t lanes_per_row);

#ifdef __cplusplus
}
#endif
#endif
