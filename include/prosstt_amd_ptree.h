/*
 * prosstt_amd_ptree.h -- the device passes of a regularised principal tree in a reduced space (libprosstt_amd_ptree.so).
 *
 * The reference's examples/reproduce_axolotl.ipynb reads the topology, the branch lengths and the cells' nodes from an
 * elastic principal tree fitted outside Python.  prosstt_amd/ptree.py fits such a tree by SimplePPT's alternation of a soft
 * assignment, a minimum spanning tree and a linear solve; its hard limit is Lloyd's k-means.  The spanning tree and the
 * solve are host numpy in binary64 (R nodes, R <= 4096); the two passes over the cells are this library.
 *
 * Definition.  Y is an N x d panel of binary32 coordinates, C an R x d panel of binary32 centres.
 *
 *     d2(i, k) = acc_d,  acc_0 = 0,  acc_{c+1} = fl32(acc_c + fl32(t_c * t_c)),  t_c = fl32(Y[i][c] - C[k][c]),  c = 0 .. d-1
 *
 * exactly prosstt_amd_knn.h's distance: a separate binary32 subtract, multiply and add per coordinate in ascending c;
 * nothing is fused and subnormals are kept.
 *
 * The assign pass.  best_i is the node with the smallest key (bits(d2(i, k)), k), bits the 32-bit pattern read as unsigned:
 * ties go to the lower index.  m_i = d2(i, best_i).  From here everything is binary64 and every operation is rounded on its
 * own (fl is binary64 rounding to nearest):
 *   sigma > 0 (soft)
 *     w_ik = exp(-fl(fl((double)d2_ik - (double)m_i) / sigma))
 *     Z_i  = the sum of the w_ik in THIS order: for l = 0 .. 63, p_l = the sum from 0.0 of w_ik over k = l, l + 64, l + 128,
 *            ... < R in ascending k (p_l = 0.0 when l >= R); then six butterfly stages off = 32, 16, 8, 4, 2, 1, each
 *            replacing every p_l by fl(p_l + p_(l xor off)); Z_i is p_0 (all 64 are equal).  Z_i >= 1 always.
 *     r_ik = fl(w_ik / Z_i)
 *     F_i  = fl((double)m_i - fl(sigma * log(Z_i)))
 *   sigma = 0 (hard, the k-means step)
 *     r_ik = 1.0 if k = best_i, else 0.0;  F_i = (double)m_i
 *   per node
 *     Gamma_k = sum_i r_ik,   S_kc = sum_i fl(r_ik * (double)Y[i][c])
 *     in THIS order over the cells: the cells are cut into consecutive chunks of PROSSTT_AMD_PTREE_CHUNK = 128 cells from
 *     cell 0; within a chunk the terms are added one by one from 0.0 in ascending i; the chunk sums are added one by one from
 *     0.0 in ascending chunk.  (The product is rounded before it is added: no fused multiply-add.)
 * exp and log are the device library's binary64 functions (1 ulp); everything else is IEEE.  There is no
 * floating-point atomic, and the ABI has no launch-geometry option: equal inputs give equal bits on any stream.  best,
 * d2min, free_energy and the resp row of a cell depend on that cell's row of Y and on C alone: they are the same bits
 * whether the cell is passed alone or among others.
 *
 * The project pass.  For E edges (a_e, b_e), int32 pairs of node indices, per cell and edge in binary64 from the binary32
 * inputs, ascending c, every operation rounded on its own, with y = (double)Y[i][c], a = (double)C[a_e][c], b = (double)C[b_e][c]:
 *     u = sum_c fl(fl(y - a) * fl(b - a)),   l = sum_c fl(fl(b - a) * fl(b - a))       (both from 0.0)
 *     t = fl(u / l), then 0 if t < 0, 1 if t > 1; t = 0 when l = 0
 *     q = sum_c fl(e_c * e_c),  e_c = fl(fl(y - a) - fl(t * fl(b - a)))                 (from 0.0)
 * The cell's edge is the one with the smallest key (bits(q), e), bits the 64-bit pattern read as unsigned: ties go to the
 * lower edge.  Every step is IEEE (the division is correctly rounded).
 *
 * Conventions (as in prosstt_amd_knn.h)
 *  - extern "C", plain pointers and sizes; never throws.  Return 0 on success, a negative PROSSTT_AMD_PTREE_E* code
 *    otherwise; the message is in the thread-local prosstt_amd_ptree_last_error.  Bad sizes are refused before anything
 *    is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates: the caller passes a workspace of
 *    prosstt_amd_ptree_workspace_bytes bytes for (N, d, R, soft), 16-byte aligned (the N x R distances, for soft != 0 the
 *    N x R responsibilities, and the chunk sums).
 *  - Y: cell i, coordinate c at Y[i*ld + c] (unit column stride, row stride ld >= d, any base alignment of 4 bytes); C
 *    likewise with ldc.  Outputs are dense: gamma (R), sums (R x d, row stride d), resp (N x R, row stride R) or NULL.
 *  - status: one uint32 the caller zeroes; the passes OR bits into it (PROSSTT_AMD_PTREE_NONFINITE: a coordinate or a
 *    centre is not finite; PROSSTT_AMD_PTREE_EDGE_RANGE: an edge names a node outside 0 .. R-1, it is skipped).  With a bit
 *    set the other outputs are within bounds but mean nothing.
 *  - Limits, refused with PROSSTT_AMD_PTREE_EINVAL: 1 <= N < 2^31, 1 <= d <= 128, 1 <= R <= 4096, ld >= d, ldc >= d,
 *    sigma >= 0 and finite, 1 <= E <= 8192.
 */
#ifndef PROSSTT_AMD_PTREE_H
#define PROSSTT_AMD_PTREE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_PTREE_OK = 0,
    PROSSTT_AMD_PTREE_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_PTREE_EHIP = -3    /* HIP runtime error */
};

enum {
    PROSSTT_AMD_PTREE_NONFINITE = 1,
    PROSSTT_AMD_PTREE_EDGE_RANGE = 2
};

#define PROSSTT_AMD_PTREE_CHUNK 128
#define PROSSTT_AMD_PTREE_MAX_DIM 128
#define PROSSTT_AMD_PTREE_MAX_NODES 4096
#define PROSSTT_AMD_PTREE_MAX_EDGES 8192

const char* prosstt_amd_ptree_last_error(void);

/* Device workspace (bytes) of the assign pass for these sizes; soft != 0 for sigma > 0.  Pure. */
int prosstt_amd_ptree_workspace_bytes(int64_t N, int64_t d, int64_t R, int32_t soft, uint64_t* bytes);

/* The assign pass: best (N), d2min (N), free_energy (N), gamma (R), sums (R x d), resp (N x R) or NULL. */
int prosstt_amd_ptree_assign(void* stream, const float* Y, int64_t N, int64_t d, int64_t ld, const float* C, int64_t R,
                             int64_t ldc, double sigma, void* ws, uint64_t ws_bytes, int32_t* best, float* d2min,
                             double* free_energy, double* gamma, double* sums, double* resp, uint32_t* status);

/* The project pass: edges (E x 2 int32); edge (N), t (N), q (N). */
int prosstt_amd_ptree_project(void* stream, const float* Y, int64_t N, int64_t d, int64_t ld, const float* C, int64_t R,
                              int64_t ldc, const int32_t* edges, int64_t E, int32_t* edge, double* t, double* q,
                              uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
