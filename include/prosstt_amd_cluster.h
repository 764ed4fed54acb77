/*
 * prosstt_amd_cluster.h -- Louvain (modularity) clustering of the connectivities of a kNN graph of cells, on the device
 * (libprosstt_amd_cluster.so).
 *
 * The step between prosstt_amd_graph.h (W, scanpy's obsp["connectivities"]) and prosstt_amd_markers.h (marker genes of
 * groups of cells): scanpy.tl.louvain.  The algorithm is written as a synchronous, reproducible one: equal calls give
 * equal labels on every run, every stream and every kernel path.  prosstt_amd/cluster.py drives the kernels below;
 * tests/cluster_model.py is the same definition in numpy.
 *
 * Definition
 *
 *   Input.  W symmetric, CSR as prosstt_amd_graph.h holds it: indptr int64 (N + 1), indices int32 ascending within a row,
 *   data binary64 with 0 <= w <= 1.  3 <= N < 2^31, nnz < 2^30.  gamma = the resolution, > 0 and finite.
 *
 *   Quantisation.  u_ij = (int64) floor(w_ij * 2^32 + 0.5): every weight is at most 2^32 and every sum below stays under
 *   2^62.  W is symmetric to the bit, so u is.  From here on every sum of weights is an int64 and exact: no order of
 *   summation shows.
 *
 *   Level graph.  n nodes, symmetric integer CSR; from the second level on with a diagonal entry u_ii, the weight inside
 *   the merged community, both directions counted.  k_i = sum_j u_ij (the diagonal included), M2 = sum_i k_i; M2 = 0 is
 *   refused by the caller.
 *
 *   State.  c_i, the community of node i, is a node index and starts as c_i = i.  tot[d] = sum_{c_i = d} k_i.
 *   in[d] = sum_{c_i = c_j = d} u_ij, the diagonal included.
 *
 *   Gain.  g(e, T) = (double)e - (gamma * ((double)k_i * (double)T)) / (double)M2; every operation rounded on its own (no
 *   fused multiply-add), the int64 -> binary64 conversions to nearest.
 *
 *   Sweep of parity p (synchronous: every node reads the c and tot from before the sweep, c_new is another array).  For
 *   node i and a community d, e_i(d) = sum_{j != i, c_j = d} u_ij.  stay = g(e_i(c_i), tot[c_i] - k_i), the subtraction
 *   in integers.  The candidates are the communities d != c_i of the stored entries j != i (entries of weight 0 count);
 *   for p = 0 only d < c_i, for p = 1 only d > c_i.  Node i moves to the candidate of largest g(e_i(d), tot[d]), the
 *   lowest d among equals, and only if that gain is strictly greater than stay.  (The one-direction rule keeps a
 *   synchronous sweep from swapping two nodes forever.)
 *
 *   Round.  A sweep of parity 0, the totals recomputed, a sweep of parity 1, the totals recomputed.  Then the quality
 *   Q = fsum_d ((double)in[d] / (double)M2 - gamma * (t * t)), t = (double)tot[d] / (double)M2, every operation rounded
 *   on its own and the sum exact (math.fsum, on the host).  A round is accepted if it moved at least one node and
 *   Q > Q_before + tol; otherwise the state from before the round is restored and the level ends.  A level also ends
 *   after max_rounds accepted rounds.
 *
 *   Aggregation.  The level's communities are renumbered 0 .. n' - 1 by ascending community id; U'_ab = sum_{c_i = a,
 *   c_j = b} u_ij, the diagonal included; columns ascend within a row.  If n' = n the call ends, otherwise the next level
 *   starts on U'; there are at most max_levels levels.  A node's final community is the composition of the levels.
 *
 *   Result labels.  Communities are numbered by size in cells, descending; equal sizes go to the community that holds the
 *   lowest cell index.  Label 0 is the largest cluster.
 *
 * Conventions (as in prosstt_amd_graph.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_CLUSTER_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_cluster_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory.
 *  - Values are checked on the device: a kernel that meets a bad one ORs a bit into *status (a device word the caller
 *    zeroes and reads back), leaves that value out and stays within bounds.  PROSSTT_AMD_CLUSTER_BAD_* name the bits.
 *  - Kernels use 256-thread blocks and 64-bit offsets.  Floating point appears in _quantize and in the gain only; every
 *    sum is an integer, every atomic an integer atomic, so the order in which lanes arrive never shows.
 *
 * A level graph is (indptr int64 (n + 1), indices int32 (nnz), u int64 (nnz), k int64 (n)), 1 <= n < 2^31,
 * 1 <= nnz < 2^31.  Communities c are int32 (n), tot and in are int64 (n).
 */
#ifndef PROSSTT_AMD_CLUSTER_H
#define PROSSTT_AMD_CLUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_CLUSTER_OK = 0,
    PROSSTT_AMD_CLUSTER_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_CLUSTER_EHIP = -3    /* HIP runtime error */
};

/* bits of *status */
enum {
    PROSSTT_AMD_CLUSTER_BAD_WEIGHT = 1,    /* _quantize: a weight that is NaN, negative or above 1 */
    PROSSTT_AMD_CLUSTER_BAD_GRAPH = 2,     /* a row outside [0, n), row bounds outside [0, nnz] or a column outside [0, n) */
    PROSSTT_AMD_CLUSTER_BAD_COMMUNITY = 4, /* a community outside [0, n) (of [0, n_new) in _aggregate_emit) */
    PROSSTT_AMD_CLUSTER_BAD_BINS = 8,      /* _sweep: a row longer than the path it was binned into can hold */
    PROSSTT_AMD_CLUSTER_BAD_SORT = 16      /* _aggregate_fold: a perm or pos entry outside its range */
};

/* The paths of _sweep and the longest row (stored entries) each can hold. */
enum {
    PROSSTT_AMD_CLUSTER_PATH_AUTO = 0,   /* every row on the first of the paths below that holds it */
    PROSSTT_AMD_CLUSTER_PATH_GROUP16 = 1, /* 16 lanes per row, entries in registers, shuffles, no LDS: rows <= 16 */
    PROSSTT_AMD_CLUSTER_PATH_WAVE = 2,   /* a wave per row, entries in registers, no LDS: rows <= 64 */
    PROSSTT_AMD_CLUSTER_PATH_TABLE = 3,  /* a block per row, an open-addressing table in LDS: rows <= 512 */
    PROSSTT_AMD_CLUSTER_PATH_RANGE = 4   /* a block per row, passes over ranges of 2048 community ids: every row */
};
#define PROSSTT_AMD_CLUSTER_GROUP16_ROW 16
#define PROSSTT_AMD_CLUSTER_WAVE_ROW 64
#define PROSSTT_AMD_CLUSTER_TABLE_ROW 512

const char* prosstt_amd_cluster_last_error(void);

/* Device workspace (bytes) of the aggregation of a level graph of these sizes: its nnz int64 keys.  Pure. */
int prosstt_amd_cluster_workspace_bytes(int64_t n, int64_t nnz, uint64_t* bytes);

/* u (nnz) and k (N) of the definition from W's values; a bad weight sets BAD_WEIGHT and counts as 0. */
int prosstt_amd_cluster_quantize(void* stream, const int64_t* indptr, const int32_t* indices, const double* W, int64_t N,
                                 int64_t nnz, int64_t* u, int64_t* k, uint32_t* status);

/* One sweep of parity 0 or 1: c_new (n) from c and tot; *moved (a device counter the caller zeroes) grows by the number
 * of nodes with c_new != c.  c_new must not alias c.
 * rows (n): the nodes ordered by ascending row length (any order among equals); n16, n64, n512: how many of them have at
 * most 16, 64, 512 stored entries.  With path 0 rows[0 .. n16) take GROUP16, rows[n16 .. n64) WAVE, rows[n64 .. n512)
 * TABLE and the rest RANGE, each in a launch of its own, an empty part in none.  Any other path takes every row and is
 * refused (EINVAL) unless the counts say it holds them all.  A row longer than its path holds (counts that are not those
 * of rows) is cut to what the path holds and sets BAD_BINS.  Every path gives the same c_new. */
int prosstt_amd_cluster_sweep(void* stream, const int64_t* indptr, const int32_t* indices, const int64_t* u,
                              const int64_t* k, int64_t n, int64_t nnz, const int32_t* rows, int64_t n16, int64_t n64,
                              int64_t n512, const int32_t* c, const int64_t* tot, int64_t M2, double gamma, int32_t parity,
                              int32_t path, int32_t* c_new, uint32_t* moved, uint32_t* status);

/* tot (n) and in (n) of the definition for the communities c: zeroed, then accumulated with 64-bit integer atomics. */
int prosstt_amd_cluster_totals(void* stream, const int64_t* indptr, const int32_t* indices, const int64_t* u,
                               const int64_t* k, int64_t n, int64_t nnz, const int32_t* c, int64_t* tot, int64_t* in,
                               uint32_t* status);

/* The aggregation has a sort in the middle, which is the caller's (as in prosstt_amd_graph.h):
 *   1. _aggregate_emit writes key[e] = c'_i << 32 | c'_j for every stored entry e = (i, j) into the workspace; cnew (n)
 *      holds the renumbered community c'_i in [0, n_new) of every node.  The values are u itself.
 *   2. the caller sorts the keys ascending and keeps the permutation: sorted[p] = key[perm[p]]; and computes pos[p] = the
 *      number of p' <= p with p' = 0 or sorted[p'] != sorted[p' - 1], nnz_new = pos[nnz - 1].
 *   3. _aggregate_fold zeroes u_new and adds u[perm[p]] into u_new[pos[p] - 1] (a thread sums what eight consecutive p
 *      share before its integer atomic); the head of each run writes indices_new, the first head of each row indptr_new. */
int prosstt_amd_cluster_aggregate_emit(void* stream, const int64_t* indptr, const int32_t* indices, int64_t n, int64_t nnz,
                                       const int32_t* cnew, int64_t n_new, void* ws, uint64_t ws_bytes, uint32_t* status);

int prosstt_amd_cluster_aggregate_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm, const int64_t* pos,
                                       const int64_t* u, int64_t nnz, int64_t n_new, int64_t nnz_new,
                                       int64_t* indptr_new /* n_new + 1 */, int32_t* indices_new /* nnz_new */,
                                       int64_t* u_new /* nnz_new */, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
