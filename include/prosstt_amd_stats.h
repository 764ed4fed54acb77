/*
 * prosstt_amd_stats.h -- summary statistics of a count matrix on the device (libprosstt_amd_stats.so).
 *
 * The reference matches a simulation to real data through five summaries of a count matrix X (cells x genes), computed
 * with numpy on the host in every compare_*.ipynb notebook:
 *     sim_means      = np.mean(X, axis=0)       per gene
 *     sim_vars       = np.var(X, axis=0)        per gene, ddof 0
 *     sim_zeros_gene = np.sum(X == 0, axis=0)
 *     sim_zeros_cell = np.sum(X == 0, axis=1)
 *     sim_totals     = np.sum(X, axis=1)        per cell: library size
 * and sim_utils.learn_data_summary (sim_utils.py:670-719) reads the same numbers as cell_stats.loc["total" | "zeros"] and
 * gene_stats.loc["means" | "var" | "zeros"].  The entry point below computes the exact integer sums behind all five in one
 * read of a matrix that is already on the device (the sampler's output); only O(N + G) numbers then cross PCIe.  The
 * means and variances are formed from these integers on the host (prosstt_amd/summary.py).
 *
 * Conventions (as in prosstt_amd.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_STATS_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_stats_last_error().
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (e.g. torch's current stream; NULL
 *    is the default stream of the current device); nothing synchronises, nothing allocates device memory: the caller
 *    passes a workspace of prosstt_amd_stats_workspace_bytes(N, G) bytes.
 *  - Results are exact integers, so they do not depend on launch geometry or arrival order.
 */
#ifndef PROSSTT_AMD_STATS_H
#define PROSSTT_AMD_STATS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_STATS_OK = 0,
    PROSSTT_AMD_STATS_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_STATS_EHIP = -3    /* HIP runtime error */
};

/* flags of prosstt_amd_stats_count_summary */
#define PROSSTT_AMD_STATS_ACCUMULATE 1u /* add the per-gene results to what gene_sum / gene_sumsq / gene_zeros hold (a matrix
                                           summarised in chunks of cells); the per-cell results are always written */

const char* prosstt_amd_stats_last_error(void);

/* Device workspace (bytes) that prosstt_amd_stats_count_summary needs for an N x G matrix.  A pure function of (N, G). */
int prosstt_amd_stats_workspace_bytes(int64_t N, int64_t G, uint64_t* bytes);

/*
 * Exact sums of an int32 count matrix X: row r, gene g at X[r*ld + g] (rows of stride ld >= G elements, unit column
 * stride; any base alignment -- rows that start on 16 bytes are read with 16-byte loads).  Replaces the five numpy lines
 * above and the inputs of learn_data_summary (sim_utils.py:670-719):
 *   gene_sum[g]          = sum_r X[r][g]                          u64       (np.mean(X, axis=0) * N)
 *   gene_sumsq[2g, 2g+1] = sum_r X[r][g]^2  as (low, high) words  128 bits  (np.var(X, axis=0): N*S2 - S1^2 over N^2)
 *   gene_zeros[g]        = #{r : X[r][g] == 0}                    u64       (np.sum(X == 0, axis=0))
 *   cell_total[r]        = sum_g X[r][g]                          u64       (np.sum(X, axis=1))
 *   cell_zeros[r]        = #{g : X[r][g] == 0}                    u64       (np.sum(X == 0, axis=1))
 * Every entry must be >= 0 (a count); a negative entry sets *status to 1 (the caller zeroes it; it is only ever set) and
 * leaves the sums meaningless.  The sum of squares is exact for every int32 input (x^2 < 2^62; a few rows overflow 64 bits).
 * Limits, refused with PROSSTT_AMD_STATS_EINVAL: 1 <= N < 2^31, 0 <= G, ld >= G, workspace_bytes at least the query's.
 */
int prosstt_amd_stats_count_summary(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                    void* workspace, uint64_t workspace_bytes,
                                    uint64_t* gene_sum, uint64_t* gene_sumsq, uint64_t* gene_zeros,
                                    uint64_t* cell_total, uint64_t* cell_zeros, uint32_t* status, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
