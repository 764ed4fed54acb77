/*
 * prosstt_amd_autocorr.h -- sums over the edges of a cell graph of the log-normalised count matrix on the device
 * (libprosstt_amd_autocorr.so): what Moran's I and Geary's C of every gene (scanpy's metrics.morans_i and metrics.gearys_c on
 * obsp["connectivities"]) are computed from, and the graph-smoothed expression W.A.  prosstt_amd/autocorr.py drives it and
 * holds the statistics.
 *
 * Definition.
 *
 *   Input.  X: N rows x G genes, int32, and inv_size: N floats PER MATRIX ROW, both exactly as in prosstt_amd_embed.h (row
 *   r, gene g at X[r*ld + g], ld >= G, any base alignment; inv_size[r] = fl32(1 / s) in [2^-126, 2^94]).  cell_of_row: N
 *   int32, the cell (the graph's node) that matrix row r holds, a permutation of 0 .. N - 1, or NULL: row r is cell r.  The
 *   matrix is read in place.  W: a CSR matrix of cells x cells (indptr N + 1 int64 ascending from 0 to nnz, indexed by CELL;
 *   data nnz binary64; indices nnz int32 in [0, N), each the MATRIX ROW of the neighbour: with a cell_of_row the caller
 *   relabels the columns once, row_of_cell[j] for j, so that the kernels reach a neighbour's counts in one hop), which need
 *   not be symmetric, may hold a diagonal, stored zeros and empty rows.  mean: G binary64, the mu of every gene.
 *
 *   a[i][g] = (double) of the float32 entry log1p(X[r][g] * inv_size[r]), r the row of cell i, of prosstt_amd_embed.h, bit
 *   for bit that library's (one definition in the source, csrc/log1p_entry.h);  z[i][g] = a[i][g] - mean[g].
 *
 *   Per cell i, over the entries e = indptr[i] .. indptr[i + 1] - 1 of its row IN THAT ORDER, j the cell in row indices[e],
 *   w = data[e], both from 0, every operation rounded on its own (no fma):
 *       m = m + w * z[j]                      (the lag of z)
 *       d = a[i] - a[j];  q = q + w * (d * d)
 *
 *   _gene_sums, each [G]:
 *       cross  = sum_i z[i] * m[i]            sqdiff = sum_i q[i]
 *       m2     = sum_i z[i] * z[i]            m4     = sum_i (z[i] * z[i]) * (z[i] * z[i])
 *   Order of the sums over cells (part of the definition).  The cells are taken in the order of their MATRIX ROWS (a
 *   presented matrix keeps cells of one branch together, so a block's neighbours lie in nearby rows): the rows 0 .. N - 1 are
 *   cut into ceil(N / rows_per_block) blocks of rows_per_block consecutive rows (the last one shorter).  Within a block, row
 *   after row from 0: s = s + term of the row's cell.  Then the blocks are added in ascending order, from 0.  The order
 *   depends on N, rows_per_block and the matrix's row order alone: not on G, the gene's position, the view's alignment,
 *   gene_tile or the stream.
 *
 *   _smooth, [N][G] float32, row i (a CELL: plan order) at out[i*ldo + g]:
 *       out[i][g] = (float)(m[i][g] * scale_i)    with mean = 0, so m = sum_e w * a[j] as above
 *   scale_i = 1 when normalize == 0; otherwise d_i = sum_e w_e over the row's entries in order from 0, scale_i = 1 / d_i
 *   (binary64), and a cell with d_i == 0 (no entries among them) gives zeros.  One binary64 product, one rounding to float32.
 *
 * Kernels (256 threads, 64-bit offsets, no scratch, no LDS, no floating-point atomic).
 *   autocorr_sums_kernel    a WAVE owns one block of rows and a tile of genes; its lanes run across the tile (gene_tile 256:
 *                           four genes per lane, one 16-byte load per lane and row when rows are 16-byte aligned; gene_tile 64:
 *                           one gene per lane).  The four waves of a workgroup take four adjacent tiles of the same rows, and
 *                           workgroups are ordered rows-fastest, so resident workgroups gather from one column slab.  The
 *                           neighbour's index, weight, row and inv_size are wave-uniform loads; four neighbours' segments
 *                           are in flight together and are consumed in order.  Partials go to slabs [4][blocks][G].
 *   autocorr_finish_kernel  one thread per gene adds the blocks in ascending order.
 *   autocorr_smooth_kernel  the same loop with mean = 0 over 8 rows per wave, and a store to the cell's row of out.
 *
 * Conventions (as in prosstt_amd_embed.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_AUTOCORR_E* code otherwise; the message is in the thread-local
 *    prosstt_amd_autocorr_last_error.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory: the caller passes a workspace of
 *    _workspace_bytes(N, G, rows_per_block) bytes, 16-byte aligned (_smooth needs none).
 *  - Deterministic: equal inputs give bit-identical outputs on any stream.
 *  - The CSR arrays are the caller's to check: the kernels trust indptr to ascend from 0 to nnz.  As a guard an entry outside
 *    [0, nnz) and an index or a cell_of_row outside [0, N) are not read through; they set a bit instead.
 *  - *status (the caller zeroes it; bits are only ever set) and, when it is not zero, meaningless outputs:
 *      PROSSTT_AMD_AUTOCORR_NEGATIVE     a negative count (every row is read once as its own cell's row: flagged there)
 *      PROSSTT_AMD_AUTOCORR_INDEX_RANGE  the guard above
 *  - Limits, refused with PROSSTT_AMD_AUTOCORR_EINVAL: 1 <= N < 2^31, 1 <= G <= 65535 * 4 * gene_tile, ld >= G, ldo >= G,
 *    nnz >= 0, rows_per_block >= 0, gene_tile in {0, 64, 256}, NULL or misaligned pointers (int64 and binary64 arrays on 8
 *    bytes, the workspace on 16), a workspace below the query's.
 */
#ifndef PROSSTT_AMD_AUTOCORR_H
#define PROSSTT_AMD_AUTOCORR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_AUTOCORR_OK = 0,
    PROSSTT_AMD_AUTOCORR_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_AUTOCORR_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_AUTOCORR_NEGATIVE 1u
#define PROSSTT_AMD_AUTOCORR_INDEX_RANGE 2u

const char* prosstt_amd_autocorr_last_error(void);

/* Device workspace (bytes) of _gene_sums for these sizes.  rows_per_block as there.  Pure. */
int prosstt_amd_autocorr_workspace_bytes(int64_t N, int64_t G, int64_t rows_per_block, uint64_t* bytes);

/* The four sums of the definition.  rows_per_block: 0 for the library's rule max(16, ceil(N / 512)) (a function of N alone),
 * or any positive value.  gene_tile: 64 or 256 genes per wave, 0 for the library's rule (256 when rows are 16-byte aligned
 * and that leaves at least 4096 waves, else 64); the results do not depend on it. */
int prosstt_amd_autocorr_gene_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const float* inv_size,
                                   const int32_t* cell_of_row /* or NULL */, const int64_t* indptr, const int32_t* indices,
                                   const double* data, int64_t nnz, const double* mean /* G */, int64_t rows_per_block,
                                   int32_t gene_tile, void* ws, uint64_t ws_bytes, double* cross, double* sqdiff, double* m2,
                                   double* m4, uint32_t* status);

/* The smoothed panel of the definition. */
int prosstt_amd_autocorr_smooth(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const float* inv_size,
                                const int32_t* cell_of_row /* or NULL */, const int64_t* indptr, const int32_t* indices,
                                const double* data, int64_t nnz, int32_t normalize, int32_t gene_tile, float* out, int64_t ldo,
                                uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
