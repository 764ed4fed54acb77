// The device half of a column kernel (abi_util.h holds the host half: kColumn, kColumnTile, row_blocking, aligned and the
// two refusals of a column library's sizes).
// Internal: included after abi_util.h by fit/fit.hip and regress/regress.hip, and by factors/factors.hip for kBig and
// column_admissible alone (its lane owns a cell, not a gene); not installed under include/.
//
// A column kernel reads the int32 count matrix for sums that need many registers per gene.  A block of kThreads lanes owns
// the kColumn = 256 genes from `gbase` on and the rows [r0, r0 + n_rows) of its row block (row_blocking); a lane owns ONE
// gene, g = gbase + tid, whose parameters and sums stay in its registers across the rows.  VEC (every row can be read in
// 16-byte pieces: aligned(X, ld, 4)) and a whole strip of 256 genes: a tile of kColumnTile = 8 rows goes through LDS -- wave
// w loads rows w and w + 4 of the tile, a lane 16 bytes (four genes) of each -- and every lane then reads its own gene's
// column of the tile.  Otherwise (any alignment, and the last, partial strip under either) the lane loads its gene's entry
// of the row itself, 4 bytes, coalesced; a gene at or past G reads nothing and counts as 0.  Per-block sums go to slabs
// [row_blocks][...][G], which a finish kernel adds from row block 0 upward: the order is part of the result.  No atomic but
// the OR of a status bit.
//
// Every function here is inlined.  DESIGN.md, section 33, compares each kernel's machine code with the same kernel written
// out, by section 24's method: ten of the twelve kernels of fit and regress are identical, regress's two Q kernels
// (ACC = 0) differ outside their loops.  That holds for the calls where they stand and for the order of column_reader's
// lines: the kernels' text follows the order in which the values are formed, so regress_pass_kernel forms its lane view
// below the bookkeeping of its sums, and both kernels form labels + r0 and size + r0 before the reader.  Where sharing
// changed a loop the code stays written out:
//   regress_pass_kernel keeps its staging loop, the body of column_stage (as a call it changed the four aligned pass
//   kernels by 32 to 149 lines each, most of them in the row loops, at equal register counts; fit_loglik_kernel, with the
//   same call, did not change);
//   fit_finish_kernel and regress_finish_kernel keep the fold of their binary64 slab (as a function, returning the sum or
//   adding to a reference, with or without __restrict__, the loop's closing compare and branch changed their sense), and
//   the folds of the uint32 slabs beside it (fit's bad in one loop with base, regress's used);
//   each kernel keeps its `asm volatile("" : "+v"(...))` pin of the epilogue's pointers, whose operands differ;
//   fit keeps its scalar label and size loads, regress its per-tile LDS tables, both their <VEC> launch pairs.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr double kBig = 1.7976931348623157e308;         // the largest finite binary64

// Finite with a >= 0 and b >= 1 (false for a NaN): what every column library asks of a gene's (alpha, beta).
__device__ __forceinline__ bool column_admissible(double a, double b) { return a >= 0.0 && a <= kBig && b >= 1.0 && b <= kBig; }

// The lane's view of its block: which gene and which rows.
struct ColumnLane {
    int tid;
    int64_t gbase, g;               // the block's first gene and the lane's own
    bool mine;                      // g < G
    bool staged;                    // the block's rows go through the LDS tile (block-uniform)
    int64_t r0, r1;                 // the block's rows
};

template <bool VEC>
__device__ __forceinline__ ColumnLane column_lane(int64_t N, int64_t G, int64_t rows_per_block)
{
    ColumnLane l;
    l.tid = threadIdx.x;
    l.gbase = (int64_t)blockIdx.x * kColumn;
    l.g = l.gbase + l.tid;
    l.mine = l.g < G;
    l.r0 = (int64_t)blockIdx.y * rows_per_block;
    l.r1 = (l.r0 + rows_per_block < N) ? l.r0 + rows_per_block : N;
    l.staged = VEC && l.gbase + kColumn <= G;       // (the last, partial strip reads as the unaligned kernel does)
    return l;
}

// How the lane reads the block's rows, counted from r0 in 32 bits.
struct ColumnReader : ColumnLane {
    int n_rows;
    int lrow, lcol;                 // the lane's part of a tile's loads: row (wave + 4 i), genes 4 * (lane of the wave) .. + 3
    const int32_t* __restrict__ xcol;       // the lane's own column (read when not staged)
    const int32_t* __restrict__ xtile;      // the lane's 16 bytes of a staged row
};

__device__ __forceinline__ ColumnReader column_reader(const ColumnLane& l, const int32_t* __restrict__ X, int64_t ld)
{
    ColumnReader r;
    static_cast<ColumnLane&>(r) = l;
    r.n_rows = (int)(l.r1 - l.r0);
    r.lcol = 4 * (l.tid & 63);                      // (lcol first: the other way two registers of fit's row loop change places)
    r.lrow = l.tid >> 6;
    r.xcol = X + l.r0 * ld + (l.mine ? l.g : 0);
    r.xtile = X + l.r0 * ld + l.gbase + r.lcol;
    return r;
}

// The lane's loads of the tile of `rows` rows from row rt on (of a staged block; between two barriers).
template <int R>
__device__ __forceinline__ void column_stage(int32_t (&tile)[R][kColumn], const ColumnReader& r, int64_t ld, int rt, int rows)
{
#pragma unroll
    for (int i = 0; i < kColumnTile / 4; ++i) {
        const int tr = r.lrow + 4 * i;
        if (tr < rows)
            *reinterpret_cast<int4*>(&tile[tr][r.lcol]) = *reinterpret_cast<const int4*>(r.xtile + (int64_t)(rt + tr) * ld);
    }
}

// The lane's entry of row rt + tr.
template <int R>
__device__ __forceinline__ int32_t column_entry(const int32_t (&tile)[R][kColumn], const ColumnReader& r, int64_t ld, int rt, int tr)
{
    return r.staged ? tile[tr][r.tid] : (r.mine ? r.xcol[(int64_t)(rt + tr) * ld] : 0);
}
