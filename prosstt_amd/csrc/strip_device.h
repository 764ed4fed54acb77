// The device half of a strip kernel (abi_util.h holds the host half: kStrip, strip_geometry, aligned).
// Internal: included after abi_util.h by stats/count_summary.hip, embed/embed.hip, hvg/hvg.hip, markers/markers.hip,
// ranks/ranks.hip, trends/trends.hip and thin/thin.hip (which writes a matrix and keeps its store_row4), not installed under
// include/.
//
// A block of kThreads lanes owns the kStrip genes from `gbase` on, and a lane owns four of them.  VEC (every row can be read
// in 16-byte pieces: aligned(X, ld, 4)): the four are contiguous from g0 = gbase + 4 tid, so that a row of a whole strip is
// one 16-byte load per lane.  Otherwise they are 256 apart from g0 = gbase + tid, so that each of four 4-byte loads
// coalesces.  Per-block sums go to slabs [row_blocks][G], which a small kernel folds.
//
// Every function here is inlined.  DESIGN.md, section 24, compares each kernel's machine code with the same kernel written
// out; where sharing changed a kernel's loops or registers the code stays written out:
//   count_summary's accumulate and rows4 keep `VEC ? g0 + j : g0 + 256 * j` (strip_gene there changed the register counts);
//   markers_pass_kernel keeps its store loop (for_lane_genes there changed the row loops);
//   autocorr keeps load_counts<V, WIDE>: V = 1 or 4 contiguous genes per lane over tiles of 64 V genes, not over strips;
//   markers' sum_rows and autocorr's gather_row keep their batched reads of indexed rows: a shared skeleton taking the row
//   index, the fetch, the sum and the flag as callables changed markers_pass_kernel's register counts.
// (embed_moments_kernel's row loop also changed, with load_row4; it was timed instead and keeps the shared load.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// The lane's first column of the strip, and its first gene.
template <bool VEC>
__device__ __forceinline__ int strip_col(int tid) { return VEC ? 4 * tid : tid; }

template <bool VEC>
__device__ __forceinline__ int64_t strip_g0(int64_t gbase, int tid) { return gbase + strip_col<VEC>(tid); }

// The gene of the lane's slot j (0 .. 3).
template <bool VEC>
__device__ __forceinline__ int64_t strip_gene(int64_t g0, int j) { return VEC ? g0 + j : g0 + 256 * j; }

// Does the block's strip lie wholly below gene `end`?  Block-uniform.
__device__ __forceinline__ bool strip_whole(int64_t gbase, int64_t end) { return gbase + kStrip <= end; }

// The lane's four counts of row rp.  VEC and `whole` (= strip_whole(gbase, end), block-uniform): one 16-byte load.
// Otherwise four 4-byte loads; genes from `end` on read nothing and count as 0.
template <bool VEC>
__device__ __forceinline__ void load_row4(int32_t (&x)[4], const int32_t* __restrict__ rp, int64_t g0, int64_t end, bool whole)
{
    if (VEC && whole) {
        const int4 v = *reinterpret_cast<const int4*>(rp + g0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t g = strip_gene<VEC>(g0, j);
            x[j] = g < end ? rp[g] : 0;
        }
    }
}

// The same for a kernel that is instantiated once for whole strips (WIDE, only with VEC) and once for the rest.
template <bool VEC, bool WIDE>
__device__ __forceinline__ void load_row4(int32_t (&x)[4], const int32_t* __restrict__ rp, int64_t g0, int64_t end)
{
    load_row4<VEC>(x, rp, g0, end, WIDE);
}

// f(j, at + g) for each of the lane's genes g below G: the stores of a lane's sums to the block's row of a slab.
template <bool VEC, typename F>
__device__ __forceinline__ void for_lane_genes(int64_t g0, int64_t G, size_t at, F f)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t g = strip_gene<VEC>(g0, j);
        if (g < G) f(j, at + g);
    }
}

// The fold of two binary64 slabs [row_blocks][G], a thread per gene: row block 0 upward, which is part of the result.
__device__ __forceinline__ void fold_two_slabs(const double* __restrict__ s1slab, const double* __restrict__ s2slab, int64_t G,
                                               int64_t row_blocks, double* __restrict__ S1, double* __restrict__ S2)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    double a = 0.0, b = 0.0;
    for (int64_t k = 0; k < row_blocks; ++k) {
        a += s1slab[k * G + g];
        b += s2slab[k * G + g];
    }
    S1[g] = a;
    S2[g] = b;
}
