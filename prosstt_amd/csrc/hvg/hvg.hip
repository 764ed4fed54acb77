// libprosstt_amd_hvg.so -- the passes over a device count matrix behind the choice of highly variable genes
// (include/prosstt_amd_hvg.h).
//
// Kernels (256 threads = 4 waves each)
//   hvg_clipped_kernel        count_summary's strip layout: a block owns a strip of 1024 genes over a range of rows.  Per gene
//                             the lane keeps its threshold and its three sums in registers across the rows and stores them to
//                             slabs [row_blocks][G] at the end
//   hvg_clipped_sum_kernel    sums the slabs over the row blocks (64 genes per block, the row blocks split over its four
//                             waves, as count_summary_genes_kernel does) and looks at the thresholds' signs
//   hvg_moments_kernel        the same strip layout for the binary64 sums of y = (float)x * inv_size[i] and y^2: rows in
//                             ascending order, embed_moments_kernel's loop without the log1p
//   hvg_moments_sum_kernel    sums those slabs over the row blocks in ascending order
//   hvg_gather_kernel         Y[r][c] = X[r][cols[c]]: a block owns 256 selected columns (a lane each, so the writes of a row
//                             coalesce) over a range of rows and loads its 256 entries of cols once
// The integer sums are exact and the binary64 sums have a fixed order: no atomics but the OR of a status bit.
//
// Exactness of the clipped pass.  A kept count is at most the threshold < 2^31, so what count_summary says of its sums
// holds: per gene in one block S1 < 2^62 (u64), S2 as a u64 low word plus a u32 count of its carries, the count of
// entries over the threshold < 2^31 (u32); over the row blocks S2 in 128 bits and the count in u64.
#include "../../../include/prosstt_amd_hvg.h"

#define ABI_EINVAL PROSSTT_AMD_HVG_EINVAL
#define ABI_EHIP PROSSTT_AMD_HVG_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, load_row4, for_lane_genes, fold_two_slabs
#include "../log1p_entry.h"                 // scaled(): the float32 x * inv that embed's log1p entry starts from

namespace {

constexpr int kGatherRows = 32;             // rows per block of the gather: cols is read once per 32 rows
constexpr int64_t kMaxGridY = 65535;

struct Geometry {
    StripGeometry grid;
    size_t s1 = 0, s2lo = 0, s2hi = 0, over = 0;     // clipped pass: offsets of the slabs in the workspace
    size_t m2 = 0;                                   // moments: offset of the S2 slab (S1 at 0)
    size_t bytes = 0;
};

Geometry geometry(int64_t N, int64_t G)
{
    Geometry g;
    g.grid = strip_geometry(N, G);
    const size_t cells = (size_t)g.grid.row_blocks * (size_t)G;
    g.s1 = 0;
    g.s2lo = g.s1 + pad(cells * 8);
    g.s2hi = g.s2lo + pad(cells * 8);
    g.over = g.s2hi + pad(cells * 4);
    g.bytes = g.over + pad(cells * 4);
    g.m2 = pad(cells * 8);                           // (two binary64 slabs: less than the clipped pass's four)
    return g;
}

// ---------------------------------------------------------------------------------------------------- clipped sums

struct ClipSlabs {
    uint64_t* s1;      // [row_blocks][G]
    uint64_t* s2lo;    // [row_blocks][G]
    uint32_t* s2hi;    // [row_blocks][G] carries out of s2lo
    uint32_t* over;    // [row_blocks][G]
};

struct ClipAcc {
    uint64_t s1[4], s2lo[4];
    uint32_t s2hi[4], over[4];
    int32_t neg;
};

__device__ __forceinline__ void clip_add(const int32_t (&x)[4], const uint32_t (&t)[4], ClipAcc& a)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        a.neg |= x[j];
        const uint32_t v = (uint32_t)x[j];
        const bool above = v > t[j];
        a.over[j] += above ? 1u : 0u;
        const uint32_t w = above ? 0u : v;
        a.s1[j] += w;
        const uint64_t sq = uint64_t(w) * w;
        a.s2lo[j] += sq;
        a.s2hi[j] += (a.s2lo[j] < sq) ? 1u : 0u;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads, 4) void hvg_clipped_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                  int64_t ld, const int32_t* __restrict__ threshold,
                                                                  int64_t rows_per_block, ClipSlabs s,
                                                                  uint32_t* __restrict__ status)
{
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.x * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
    const bool full = strip_whole(gbase, G);

    uint32_t t[4];
    ClipAcc a;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t g = strip_gene<VEC>(g0, j);
        t[j] = g < G ? (uint32_t)threshold[g] : 0u;     // (a negative threshold: hvg_clipped_sum_kernel reports it)
        a.s1[j] = 0; a.s2lo[j] = 0; a.s2hi[j] = 0; a.over[j] = 0;
    }
    a.neg = 0;

    // One row's load in flight per wave: with eight waves per SIMD that keeps HBM busiest.  At 50 000 x 20 000 the pass took
    // 0.82 ms this way and 0.89 / 0.94 / 0.96 / 1.05 ms with the loads of 2 / 3 / 4 / 8 rows issued ahead.
#pragma unroll 1
    for (int64_t r = r0; r < r1; ++r) {
        int32_t x[4];
        load_row4<VEC>(x, X + r * ld, g0, G, full);
        clip_add(x, t, a);
    }

    const size_t at = (size_t)blockIdx.y * (size_t)G;
    for_lane_genes<VEC>(g0, G, at, [&](int j, size_t i) {
        s.s1[i] = a.s1[j];
        s.s2lo[i] = a.s2lo[j];
        s.s2hi[i] = a.s2hi[j];
        s.over[i] = a.over[j];
    });
    if (a.neg < 0) atomicOr(status, PROSSTT_AMD_HVG_NEGATIVE);
}

__global__ __launch_bounds__(256) void hvg_clipped_sum_kernel(ClipSlabs s, int64_t G, int64_t row_blocks,
                                                              const int32_t* __restrict__ threshold,
                                                              uint64_t* __restrict__ n_over, uint64_t* __restrict__ sum_le,
                                                              uint64_t* __restrict__ sumsq_le, uint32_t* __restrict__ status)
{
    __shared__ uint64_t sh[4][4][64];     // [s1, s2 low, s2 high, over][wave][gene]
    const int gl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 64 + gl;
    uint64_t s1 = 0, lo = 0, hi = 0, over = 0;
    if (g < G) {
#pragma unroll 4
        for (int64_t b = w; b < row_blocks; b += 4) {
            const size_t i = (size_t)b * (size_t)G + (size_t)g;
            s1 += s.s1[i];
            const uint64_t l = s.s2lo[i];
            lo += l;
            hi += (lo < l ? 1u : 0u) + (uint64_t)s.s2hi[i];
            over += s.over[i];
        }
    }
    sh[0][w][gl] = s1; sh[1][w][gl] = lo; sh[2][w][gl] = hi; sh[3][w][gl] = over;
    __syncthreads();
    if (w != 0 || g >= G) return;
    for (int k = 1; k < 4; ++k) {
        s1 += sh[0][k][gl];
        const uint64_t l = sh[1][k][gl];
        lo += l;
        hi += (lo < l ? 1u : 0u) + sh[2][k][gl];
        over += sh[3][k][gl];
    }
    n_over[g] = over;
    sum_le[g] = s1;
    sumsq_le[2 * g] = lo;
    sumsq_le[2 * g + 1] = hi;
    if (threshold[g] < 0) atomicOr(status, PROSSTT_AMD_HVG_RANGE);
}

// ---------------------------------------------------------------------------------------------- normalised moments

template <bool VEC>
__global__ __launch_bounds__(kThreads) void hvg_moments_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                               int64_t ld, const float* __restrict__ inv_size,
                                                               int64_t rows_per_block, double* __restrict__ s1slab,
                                                               double* __restrict__ s2slab, uint32_t* __restrict__ status)
{
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.x * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
    const bool full = strip_whole(gbase, G);
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    int32_t neg = 0;
#pragma unroll 1                            // (one row in flight, as in hvg_clipped_kernel: 0.78 ms; unrolled by 2 / 4: 0.89 / 0.98)
    for (int64_t r = r0; r < r1; ++r) {
        const float inv = inv_size[r];
        int32_t x[4];
        load_row4<VEC>(x, X + r * ld, g0, G, full);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            neg |= x[j];
            const double y = (double)scaled(x[j], inv);
            s1[j] += y;
            s2[j] = __builtin_fma(y, y, s2[j]);         // (y * y is exact in binary64: one rounding either way)
        }
    }
    const size_t at = (size_t)blockIdx.y * (size_t)G;
    for_lane_genes<VEC>(g0, G, at, [&](int j, size_t i) {
        s1slab[i] = s1[j];
        s2slab[i] = s2[j];
    });
    if (neg < 0) atomicOr(status, PROSSTT_AMD_HVG_NEGATIVE);
}

__global__ __launch_bounds__(kThreads) void hvg_moments_sum_kernel(const double* __restrict__ s1slab,
                                                                   const double* __restrict__ s2slab, int64_t G,
                                                                   int64_t row_blocks, double* __restrict__ S1,
                                                                   double* __restrict__ S2)
{
    fold_two_slabs(s1slab, s2slab, G, row_blocks, S1, S2);
}

// ------------------------------------------------------------------------------------------------- gather columns

__global__ __launch_bounds__(kThreads) void hvg_gather_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                              int64_t ld, const int32_t* __restrict__ cols, int64_t n_sel,
                                                              int32_t* __restrict__ Y, int64_t ldy, int64_t rows_per_block,
                                                              uint32_t* __restrict__ status)
{
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n_sel) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
    const int32_t col = cols[c];
    int32_t* __restrict__ dst = Y + c;
    if (col < 0 || col >= G) {                          // reads nothing
        atomicOr(status, PROSSTT_AMD_HVG_RANGE);
        for (int64_t r = r0; r < r1; ++r) dst[r * ldy] = 0;
        return;
    }
    const int32_t* __restrict__ src = X + col;
    int64_t r = r0;
    for (; r + 4 <= r1; r += 4) {                       // four rows' loads in flight
        int32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[(r + k) * ld];
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[(r + k) * ldy] = v[k];
    }
    for (; r < r1; ++r) dst[r * ldy] = src[r * ld];
}

int check_matrix(const int32_t* X, int64_t N, int64_t G, int64_t ld)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_HVG_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (!X) return fail(PROSSTT_AMD_HVG_EINVAL, "NULL argument");
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_hvg_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_hvg_workspace_bytes(int64_t N, int64_t G, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_HVG_EINVAL, "NULL argument");
    if (cells_out_of_range(N) || G < 1) return fail(PROSSTT_AMD_HVG_EINVAL, "need 1 <= N < 2^31 and G >= 1");
    *bytes = geometry(N, G).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_hvg_clipped_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                            const int32_t* threshold, void* ws, uint64_t ws_bytes, uint64_t* n_over,
                                            uint64_t* sum_le, uint64_t* sumsq_le, uint32_t* status) try
{
    if (int rc = check_matrix(X, N, G, ld)) return rc;
    if (!threshold || !n_over || !sum_le || !sumsq_le || !status) return fail(PROSSTT_AMD_HVG_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G);
    if (!ws || ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const ClipSlabs s{(uint64_t*)(w + geo.s1), (uint64_t*)(w + geo.s2lo), (uint32_t*)(w + geo.s2hi), (uint32_t*)(w + geo.over)};
    const dim3 grid((unsigned)geo.grid.strips, (unsigned)geo.grid.row_blocks);
    const int64_t rows = geo.grid.rows_per_block;
    if (aligned(X, ld, 4)) hvg_clipped_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, threshold, rows, s, status);
    else hvg_clipped_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, threshold, rows, s, status);
    HIP_TRY(hipGetLastError());
    hvg_clipped_sum_kernel<<<dim3((unsigned)cdiv(G, 64)), dim3(256), 0, st>>>(s, G, geo.grid.row_blocks, threshold, n_over,
                                                                            sum_le, sumsq_le, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_hvg_normalized_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                                  const float* inv_size, void* ws, uint64_t ws_bytes, double* S1,
                                                  double* S2, uint32_t* status) try
{
    if (int rc = check_matrix(X, N, G, ld)) return rc;
    if (!inv_size || !S1 || !S2 || !status) return fail(PROSSTT_AMD_HVG_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G);
    if (!ws || ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    double* s1 = (double*)ws;
    double* s2 = (double*)((char*)ws + geo.m2);
    const dim3 grid((unsigned)geo.grid.strips, (unsigned)geo.grid.row_blocks);
    const int64_t rows = geo.grid.rows_per_block;
    if (aligned(X, ld, 4)) hvg_moments_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, rows, s1, s2, status);
    else hvg_moments_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, rows, s1, s2, status);
    HIP_TRY(hipGetLastError());
    hvg_moments_sum_kernel<<<dim3((unsigned)cdiv(G, kThreads)), dim3(kThreads), 0, st>>>(s1, s2, G, geo.grid.row_blocks, S1, S2);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_hvg_gather_columns(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                              const int32_t* cols, int64_t n_sel, int32_t* Y, int64_t ldy,
                                              uint32_t* status) try
{
    if (int rc = check_matrix(X, N, G, ld)) return rc;
    if (n_sel < 1 || n_sel >= (int64_t(1) << 31))
        return fail(PROSSTT_AMD_HVG_EINVAL, "need 1 <= n_sel < 2^31 (got %lld)", (long long)n_sel);
    if (ldy < n_sel) return stride_below_row(ldy, n_sel);
    if (!cols || !Y || !status) return fail(PROSSTT_AMD_HVG_EINVAL, "NULL argument");
    const int64_t row_blocks = clamp64(cdiv(N, kGatherRows), 1, kMaxGridY);
    const int64_t rows = cdiv(N, row_blocks);
    const dim3 grid((unsigned)cdiv(n_sel, kThreads), (unsigned)cdiv(N, rows));
    hvg_gather_kernel<<<grid, dim3(kThreads), 0, (hipStream_t)stream>>>(X, N, G, ld, cols, n_sel, Y, ldy, rows, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
