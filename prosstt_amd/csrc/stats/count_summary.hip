// libprosstt_amd_stats.so -- exact summary statistics of a device count matrix (include/prosstt_amd_stats.h).
//
// Kernels
//   count_summary_kernel        one read of the matrix: a 256-thread block owns a strip of 1024 genes over a range of
//                               rows.  Per gene the lane keeps its sums in registers across the rows and stores them to a
//                               slab [row_blocks][G] at the end; per row the partial of the strip is reduced across the
//                               wave and the block and stored to a slab [strips][N].
//   count_summary_genes_kernel  sums the gene slab over the row blocks (and adds the previous result with ACCUMULATE)
//   count_summary_rows_kernel   sums the row slab over the strips
// All sums are integers, so the results do not depend on the geometry: the slabs are a store-and-sum, no atomics.
//
// Exactness.  Counts are int32 >= 0, so x < 2^31 and x^2 < 2^62.
//   per gene in one block (at most rows_per_block < 2^31 rows): S1 < 2^62 (u64); S2 as a u64 low word plus a u32 count of
//     its carries; zeros < 2^31 (u32)
//   per gene over the row blocks: S1 < 2^62, S2 in 128 bits (low word, high word with carry), zeros in u64
//   per row in one strip (1024 genes): sum < 2^41 and zeros <= 1024, packed as sum | zeros << 48 -- the packed words of
//     the lanes, waves and the four waves of a block add without one field reaching the other
#include "../../../include/prosstt_amd_stats.h"

#define ABI_EINVAL PROSSTT_AMD_STATS_EINVAL
#define ABI_EHIP PROSSTT_AMD_STATS_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, for_lane_genes

namespace {

constexpr int kBatch = 64;                  // rows whose per-row partials wait in LDS between two block barriers
constexpr uint64_t kSumMask = (uint64_t(1) << 48) - 1;

struct Geometry {
    StripGeometry grid;
    size_t s1 = 0, s2lo = 0, s2hi = 0, z = 0, rows = 0, bytes = 0;   // offsets of the slabs in the workspace
};

Geometry geometry(int64_t N, int64_t G)
{
    Geometry g;
    g.grid = strip_geometry(N, G);
    const size_t cells = (size_t)g.grid.row_blocks * (size_t)G;
    g.s1 = 0;
    g.s2lo = g.s1 + pad(cells * 8);
    g.s2hi = g.s2lo + pad(cells * 8);
    g.z = g.s2hi + pad(cells * 4);
    g.rows = g.z + pad(cells * 4);
    g.bytes = g.rows + pad((size_t)g.grid.strips * (size_t)N * 8);
    return g;
}

struct Slabs {
    uint64_t* s1;      // [row_blocks][G]
    uint64_t* s2lo;    // [row_blocks][G]
    uint32_t* s2hi;    // [row_blocks][G] carries out of s2lo
    uint32_t* z;       // [row_blocks][G]
    uint64_t* rows;    // [strips][N] packed: sum | zeros << 48
};

struct Acc {
    uint64_t s1[4], s2lo[4];
    uint32_t s2hi[4], z[4];
    int32_t neg;
};

// The sums of four rows of the lane's four genes (see rows4).  x^2 + s2lo is one v_mad_u64_u32, whose carry-out feeds s2hi.
// (Here and in rows4 the gene of slot j stays written out: see strip_device.h.)
template <bool VEC, bool MASK>
__device__ __forceinline__ void accumulate(const uint32_t (&x)[4][4], int nrows, int64_t G, int64_t g0, Acc& a, uint64_t p[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t zr = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t v = x[k][j];
            const int64_t g = VEC ? g0 + j : g0 + 256 * j;
            a.s1[j] += v;
            const uint64_t sq = uint64_t(v) * v;
            a.s2lo[j] += sq;
            a.s2hi[j] += (a.s2lo[j] < sq) ? 1u : 0u;
            const uint32_t zero = (v == 0u && (!MASK || (k < nrows && g < G))) ? 1u : 0u;
            a.z[j] += zero;
            zr += zero;
        }
        // two counts < 2^31 sum below 2^32
        const uint64_t s = uint64_t(x[k][0] + x[k][1]) + uint64_t(x[k][2] + x[k][3]);
        p[k] = s | (uint64_t(zr) << 48);
    }
}

// Four rows of the lane's four genes.  VEC: the lane's genes are g0 .. g0+3 (one 16-byte load per row); otherwise
// g0 + 256*j (four coalesced 4-byte loads).  MASK: rows k >= nrows and genes >= G are outside the matrix: they read nothing
// and count for nothing.  Returns the lane's packed per-row partials in p[k].
template <bool VEC, bool MASK>
__device__ __forceinline__ void rows4(const int32_t* __restrict__ X, int64_t row, int nrows, int64_t ld, int64_t G,
                                      int64_t g0, Acc& a, uint64_t p[4])
{
    uint32_t x[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t* rp = X + (row + k) * ld;
        if (VEC && !MASK) {
            const int4 v = *reinterpret_cast<const int4*>(rp + g0);
            x[k][0] = (uint32_t)v.x; x[k][1] = (uint32_t)v.y; x[k][2] = (uint32_t)v.z; x[k][3] = (uint32_t)v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t g = VEC ? g0 + j : g0 + 256 * j;
                x[k][j] = (!MASK || (k < nrows && g < G)) ? (uint32_t)rp[g] : 0u;
            }
        }
    }
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) any |= x[k][j];
    a.neg |= (int32_t)any;
    accumulate<VEC, MASK>(x, nrows, G, g0, a, p);
}

// Butterfly over the wave that sums four rows' partials at once: afterwards lane l holds the wave's total of row l >> 4.
__device__ __forceinline__ uint64_t reduce_rows4(const uint64_t p[4], int lane)
{
    const bool h5 = (lane & 32) != 0, h4 = (lane & 16) != 0;
    uint64_t k0 = h5 ? p[2] : p[0], k1 = h5 ? p[3] : p[1];
    const uint64_t t0 = h5 ? p[0] : p[2], t1 = h5 ? p[1] : p[3];
    k0 += __shfl_xor(t0, 32);
    k1 += __shfl_xor(t1, 32);
    uint64_t v = h4 ? k1 : k0;
    v += __shfl_xor(h4 ? k0 : k1, 16);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(kThreads, 4) void count_summary_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                int64_t ld, int64_t rows_per_block, Slabs s,
                                                                uint32_t* __restrict__ status)
{
    __shared__ uint64_t part[kThreads / 64][kBatch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t strip = blockIdx.x;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
    const int64_t gbase = strip * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const bool full_strip = strip_whole(gbase, G);

    Acc a;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a.s1[j] = 0; a.s2lo[j] = 0; a.s2hi[j] = 0; a.z[j] = 0; }
    a.neg = 0;

    for (int64_t rr = r0; rr < r1; rr += kBatch) {
        const int nb = (int)((r1 - rr < kBatch) ? r1 - rr : kBatch);
        for (int i = 0; i < nb; i += 4) {
            uint64_t p[4];
            if (full_strip && i + 4 <= nb) rows4<VEC, false>(X, rr + i, 4, ld, G, g0, a, p);
            else rows4<VEC, true>(X, rr + i, nb - i, ld, G, g0, a, p);
            const uint64_t v = reduce_rows4(p, lane);
            if ((lane & 15) == 0) part[wave][i + (lane >> 4)] = v;
        }
        __syncthreads();
        if (tid < nb)
            s.rows[strip * N + rr + tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
        __syncthreads();
    }

    const size_t at = (size_t)blockIdx.y * (size_t)G;
    for_lane_genes<VEC>(g0, G, at, [&](int j, size_t i) {
        s.s1[i] = a.s1[j];
        s.s2lo[i] = a.s2lo[j];
        s.s2hi[i] = a.s2hi[j];
        s.z[i] = a.z[j];
    });
    if (a.neg < 0) atomicOr(status, 1u);
}

// 64 genes per block, the row blocks split over its four waves (a wave per gene range walking all row blocks alone left
// 79 blocks at C3 waiting on one load after another: 35 us)
__global__ __launch_bounds__(256) void count_summary_genes_kernel(Slabs s, int64_t G, int64_t row_blocks,
                                                                  uint64_t* __restrict__ gene_sum,
                                                                  uint64_t* __restrict__ gene_sumsq,
                                                                  uint64_t* __restrict__ gene_zeros, int accumulate)
{
    __shared__ uint64_t sh[4][4][64];     // [s1, s2 low, s2 high, zeros][wave][gene]
    const int gl = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 64 + gl;
    uint64_t s1 = 0, lo = 0, hi = 0, z = 0;
    if (g < G) {
#pragma unroll 4
        for (int64_t b = w; b < row_blocks; b += 4) {
            const size_t i = (size_t)b * (size_t)G + (size_t)g;
            s1 += s.s1[i];
            const uint64_t l = s.s2lo[i];
            lo += l;
            hi += (lo < l ? 1u : 0u) + (uint64_t)s.s2hi[i];
            z += s.z[i];
        }
    }
    sh[0][w][gl] = s1; sh[1][w][gl] = lo; sh[2][w][gl] = hi; sh[3][w][gl] = z;
    __syncthreads();
    if (w != 0 || g >= G) return;
    for (int k = 1; k < 4; ++k) {
        s1 += sh[0][k][gl];
        const uint64_t l = sh[1][k][gl];
        lo += l;
        hi += (lo < l ? 1u : 0u) + sh[2][k][gl];
        z += sh[3][k][gl];
    }
    if (accumulate) {
        s1 += gene_sum[g];
        const uint64_t l = gene_sumsq[2 * g];
        lo += l;
        hi += (lo < l ? 1u : 0u) + gene_sumsq[2 * g + 1];
        z += gene_zeros[g];
    }
    gene_sum[g] = s1;
    gene_sumsq[2 * g] = lo;
    gene_sumsq[2 * g + 1] = hi;
    gene_zeros[g] = z;
}

__global__ __launch_bounds__(64) void count_summary_rows_kernel(const uint64_t* __restrict__ rows, int64_t N,
                                                                int64_t strips, uint64_t* __restrict__ cell_total,
                                                                uint64_t* __restrict__ cell_zeros)
{
    const int64_t r = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (r >= N) return;
    uint64_t t = 0, z = 0;
#pragma unroll 4
    for (int64_t s = 0; s < strips; ++s) {
        const uint64_t p = rows[s * N + r];
        t += p & kSumMask;
        z += p >> 48;
    }
    cell_total[r] = t;
    cell_zeros[r] = z;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_stats_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_stats_workspace_bytes(int64_t N, int64_t G, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_STATS_EINVAL, "NULL argument");
    if (cells_out_of_range(N) || G < 0) return fail(PROSSTT_AMD_STATS_EINVAL, "need 1 <= N < 2^31 and G >= 0");
    *bytes = geometry(N, G).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_stats_count_summary(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                               void* workspace, uint64_t workspace_bytes,
                                               uint64_t* gene_sum, uint64_t* gene_sumsq, uint64_t* gene_zeros,
                                               uint64_t* cell_total, uint64_t* cell_zeros, uint32_t* status,
                                               uint32_t flags) try
{
    if (cells_out_of_range(N) || G < 0) return fail(PROSSTT_AMD_STATS_EINVAL, "need 1 <= N < 2^31 and G >= 0");
    if (ld < G) return stride_below_row(ld, G);
    if (!cell_total || !cell_zeros || !status || (G > 0 && (!X || !gene_sum || !gene_sumsq || !gene_zeros)))
        return fail(PROSSTT_AMD_STATS_EINVAL, "NULL argument");
    if (flags & ~PROSSTT_AMD_STATS_ACCUMULATE) return fail(PROSSTT_AMD_STATS_EINVAL, "unknown flag bits 0x%x", flags);
    const Geometry geo = geometry(N, G);
    if (!workspace || workspace_bytes < geo.bytes) return workspace_too_small(workspace_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    const Slabs s{(uint64_t*)(w + geo.s1), (uint64_t*)(w + geo.s2lo), (uint32_t*)(w + geo.s2hi), (uint32_t*)(w + geo.z),
                  (uint64_t*)(w + geo.rows)};
    if (G > 0) {
        const dim3 grid((unsigned)geo.grid.strips, (unsigned)geo.grid.row_blocks);
        const int64_t rows = geo.grid.rows_per_block;
        if (aligned(X, ld, 4)) count_summary_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, rows, s, status);
        else count_summary_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, rows, s, status);
        HIP_TRY(hipGetLastError());
        count_summary_genes_kernel<<<dim3((unsigned)((G + 63) / 64)), dim3(256), 0, st>>>(
            s, G, geo.grid.row_blocks, gene_sum, gene_sumsq, gene_zeros, (flags & PROSSTT_AMD_STATS_ACCUMULATE) ? 1 : 0);
        HIP_TRY(hipGetLastError());
    }
    count_summary_rows_kernel<<<dim3((unsigned)((N + 63) / 64)), dim3(64), 0, st>>>(s.rows, N, geo.grid.strips, cell_total,
                                                                                   cell_zeros);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
