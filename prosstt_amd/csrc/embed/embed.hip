// libprosstt_amd_embed.so -- passes over a device count matrix for a PCA of log1p(X / s) (include/prosstt_amd_embed.h).
//
// Kernels (256 threads = 4 waves each; A[i][j] = log1p(X[i][j] * inv_size[i]) is formed in registers, never stored)
//   embed_moments_kernel    a block owns a strip of 1024 genes over a range of rows; per gene the lane keeps S1 and S2 in
//                           binary64 registers and stores them to slabs [row_blocks][G] at the end
//   embed_matmul_kernel     Y = A.W, a matrix-core product (mfma_device.h: the operand mapping, the lane's 16 counts of a
//                           step, the k-steps and the tile map): a block owns 128 rows (32 per wave) over one part of the
//                           genes, all l columns, and stages the 32 x l slice of W of a step of 32 genes in LDS.  Partials
//                           go to a slab [parts][N][lp]
//   embed_rmatmul_kernel    Z = A^T.Q, the same product summed over the rows: a block owns 256 genes (64 per wave: two per
//                           lane, one 8-byte load per row, so two accumulator sets) over a range of rows and stages the
//                           32 x l slice of Q of a step of 32 rows in LDS.  Partials go to a slab [row_blocks][G][lp]
//   embed_sum_panels_kernel / embed_sum_moments_kernel  sum a slab over its parts in ascending order
// There are no floating-point atomics: the results do not depend on scheduling, and equal inputs give equal bits.
//
// What the products add to mfma_device.h: entry() forms A from the counts between the load and the k-steps, the summed
// index is split into parts (matmul: genes, rmatmul: rows) whose partial tiles go to slabs, and lp = l rounded up to 32:
// the panel's extra columns and the masked rows and genes of a step are zeros, so every l in 1..128 runs the same code.
#include "../../../include/prosstt_amd_embed.h"

#define ABI_EINVAL PROSSTT_AMD_EMBED_EINVAL
#define ABI_EHIP PROSSTT_AMD_EMBED_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, load_row4, for_lane_genes, fold_two_slabs
#include "../log1p_entry.h"                 // entry(): the float32 log1p(x * inv), shared with markers/markers.hip
#include "../mfma_device.h"                 // f32x16, kStep, load_row16, mfma_steps, tile_row, with_instantiation

namespace {

constexpr int kRowsMM = 128;                // matmul: rows per block, 32 per wave
constexpr int kGenesRM = 256;               // rmatmul: genes per block, 64 per wave

struct Geometry {
    int64_t lp = 0;                                   // panel width rounded up to 32
    StripGeometry m;                                  // moments
    int64_t mm_parts = 0, mm_genes_per_part = 0;      // matmul (blocks: ceil(N / 128) x parts)
    int64_t rm_row_blocks = 0, rm_rows_per_block = 0; // rmatmul (blocks: ceil(G / 256) x row_blocks)
    size_t m_bytes = 0, mm_bytes = 0, rm_bytes = 0, bytes = 0;
};

Geometry geometry(int64_t N, int64_t G, int64_t l)
{
    Geometry g;
    g.lp = cdiv(l, 32) * 32;
    g.m = strip_geometry(N, G);
    g.m_bytes = 2 * pad((size_t)g.m.row_blocks * (size_t)G * 8);

    const int64_t chunks = cdiv(G, kStep);
    const int64_t parts = clamp64(kTargetBlocks / cdiv(N, kRowsMM), 1, chunks);
    g.mm_genes_per_part = cdiv(chunks, parts) * kStep;
    g.mm_parts = cdiv(G, g.mm_genes_per_part);
    g.mm_bytes = pad((size_t)g.mm_parts * (size_t)N * (size_t)g.lp * 4);

    const int64_t row_steps = cdiv(N, kStep);
    const int64_t rb = clamp64(kTargetBlocks / cdiv(G, kGenesRM), 1, row_steps);
    g.rm_rows_per_block = cdiv(row_steps, rb) * kStep;
    g.rm_row_blocks = cdiv(N, g.rm_rows_per_block);
    g.rm_bytes = pad((size_t)g.rm_row_blocks * (size_t)G * (size_t)g.lp * 4);

    g.bytes = g.m_bytes > g.mm_bytes ? g.m_bytes : g.mm_bytes;
    if (g.rm_bytes > g.bytes) g.bytes = g.rm_bytes;
    return g;
}

// ---------------------------------------------------------------------------------------------------------- moments

template <bool VEC>
__global__ __launch_bounds__(kThreads) void embed_moments_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
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
#pragma unroll 2
    for (int64_t r = r0; r < r1; ++r) {
        const int32_t* rp = X + r * ld;
        const float inv = inv_size[r];
        int32_t x[4];
        load_row4<VEC>(x, rp, g0, G, full);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            neg |= x[j];
            const double a = (double)entry(x[j], inv);
            s1[j] += a;
            s2[j] = __builtin_fma(a, a, s2[j]);
        }
    }
    const size_t at = (size_t)blockIdx.y * (size_t)G;
    for_lane_genes<VEC>(g0, G, at, [&](int j, size_t i) {
        s1slab[i] = s1[j];
        s2slab[i] = s2[j];
    });
    if (neg < 0) atomicOr(status, 1u);
}

__global__ __launch_bounds__(kThreads) void embed_sum_moments_kernel(const double* __restrict__ s1slab,
                                                                     const double* __restrict__ s2slab, int64_t G,
                                                                     int64_t row_blocks, double* __restrict__ S1,
                                                                     double* __restrict__ S2)
{
    fold_two_slabs(s1slab, s2slab, G, row_blocks, S1, S2);
}

// ------------------------------------------------------------------------------------------------------------ A . W

// The thread's share of a 32 x lp panel slice: rows k0 .. k0 + 31 of P (row-major, l columns), zeros outside [k0, kend)
// and in the columns l .. lp - 1.
template <int NT>
__device__ __forceinline__ void load_panel(float (&p)[NT * 4], const float* __restrict__ P, int64_t l, int64_t k0,
                                           int64_t kend, int tid)
{
    constexpr int LP = NT * 32;
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) {
        const int idx = tid + q * kThreads;
        const int k = idx / LP, col = idx % LP;
        p[q] = (k0 + k < kend && col < l) ? P[(k0 + k) * l + col] : 0.0f;
    }
}

template <int NT>
__device__ __forceinline__ void stage_panel(float* sh, const float (&p)[NT * 4], int tid)
{
    constexpr int LP = NT * 32, LS = slice_stride(NT);
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) {
        const int idx = tid + q * kThreads;
        sh[(idx / LP) * LS + idx % LP] = p[q];
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kThreads) void embed_matmul_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                int64_t ld, const float* __restrict__ inv_size,
                                                                const float* __restrict__ W, int64_t l,
                                                                int64_t genes_per_part, float* __restrict__ slab,
                                                                uint32_t* __restrict__ status)
{
    constexpr int LP = NT * 32;
    __shared__ float wsh[kStep * slice_stride(NT)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int64_t rbase = (int64_t)blockIdx.x * kRowsMM + wave * 32;
    const int64_t r = rbase + c;
    const bool row_ok = r < N;
    const int32_t* __restrict__ rp = X + (row_ok ? r : 0) * ld;
    const float inv = row_ok ? inv_size[r] : 0.0f;
    const int64_t gb = (int64_t)blockIdx.y * genes_per_part;
    const int64_t ge = (gb + genes_per_part < G) ? gb + genes_per_part : G;

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x16{};
    int32_t x[16];
    float wp[NT * 4];
    int32_t neg = 0;
    load_row16<VEC>(x, rp, row_ok, gb, ge, h);
    load_panel<NT>(wp, W, l, gb, ge, tid);
    for (int64_t g0 = gb; g0 < ge; g0 += kStep) {
        float a[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            neg |= x[q];
            a[q] = entry(x[q], inv);
        }
        stage_panel<NT>(wsh, wp, tid);
        __syncthreads();
        if (g0 + kStep < ge) {                      // the next step's loads fly during this step's products
            load_row16<VEC>(x, rp, row_ok, g0 + kStep, ge, h);
            load_panel<NT>(wp, W, l, g0 + kStep, ge, tid);
        }
        mfma_steps<NT>(acc, a, wsh, h, c);
        __syncthreads();
    }
    if (neg < 0) atomicOr(status, 1u);
    float* out = slab + (size_t)blockIdx.y * (size_t)N * LP;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t row = rbase + tile_row(reg, h);
        if (row < N) {
#pragma unroll
            for (int t = 0; t < NT; ++t) out[row * LP + 32 * t + c] = acc[t][reg];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- A^T . Q

// The lane's two genes gw, gw + 1 on rows i0 + 16h + s, s = 0..15 (zeros outside [i0, r1) and past G).
template <bool VEC>
__device__ __forceinline__ void load_cols2(int32_t (&x)[16][2], const int32_t* __restrict__ X, int64_t ld, int64_t G,
                                           int64_t gw, int64_t i0, int64_t r1, int h)
{
    const int64_t i = i0 + 16 * h;
    if (VEC && i0 + kStep <= r1 && gw + 2 <= G) {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int2 v = *reinterpret_cast<const int2*>(X + (i + s) * ld + gw);
            x[s][0] = v.x; x[s][1] = v.y;
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int u = 0; u < 2; ++u) x[s][u] = (i + s < r1 && gw + u < G) ? X[(i + s) * ld + gw + u] : 0;
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kThreads) void embed_rmatmul_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                 int64_t ld, const float* __restrict__ inv_size,
                                                                 const float* __restrict__ Q, int64_t l,
                                                                 int64_t rows_per_block, float* __restrict__ slab,
                                                                 uint32_t* __restrict__ status)
{
    constexpr int LP = NT * 32;
    __shared__ float qsh[kStep * slice_stride(NT)];
    __shared__ float ish[kStep];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int64_t gwave = (int64_t)blockIdx.x * kGenesRM + wave * 64;
    const int64_t gw = gwave + 2 * c;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;

    f32x16 acc[2][NT];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[u][t] = f32x16{};
    int32_t x[16][2];
    float qp[NT * 4];
    float iv = 0.0f;
    int32_t neg = 0;
    load_cols2<VEC>(x, X, ld, G, gw, r0, r1, h);
    load_panel<NT>(qp, Q, l, r0, r1, tid);
    if (tid < kStep) iv = (r0 + tid < r1) ? inv_size[r0 + tid] : 0.0f;
    for (int64_t i0 = r0; i0 < r1; i0 += kStep) {
        stage_panel<NT>(qsh, qp, tid);
        if (tid < kStep) ish[tid] = iv;
        __syncthreads();
        float a[16][2];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float inv = ish[16 * h + s];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                neg |= x[s][u];
                a[s][u] = entry(x[s][u], inv);
            }
        }
        if (i0 + kStep < r1) {                      // the next step's loads fly during this step's products
            const int64_t i1 = i0 + kStep;
            load_cols2<VEC>(x, X, ld, G, gw, i1, r1, h);
            load_panel<NT>(qp, Q, l, i1, r1, tid);
            if (tid < kStep) iv = (i1 + tid < r1) ? inv_size[i1 + tid] : 0.0f;
        }
        mfma_steps<NT>(acc, a, qsh, h, c);
        __syncthreads();
    }
    if (neg < 0) atomicOr(status, 1u);
    float* out = slab + (size_t)blockIdx.y * (size_t)G * LP;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t gi = gwave + 2 * tile_row(reg, h);   // tile row i is gene gwave + 2i + u
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (gi + u < G) {
#pragma unroll
                for (int t = 0; t < NT; ++t) out[(gi + u) * LP + 32 * t + c] = acc[u][t][reg];
            }
        }
    }
}

// out[r][c] = sum over p = 0, 1, .. of slab[p][r][c], for c < l (out: rows x l, slab rows of lp floats)
__global__ __launch_bounds__(kThreads) void embed_sum_panels_kernel(const float* __restrict__ slab, int64_t parts,
                                                                    int64_t rows, int64_t lp, int64_t l,
                                                                    float* __restrict__ out)
{
    const int64_t total = rows * l;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t r = idx / l, c = idx - r * l;
        float s = slab[r * lp + c];
        for (int64_t p = 1; p < parts; ++p) s += slab[(p * rows + r) * lp + c];
        out[idx] = s;
    }
}

int sum_panels(hipStream_t st, const float* slab, int64_t parts, int64_t rows, int64_t lp, int64_t l, float* out)
{
    const int64_t blocks = clamp64(cdiv(rows * l, kThreads), 1, int64_t(1) << 20);
    embed_sum_panels_kernel<<<dim3((unsigned)blocks), dim3(kThreads), 0, st>>>(slab, parts, rows, lp, l, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int check_common(const int32_t* X, int64_t N, int64_t G, int64_t ld, const float* inv_size, void* ws, uint32_t* status)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_EMBED_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (!X || !inv_size || !ws || !status) return fail(PROSSTT_AMD_EMBED_EINVAL, "NULL argument");
    return 0;
}

int check_l(int64_t l)
{
    if (l < 1 || l > 128) return fail(PROSSTT_AMD_EMBED_EINVAL, "need 1 <= l <= 128 (got %lld)", (long long)l);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_embed_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_embed_workspace_bytes(int64_t N, int64_t G, int64_t l, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_EMBED_EINVAL, "NULL argument");
    if (cells_out_of_range(N) || G < 1) return fail(PROSSTT_AMD_EMBED_EINVAL, "need 1 <= N < 2^31 and G >= 1");
    if (int rc = check_l(l)) return rc;
    *bytes = geometry(N, G, l).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_embed_gene_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                              const float* inv_size, void* ws, uint64_t ws_bytes, double* S1, double* S2,
                                              uint32_t* status) try
{
    if (int rc = check_common(X, N, G, ld, inv_size, ws, status)) return rc;
    if (!S1 || !S2) return fail(PROSSTT_AMD_EMBED_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, 1);
    if (ws_bytes < geo.m_bytes) return workspace_too_small(ws_bytes, geo.m_bytes);
    hipStream_t st = (hipStream_t)stream;
    double* s1 = (double*)ws;
    double* s2 = (double*)((char*)ws + geo.m_bytes / 2);
    const dim3 grid((unsigned)geo.m.strips, (unsigned)geo.m.row_blocks);
    if (aligned(X, ld, 4))
        embed_moments_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, geo.m.rows_per_block, s1, s2, status);
    else
        embed_moments_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, geo.m.rows_per_block, s1, s2, status);
    HIP_TRY(hipGetLastError());
    embed_sum_moments_kernel<<<dim3((unsigned)cdiv(G, kThreads)), dim3(kThreads), 0, st>>>(s1, s2, G, geo.m.row_blocks, S1, S2);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_embed_matmul(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                        const float* inv_size, const float* W, int64_t l, float* Y, void* ws,
                                        uint64_t ws_bytes, uint32_t* status) try
{
    if (int rc = check_common(X, N, G, ld, inv_size, ws, status)) return rc;
    if (int rc = check_l(l)) return rc;
    if (!W || !Y) return fail(PROSSTT_AMD_EMBED_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, l);
    if (ws_bytes < geo.mm_bytes) return workspace_too_small(ws_bytes, geo.mm_bytes);
    hipStream_t st = (hipStream_t)stream;
    float* slab = (float*)ws;
    const dim3 grid((unsigned)cdiv(N, kRowsMM), (unsigned)geo.mm_parts);
    with_instantiation(geo.lp / 32, aligned(X, ld, 4), [&](auto nt, auto vec) {
        embed_matmul_kernel<nt(), vec()><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, W, l, geo.mm_genes_per_part,
                                                                          slab, status);
    });
    HIP_TRY(hipGetLastError());
    return sum_panels(st, slab, geo.mm_parts, N, geo.lp, l, Y);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_embed_rmatmul(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                         const float* inv_size, const float* Q, int64_t l, float* Z, void* ws,
                                         uint64_t ws_bytes, uint32_t* status) try
{
    if (int rc = check_common(X, N, G, ld, inv_size, ws, status)) return rc;
    if (int rc = check_l(l)) return rc;
    if (!Q || !Z) return fail(PROSSTT_AMD_EMBED_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, l);
    if (ws_bytes < geo.rm_bytes) return workspace_too_small(ws_bytes, geo.rm_bytes);
    hipStream_t st = (hipStream_t)stream;
    float* slab = (float*)ws;
    const dim3 grid((unsigned)cdiv(G, kGenesRM), (unsigned)geo.rm_row_blocks);
    with_instantiation(geo.lp / 32, aligned(X, ld, 2), [&](auto nt, auto vec) {
        embed_rmatmul_kernel<nt(), vec()><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, Q, l, geo.rm_rows_per_block,
                                                                           slab, status);
    });
    HIP_TRY(hipGetLastError());
    return sum_panels(st, slab, geo.rm_row_blocks, G, geo.lp, l, Z);
}
ABI_CATCH
