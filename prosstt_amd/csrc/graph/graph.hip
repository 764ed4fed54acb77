// libprosstt_amd_graph.so -- fuzzy connectivities of a kNN graph and the diffusion operator on it
// (include/prosstt_amd_graph.h has the definitions).  256 threads = 4 waves per block, 64-bit offsets, no floating-point
// atomic: every sum is a lane's own ascending partial sum followed by a fixed xor shuffle tree, in which both lanes of a
// pair add the same two numbers, so all lanes of a group hold the same bits and every branch on a sum is group-uniform.
//   graph_memberships_kernel  one wave per row.  The row's k <= 1024 distances stay in registers, lane-strided (entry c in
//                             lane c & 63, slot c >> 6: 16 slots, the unused ones +inf so that their exp is 0).  rho, the
//                             mean and each of the 64 evaluations of f are wave reductions.  Checks the values.
//   graph_emit_kernel         entry e = (i, r) becomes the keyed entries 2e and 2e + 1 of the workspace.
//   graph_fold_kernel         sorted_runs.h's fold of the sorted entries into W: a run combines as (w + b) - w b.
//   graph_normalize_kernel    16 lanes per row: <0> q = W 1; <1> K = W / (q_i q_j) into T and z = sqrt(K 1); <2> T = K /
//                             (z_i z_j) in place.
//   graph_spmv_kernel<G>      G lanes per row (4, 16, 64); lane s takes entries s, s + G, ..: a group's loads of columns
//                             and values are consecutive, x is gathered.  A row longer than G is a loop.
#include "../../../include/prosstt_amd_graph.h"

#define ABI_EINVAL PROSSTT_AMD_GRAPH_EINVAL
#define ABI_EHIP PROSSTT_AMD_GRAPH_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // the refusals and grid rules of the graph libraries, symmetrize_fold
#include "../sorted_runs.h"               // fold_sorted_runs
#include "../wave_reduce.h"               // group_sum, wave_sum, wave_min

#include <cmath>

namespace {

constexpr int kMaxK = 1024;
constexpr int kSlots = kMaxK / 64;             // distances of a row per lane
constexpr int kBisections = 64;
constexpr int kNormLanes = 16;                 // lanes per row of the normalisation

// -------------------------------------------------------------------------------------------------------- memberships

__device__ __forceinline__ double row_f(const double (&g)[kSlots], int nr, double s)
{
    double f = 0.0;
#pragma unroll
    for (int r = 0; r < kSlots; ++r)
        if (r < nr) f += exp(-g[r] / s);
    return group_sum<64>(f);
}

__global__ __launch_bounds__(kThreads) void graph_memberships_kernel(const int32_t* __restrict__ index,
                                                                     const float* __restrict__ sqdist, int64_t N, int k,
                                                                     double target, double* __restrict__ a,
                                                                     double* __restrict__ rho, double* __restrict__ sigma,
                                                                     uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                               // wave-uniform
    const int nr = (k + 63) >> 6;
    const int64_t base = i * k;
    const double inf = INFINITY;

    double g[kSlots];
    double dsum = 0.0, dmin = inf;
    uint32_t bad = 0u;
#pragma unroll
    for (int r = 0; r < kSlots; ++r) {
        g[r] = inf;
        const int c = 64 * r + lane;
        if (r < nr && c < k) {
            const int64_t j = index[base + c];
            float d2 = sqdist[base + c];
            if (j < 0 || j >= N) bad |= PROSSTT_AMD_GRAPH_BAD_INDEX;
            else if (j == i) bad |= PROSSTT_AMD_GRAPH_BAD_SELF;
            if (!(d2 >= 0.0f) || d2 == INFINITY) {
                bad |= PROSSTT_AMD_GRAPH_BAD_DISTANCE;
                d2 = 0.0f;
            }
            const double d = sqrt((double)d2);
            g[r] = d;
            dsum += d;
            if (d > 0.0) dmin = fmin(dmin, d);
        }
    }
    if (bad) atomicOr(status, bad);
    dsum = group_sum<64>(dsum);
    dmin = wave_min(dmin);
    const double rho_i = dmin == inf ? 0.0 : dmin;
#pragma unroll
    for (int r = 0; r < kSlots; ++r) g[r] = fmax(g[r] - rho_i, 0.0);      // (inf stays inf)

    double lo = 0.0, hi = inf, mid = 1.0;
    for (int it = 0; it < kBisections; ++it) {
        if (row_f(g, nr, mid) > target) {
            hi = mid;
            mid = (lo + hi) / 2;
        } else {
            lo = mid;
            mid = hi == inf ? 2 * mid : (lo + hi) / 2;
        }
    }
    const double sigma_i = fmax(mid, 1e-3 * (dsum / (double)k));
#pragma unroll
    for (int r = 0; r < kSlots; ++r) {
        const int c = 64 * r + lane;
        if (r < nr && c < k) a[base + c] = g[r] == 0.0 ? 1.0 : exp(-g[r] / sigma_i);
    }
    if (lane == 0) {
        rho[i] = rho_i;
        sigma[i] = sigma_i;
    }
}

// ------------------------------------------------------------------------------------------------------ symmetrisation

__global__ __launch_bounds__(kThreads) void graph_emit_kernel(const int32_t* __restrict__ index, const double* __restrict__ a,
                                                              int64_t entries, int64_t k, int64_t* __restrict__ keys,
                                                              double* __restrict__ vals)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < entries; e += stride) {
        const int64_t i = e / k, j = (int64_t)(uint32_t)index[e];
        const double v = a[e];
        keys[2 * e] = (i << 32) | j;
        keys[2 * e + 1] = (j << 32) | i;
        vals[2 * e] = v;
        vals[2 * e + 1] = v;
    }
}

__global__ __launch_bounds__(kThreads) void graph_fold_kernel(const int64_t* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                              const int64_t* __restrict__ pos, const double* __restrict__ vals,
                                                              int64_t M, int64_t N, int64_t nnz, int64_t* __restrict__ indptr,
                                                              int32_t* __restrict__ indices, double* __restrict__ data)
{
    fold_sorted_runs(
        sorted, perm, pos, vals, M, N, nnz, indptr, indices, data, [](double w, double b) { return (w + b) - w * b; },
        [](double w) { return w; });
}

// ------------------------------------------------------------------------------------------------------- normalisation

template <int MODE>
__global__ __launch_bounds__(kThreads) void graph_normalize_kernel(const int64_t* __restrict__ indptr,
                                                                   const int32_t* __restrict__ indices,
                                                                   const double* __restrict__ W, double* __restrict__ T,
                                                                   const double* __restrict__ scale, double* __restrict__ sums,
                                                                   int64_t N, uint32_t* __restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = t / kNormLanes;
    const int sub = (int)(t % kNormLanes);
    const bool ok = row < N;
    const int64_t begin = ok ? indptr[row] : 0, end = ok ? indptr[row + 1] : 0;
    const double si = (MODE != 0 && ok) ? scale[row] : 1.0;
    double acc = 0.0;
    for (int64_t e = begin + sub; e < end; e += kNormLanes) {
        if (MODE == 0) {
            acc += W[e];
        } else {
            const double v = (MODE == 1 ? W[e] : T[e]) / (si * scale[indices[e]]);
            T[e] = v;
            acc += v;
        }
    }
    if (MODE == 2) return;
    acc = group_sum<kNormLanes>(acc);
    if (ok && sub == 0) {
        if (!(acc > 0.0) || acc == INFINITY) atomicOr(status, (uint32_t)PROSSTT_AMD_GRAPH_BAD_DEGREE);
        sums[row] = MODE == 0 ? acc : sqrt(acc);
    }
}

// ------------------------------------------------------------------------------------------------------------ product

template <int G>
__global__ __launch_bounds__(kThreads) void graph_spmv_kernel(const int64_t* __restrict__ indptr,
                                                              const int32_t* __restrict__ indices,
                                                              const double* __restrict__ T, const double* __restrict__ x,
                                                              double* __restrict__ y, int64_t N)
{
    const int64_t row = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < N;
    const int64_t begin = ok ? indptr[row] : 0, end = ok ? indptr[row + 1] : 0;
    double acc = 0.0;
    for (int64_t e = begin + sub; e < end; e += G) acc = fma(T[e], x[indices[e]], acc);
    acc = group_sum<G>(acc);
    if (ok && sub == 0) y[row] = acc;
}

int choose_lanes(int64_t N, int64_t nnz)
{
    // measured at 50 000 rows: 16 and 64 lanes tie at 24 entries per row, 64 lanes win from 160 on, and
    // 4 lanes lose everywhere (they stay as a forced path)
    return nnz / N < 64 ? 16 : 64;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_graph_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_graph_workspace_bytes(int64_t N, int64_t k, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, k, kMaxK)) return rc;
    *bytes = 2 * half_workspace(N, k);
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_graph_memberships(void* stream, const int32_t* index, const float* sqdist, int64_t N, int64_t k,
                                             double* a, double* rho, double* sigma, uint32_t* status) try
{
    if (int rc = check_sizes(N, k, kMaxK)) return rc;
    if (!index || !sqdist || !a || !rho || !sigma || !status) return fail(ABI_EINVAL, "NULL argument");
    graph_memberships_kernel<<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        index, sqdist, N, (int)k, std::log2((double)(k + 1)), a, rho, sigma, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_graph_symmetrize_emit(void* stream, const int32_t* index, const double* a, int64_t N, int64_t k,
                                                 void* ws, uint64_t ws_bytes) try
{
    if (int rc = check_sizes(N, k, kMaxK)) return rc;
    if (!index || !a) return fail(ABI_EINVAL, "NULL argument");
    const size_t half = half_workspace(N, k);
    if (int rc = check_workspace(ws, ws_bytes, 2 * half)) return rc;
    graph_emit_kernel<<<dim3(stride_blocks(N * k)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        index, a, N * k, k, (int64_t*)ws, (double*)((char*)ws + half));
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_graph_symmetrize_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm,
                                                 const int64_t* pos, int64_t N, int64_t k, int64_t nnz, const void* ws,
                                                 uint64_t ws_bytes, int64_t* indptr, int32_t* indices, double* data) try
{
    return symmetrize_fold(graph_fold_kernel, kMaxK, stream, sorted_keys, perm, pos, N, k, nnz, ws, ws_bytes, indptr, indices,
                           data);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_graph_normalize(void* stream, const int64_t* indptr, const int32_t* indices, const double* W,
                                           int64_t N, int64_t nnz, double* T, double* q, double* z, uint32_t* status) try
{
    if (int rc = check_csr(N, nnz)) return rc;
    if (!indptr || !indices || !W || !T || !q || !z || !status) return fail(ABI_EINVAL, "NULL argument");
    if (T == W) return fail(ABI_EINVAL, "T must not alias W");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv(N, kThreads / kNormLanes)), block(kThreads);
    graph_normalize_kernel<0><<<grid, block, 0, st>>>(indptr, indices, W, T, nullptr, q, N, status);
    HIP_TRY(hipGetLastError());
    graph_normalize_kernel<1><<<grid, block, 0, st>>>(indptr, indices, W, T, q, z, N, status);
    HIP_TRY(hipGetLastError());
    graph_normalize_kernel<2><<<grid, block, 0, st>>>(indptr, indices, W, T, z, nullptr, N, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_graph_spmv(void* stream, const int64_t* indptr, const int32_t* indices, const double* T, int64_t N,
                                      int64_t nnz, const double* x, double* y, int32_t lanes_per_row) try
{
    if (int rc = check_csr(N, nnz)) return rc;
    if (!indptr || !indices || !T || !x || !y) return fail(ABI_EINVAL, "NULL argument");
    if (x == y) return fail(ABI_EINVAL, "y must not alias x");
    const int g = lanes_per_row ? lanes_per_row : choose_lanes(N, nnz);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(kThreads);
    switch (g) {
    case 4: graph_spmv_kernel<4><<<dim3((unsigned)cdiv(N, kThreads / 4)), block, 0, st>>>(indptr, indices, T, x, y, N); break;
    case 16: graph_spmv_kernel<16><<<dim3((unsigned)cdiv(N, kThreads / 16)), block, 0, st>>>(indptr, indices, T, x, y, N); break;
    case 64: graph_spmv_kernel<64><<<dim3((unsigned)cdiv(N, kThreads / 64)), block, 0, st>>>(indptr, indices, T, x, y, N); break;
    default: return fail(ABI_EINVAL, "lanes_per_row must be 0, 4, 16 or 64 (got %d)", (int)lanes_per_row);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
