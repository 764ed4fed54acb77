// libprosstt_amd_ptree.so -- the assign and project passes of a principal tree (include/prosstt_amd_ptree.h).
//
// Kernels (the definition is in the header)
//   ptree_distance_kernel     a block owns 64 cells (16 per wave, four at a time) and a tile of 64 centres staged in LDS with an
//                             odd row stride; lane l owns centre l of the tile, the cells' coordinates are wave-uniform loads;
//                             d2 goes to the N x R slab of the workspace
//   ptree_cell_kernel<SOFT>   one wave per cell over its row of the slab: the argmin by key, then exp, Z by the fixed butterfly,
//                             r = w / Z and F; the responsibilities go to the workspace (or to the caller's resp)
//   ptree_sums_kernel<Q,HARD> the tall-skinny product r^T [1 Y] of one chunk of 128 cells: a block owns 32 nodes, thread
//                             (node, s) the coordinates s, s + 8, ... (Q of them); the cells of the chunk are added in
//                             ascending order; HARD reads best instead of the responsibilities
//   ptree_fold_kernel         one thread per entry of [Gamma S]: the chunk sums in ascending chunk order
//   ptree_project_kernel      one wave per cell, lanes over edges, the argmin by key
// There is no floating-point atomic and every sum has a fixed order: equal inputs give equal bits.
#include "../../../include/prosstt_amd_ptree.h"

#define ABI_EINVAL PROSSTT_AMD_PTREE_EINVAL
#define ABI_EHIP PROSSTT_AMD_PTREE_EHIP
#include "../abi_util.h"
#include "../wave_reduce.h"               // wave_sum: the butterfly of Z

namespace {

constexpr int kTile = 64;                           // centres per tile of the distance kernel, one per lane
constexpr int kBlockCells = 64;                     // cells per block of the distance kernel, 16 per wave
constexpr int kMaxDim = PROSSTT_AMD_PTREE_MAX_DIM;
constexpr int kChunk = PROSSTT_AMD_PTREE_CHUNK;
constexpr int kWaves = kThreads / 64;               // cells per block of the one-wave-per-cell kernels
constexpr int kSumNodes = 32;                       // nodes per block of the sums kernel
constexpr int kSumSlots = kThreads / kSumNodes;     // its coordinate slots: thread (node, s) owns c = s, s + 8, ...

__device__ __forceinline__ bool not_finite(float v) { return !(fabsf(v) < __builtin_inff()); }

// ------------------------------------------------------------------------------------------------------ distances

__global__ __launch_bounds__(kThreads) void ptree_distance_kernel(const float* __restrict__ Y, int64_t N, int d, int64_t ld,
                                                                  const float* __restrict__ C, int64_t R, int64_t ldc,
                                                                  float* __restrict__ D, uint32_t* __restrict__ status)
{
    __shared__ float sh[kTile * (kMaxDim + 1)];
    const int LS = d | 1;                           // odd: the 64 lanes of a read hit 32 banks twice, no conflict
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t k0 = (int64_t)blockIdx.y * kTile;
    bool bad = false;
    for (int idx = tid; idx < kTile * d; idx += kThreads) {
        const int node = idx / d, c = idx - node * d;
        const float v = (k0 + node < R) ? C[(k0 + node) * ldc + c] : 0.0f;
        bad |= not_finite(v);
        sh[node * LS + c] = v;
    }
    __syncthreads();
    const float* __restrict__ mine = sh + lane * LS;
    const int64_t k = k0 + lane;
    const int64_t base = (int64_t)blockIdx.x * kBlockCells + wave * (kBlockCells / kWaves);
    for (int g = 0; g < kBlockCells / kWaves; g += 4) {
        const int64_t i0 = base + g;
        if (i0 >= N) break;                         // (wave-uniform)
        const int64_t last = N - 1;
        const float* __restrict__ y0 = Y + i0 * ld;
        const float* __restrict__ y1 = Y + (i0 + 1 < N ? i0 + 1 : last) * ld;
        const float* __restrict__ y2 = Y + (i0 + 2 < N ? i0 + 2 : last) * ld;
        const float* __restrict__ y3 = Y + (i0 + 3 < N ? i0 + 3 : last) * ld;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int c = 0; c < d; ++c) {
            const float cv = mine[c];
            const float v0 = y0[c], v1 = y1[c], v2 = y2[c], v3 = y3[c];
            bad = bad || not_finite(v0) || not_finite(v1) || not_finite(v2) || not_finite(v3);
            const float t0 = v0 - cv, t1 = v1 - cv, t2 = v2 - cv, t3 = v3 - cv;
            a0 = a0 + t0 * t0;
            a1 = a1 + t1 * t1;
            a2 = a2 + t2 * t2;
            a3 = a3 + t3 * t3;
        }
        if (k < R) {
            D[i0 * R + k] = a0;
            if (i0 + 1 < N) D[(i0 + 1) * R + k] = a1;
            if (i0 + 2 < N) D[(i0 + 2) * R + k] = a2;
            if (i0 + 3 < N) D[(i0 + 3) * R + k] = a3;
        }
    }
    if (bad) atomicOr(status, PROSSTT_AMD_PTREE_NONFINITE);
}

// ------------------------------------------------------------------------------------------------------ per cell

__device__ __forceinline__ unsigned long long wave_min_key(unsigned long long key)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(key, off, 64);
        key = other < key ? other : key;
    }
    return key;
}

template <bool SOFT>
__global__ __launch_bounds__(kThreads) void ptree_cell_kernel(const float* __restrict__ D, int64_t N, int64_t R, double sigma,
                                                              int32_t* __restrict__ best, float* __restrict__ d2min,
                                                              double* __restrict__ free_energy, double* __restrict__ resp)
{
    const int lane = threadIdx.x & 63;
    const int64_t cell = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (cell >= N) return;                          // (a whole wave: the shuffles below are among the lanes of one cell)
    const float* __restrict__ row = D + cell * R;
    unsigned long long key = ~0ull;
    for (int64_t k = lane; k < R; k += 64) {
        const unsigned long long mine = ((unsigned long long)__float_as_uint(row[k]) << 32) | (unsigned long long)k;
        key = mine < key ? mine : key;
    }
    key = wave_min_key(key);
    const int b = (int)(key & 0xffffffffull);
    const float m = __uint_as_float((uint32_t)(key >> 32));
    double F = (double)m;
    if (SOFT) {
        double* __restrict__ out = resp + cell * R;
        double part = 0.0;
        for (int64_t k = lane; k < R; k += 64) {
            const double a = (double)row[k] - (double)m;
            const double w = exp(-(a / sigma));
            out[k] = w;
            part = part + w;
        }
        const double Z = wave_sum(part);
        for (int64_t k = lane; k < R; k += 64) out[k] = out[k] / Z;      // (the lane's own stores)
        F = (double)m - sigma * log(Z);
    } else if (resp) {
        double* __restrict__ out = resp + cell * R;
        for (int64_t k = lane; k < R; k += 64) out[k] = k == b ? 1.0 : 0.0;
    }
    if (lane == 0) {
        best[cell] = b;
        d2min[cell] = m;
        free_energy[cell] = F;
    }
}

// ------------------------------------------------------------------------------------------------------ per node

// part[(chunk * R + k) * (d + 1) + c]: the chunk's sum of r_ik Y_ic, c < d, and of r_ik at c = d.
template <int Q, bool HARD>
__global__ __launch_bounds__(kThreads) void ptree_sums_kernel(const float* __restrict__ Y, int64_t N, int d, int64_t ld,
                                                              const double* __restrict__ resp,
                                                              const int32_t* __restrict__ best, int64_t R,
                                                              double* __restrict__ part)
{
    const int tid = threadIdx.x, slot = tid / kSumNodes;
    const int64_t k = (int64_t)blockIdx.y * kSumNodes + (tid % kSumNodes);
    const int64_t kk = k < R ? k : R - 1;           // (a lane past R reads node R - 1 and stores nothing)
    const int64_t i0 = (int64_t)blockIdx.x * kChunk;
    const int64_t i1 = i0 + kChunk < N ? i0 + kChunk : N;
    double acc[Q], gamma = 0.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double r = HARD ? (best[i] == (int32_t)kk ? 1.0 : 0.0) : resp[i * R + kk];
        const float* __restrict__ y = Y + i * ld;
        gamma = gamma + r;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = slot + kSumSlots * q;
            const double v = c < d ? (double)y[c] : 0.0;
            acc[q] = acc[q] + r * v;
        }
    }
    if (k >= R) return;
    double* __restrict__ out = part + ((int64_t)blockIdx.x * R + k) * (d + 1);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = slot + kSumSlots * q;
        if (c < d) out[c] = acc[q];
    }
    if (slot == 0) out[d] = gamma;
}

__global__ __launch_bounds__(kThreads) void ptree_fold_kernel(const double* __restrict__ part, int64_t chunks, int64_t R,
                                                              int d, double* __restrict__ gamma, double* __restrict__ sums)
{
    const int64_t per = R * (d + 1);
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= per) return;
    double s = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) s = s + part[ch * per + j];
    const int64_t k = j / (d + 1);
    const int c = (int)(j - k * (d + 1));
    if (c == d)
        gamma[k] = s;
    else
        sums[k * d + c] = s;
}

// ------------------------------------------------------------------------------------------------------ the projection

__global__ __launch_bounds__(kThreads) void ptree_project_kernel(const float* __restrict__ Y, int64_t N, int d, int64_t ld,
                                                                 const float* __restrict__ C, int64_t R, int64_t ldc,
                                                                 const int32_t* __restrict__ edges, int64_t E,
                                                                 int32_t* __restrict__ edge, double* __restrict__ tout,
                                                                 double* __restrict__ qout, uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t cell = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (cell >= N) return;                          // (a whole wave)
    const float* __restrict__ y = Y + cell * ld;
    unsigned long long kq = ~0ull;                  // the lane's best (bits(q), e) and its t
    int ke = 0x7fffffff;
    double kt = 0.0;
    bool bad = false, range = false;
    for (int64_t e = lane; e < E; e += 64) {
        const int32_t na = edges[2 * e], nb = edges[2 * e + 1];
        if (na < 0 || na >= R || nb < 0 || nb >= R) {
            range = true;
            continue;
        }
        const float* __restrict__ ca = C + (int64_t)na * ldc;
        const float* __restrict__ cb = C + (int64_t)nb * ldc;
        double u = 0.0, l = 0.0;
        for (int c = 0; c < d; ++c) {
            const float fy = y[c], fa = ca[c], fb = cb[c];
            bad = bad || not_finite(fy) || not_finite(fa) || not_finite(fb);
            const double dy = (double)fy - (double)fa, db = (double)fb - (double)fa;
            u = u + dy * db;
            l = l + db * db;
        }
        double t = 0.0;
        if (l != 0.0) {
            t = u / l;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        }
        double q = 0.0;
        for (int c = 0; c < d; ++c) {
            const double dy = (double)y[c] - (double)ca[c], db = (double)cb[c] - (double)ca[c];
            const double r = dy - t * db;
            q = q + r * r;
        }
        const unsigned long long bits = (unsigned long long)__double_as_longlong(q);
        if (bits < kq) {                            // (ascending e within the lane: an equal q keeps the lower edge)
            kq = bits;
            ke = (int)e;
            kt = t;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long oq = __shfl_xor(kq, off, 64);
        const int oe = __shfl_xor(ke, off, 64);
        const double ot = __shfl_xor(kt, off, 64);
        if (oq < kq || (oq == kq && oe < ke)) {
            kq = oq;
            ke = oe;
            kt = ot;
        }
    }
    if (lane == 0) {
        const bool none = ke == 0x7fffffff;         // every edge was out of range
        edge[cell] = none ? 0 : ke;
        tout[cell] = kt;
        qout[cell] = none ? 0.0 : __longlong_as_double((long long)kq);
    }
    if (bad) atomicOr(status, PROSSTT_AMD_PTREE_NONFINITE);
    if (range && cell == 0) atomicOr(status, PROSSTT_AMD_PTREE_EDGE_RANGE);
}

// ------------------------------------------------------------------------------------------------------ the host

int check_sizes(int64_t N, int64_t d, int64_t R)
{
    if (cells_out_of_range(N)) return fail(ABI_EINVAL, "need 1 <= N < 2^31 (got %lld)", (long long)N);
    if (d < 1 || d > kMaxDim) return fail(ABI_EINVAL, "need 1 <= d <= %d (got %lld)", kMaxDim, (long long)d);
    if (R < 1 || R > PROSSTT_AMD_PTREE_MAX_NODES)
        return fail(ABI_EINVAL, "need 1 <= R <= %d nodes (got %lld)", PROSSTT_AMD_PTREE_MAX_NODES, (long long)R);
    return 0;
}

int check_panels(const float* Y, int64_t d, int64_t ld, const float* C, int64_t ldc)
{
    if (ld < d) return stride_below_row(ld, d);
    if (ldc < d) return fail(ABI_EINVAL, "centre stride %lld is below the row length %lld", (long long)ldc, (long long)d);
    if (!Y || !C) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)Y % 4 != 0 || (uintptr_t)C % 4 != 0) return fail(ABI_EINVAL, "Y and C must be 4-byte aligned");
    return 0;
}

struct Workspace {
    size_t distances, resp, partials, total;
};

Workspace layout(int64_t N, int64_t d, int64_t R, bool soft)
{
    Workspace w;
    w.distances = pad((size_t)N * (size_t)R * 4);
    w.resp = soft ? pad((size_t)N * (size_t)R * 8) : 0;
    w.partials = pad((size_t)cdiv(N, kChunk) * (size_t)R * (size_t)(d + 1) * 8);
    w.total = w.distances + w.resp + w.partials;
    return w;
}

template <bool HARD>
void launch_sums(hipStream_t st, const float* Y, int64_t N, int d, int64_t ld, const double* resp, const int32_t* best,
                 int64_t R, double* part)
{
    const dim3 grid((unsigned)cdiv(N, kChunk), (unsigned)cdiv(R, kSumNodes)), block(kThreads);
    const int q = (int)cdiv(d, kSumSlots);
    if (q <= 1)
        ptree_sums_kernel<1, HARD><<<grid, block, 0, st>>>(Y, N, d, ld, resp, best, R, part);
    else if (q <= 2)
        ptree_sums_kernel<2, HARD><<<grid, block, 0, st>>>(Y, N, d, ld, resp, best, R, part);
    else if (q <= 4)
        ptree_sums_kernel<4, HARD><<<grid, block, 0, st>>>(Y, N, d, ld, resp, best, R, part);
    else if (q <= 8)
        ptree_sums_kernel<8, HARD><<<grid, block, 0, st>>>(Y, N, d, ld, resp, best, R, part);
    else
        ptree_sums_kernel<16, HARD><<<grid, block, 0, st>>>(Y, N, d, ld, resp, best, R, part);
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_ptree_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_ptree_workspace_bytes(int64_t N, int64_t d, int64_t R, int32_t soft, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, d, R)) return rc;
    *bytes = layout(N, d, R, soft != 0).total;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_ptree_assign(void* stream, const float* Y, int64_t N, int64_t d, int64_t ld, const float* C,
                                        int64_t R, int64_t ldc, double sigma, void* ws, uint64_t ws_bytes, int32_t* best,
                                        float* d2min, double* free_energy, double* gamma, double* sums, double* resp,
                                        uint32_t* status) try
{
    if (int rc = check_sizes(N, d, R)) return rc;
    if (int rc = check_panels(Y, d, ld, C, ldc)) return rc;
    if (!(sigma >= 0.0) || !(sigma < __builtin_inf()))
        return fail(ABI_EINVAL, "need sigma >= 0 and finite (got %g)", sigma);
    if (!ws || !best || !d2min || !free_energy || !gamma || !sums || !status) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)best % 4 != 0 || (uintptr_t)d2min % 4 != 0 || (uintptr_t)status % 4 != 0)
        return fail(ABI_EINVAL, "best, d2min and status must be 4-byte aligned");
    if ((uintptr_t)free_energy % 8 != 0 || (uintptr_t)gamma % 8 != 0 || (uintptr_t)sums % 8 != 0 || (uintptr_t)resp % 8 != 0)
        return fail(ABI_EINVAL, "free_energy, gamma, sums and resp must be 8-byte aligned");
    if ((uintptr_t)ws % 16 != 0) return fail(ABI_EINVAL, "the workspace is not 16-byte aligned");
    const bool soft = sigma > 0.0;
    const Workspace w = layout(N, d, R, soft);
    if (ws_bytes < w.total) return workspace_too_small(ws_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    float* D = (float*)ws;
    double* r = resp ? resp : (soft ? (double*)((char*)ws + w.distances) : nullptr);
    double* part = (double*)((char*)ws + w.distances + w.resp);
    ptree_distance_kernel<<<dim3((unsigned)cdiv(N, kBlockCells), (unsigned)cdiv(R, kTile)), dim3(kThreads), 0, st>>>(
        Y, N, (int)d, ld, C, R, ldc, D, status);
    HIP_TRY(hipGetLastError());
    const dim3 cells((unsigned)cdiv(N, kWaves));
    if (soft) {
        ptree_cell_kernel<true><<<cells, dim3(kThreads), 0, st>>>(D, N, R, sigma, best, d2min, free_energy, r);
        HIP_TRY(hipGetLastError());
        launch_sums<false>(st, Y, N, (int)d, ld, r, best, R, part);
    } else {
        ptree_cell_kernel<false><<<cells, dim3(kThreads), 0, st>>>(D, N, R, sigma, best, d2min, free_energy, r);
        HIP_TRY(hipGetLastError());
        launch_sums<true>(st, Y, N, (int)d, ld, r, best, R, part);
    }
    HIP_TRY(hipGetLastError());
    ptree_fold_kernel<<<dim3((unsigned)cdiv(R * (d + 1), kThreads)), dim3(kThreads), 0, st>>>(part, cdiv(N, kChunk), R, (int)d,
                                                                                             gamma, sums);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_ptree_project(void* stream, const float* Y, int64_t N, int64_t d, int64_t ld, const float* C,
                                         int64_t R, int64_t ldc, const int32_t* edges, int64_t E, int32_t* edge, double* t,
                                         double* q, uint32_t* status) try
{
    if (int rc = check_sizes(N, d, R)) return rc;
    if (int rc = check_panels(Y, d, ld, C, ldc)) return rc;
    if (E < 1 || E > PROSSTT_AMD_PTREE_MAX_EDGES)
        return fail(ABI_EINVAL, "need 1 <= E <= %d edges (got %lld)", PROSSTT_AMD_PTREE_MAX_EDGES, (long long)E);
    if (!edges || !edge || !t || !q || !status) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)edges % 4 != 0 || (uintptr_t)edge % 4 != 0 || (uintptr_t)status % 4 != 0)
        return fail(ABI_EINVAL, "edges, edge and status must be 4-byte aligned");
    if ((uintptr_t)t % 8 != 0 || (uintptr_t)q % 8 != 0) return fail(ABI_EINVAL, "t and q must be 8-byte aligned");
    ptree_project_kernel<<<dim3((unsigned)cdiv(N, kWaves)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        Y, N, (int)d, ld, C, R, ldc, edges, E, edge, t, q, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
