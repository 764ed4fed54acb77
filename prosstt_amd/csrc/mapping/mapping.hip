// libprosstt_amd_mapping.so -- the score of every cell at every node of a lineage tree (include/prosstt_amd_mapping.h).
//
// Kernels (the definition is in the header)
//   mapping_pass_kernel<NT, VEC>  a matrix-core product (mfma_device.h: the operand mapping, the lane's 16 counts of a step,
//                                 the k-steps and the tile map) of the counts, converted in registers, with a node-major
//                                 panel: a block owns 128 rows (32 per wave) and 32 NT nodes and loops over all genes; the
//                                 32 x 32 NT panel slice of a step is read along the genes and staged transposed in LDS; at
//                                 a chain's end the binary32 accumulators are added into binary64 registers and cleared;
//                                 the epilogue stores S = (D - s m) + c
//   mapping_finish_kernel         one wave per row of S: argmax, log-sum-exp, log-sum-exp of every branch
// There is no floating-point atomic and every sum has a fixed order: equal inputs give equal bits.
#include "../../../include/prosstt_amd_mapping.h"

#define ABI_EINVAL PROSSTT_AMD_MAPPING_EINVAL
#define ABI_EHIP PROSSTT_AMD_MAPPING_EHIP
#include "../abi_util.h"
#include "../mfma_device.h"               // f32x16, kStep, load_row16, mfma, tile_row, with_instantiation
#include "../wave_reduce.h"               // wave_sum: the butterfly of the log-sum-exp

namespace {

constexpr int kRows = 128;                  // rows per block of the pass, 32 per wave
constexpr int kFinishRows = kThreads / 64;  // rows per block of the finish kernel, one per wave
constexpr int64_t kMaxNodes = PROSSTT_AMD_MAPPING_MAX_NODES;

// ------------------------------------------------------------------------------------------------------ the pass

// The thread's share of the panel slice of a step: element idx = tid + 256 q is node n0 + idx / 32, gene g0 + idx % 32 (a
// wave reads 128 consecutive bytes of two nodes); zeros past R and past G.
template <int NT>
__device__ __forceinline__ void load_panel(float (&p)[NT * 4], const float* __restrict__ P, int64_t ldp, int64_t R,
                                           int64_t G, int64_t n0, int64_t g0, int tid)
{
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) {
        const int idx = tid + q * kThreads;
        const int64_t node = n0 + (idx >> 5), g = g0 + (idx & 31);
        p[q] = (node < R && g < G) ? P[node * ldp + g] : 0.0f;
    }
}

// ... stored transposed: gene k of the step, node j of the tile at sh[k * LS + j].
template <int NT>
__device__ __forceinline__ void stage_panel(float* sh, const float (&p)[NT * 4], int tid)
{
    constexpr int LS = slice_stride(NT);
#pragma unroll
    for (int q = 0; q < NT * 4; ++q) {
        const int idx = tid + q * kThreads;
        sh[(idx & 31) * LS + (idx >> 5)] = p[q];
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(kThreads) void mapping_pass_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                int64_t ld, const double* __restrict__ size,
                                                                const float* __restrict__ P, int64_t ldp, int64_t R,
                                                                const double* __restrict__ exposure,
                                                                const double* __restrict__ constant, int steps_per_chain,
                                                                double* __restrict__ S, uint32_t* __restrict__ status)
{
    constexpr int LP = NT * 32;
    __shared__ float psh[kStep * slice_stride(NT)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int64_t rbase = (int64_t)blockIdx.x * kRows + wave * 32;
    const int64_t r = rbase + c;
    const bool row_ok = r < N;
    const int32_t* __restrict__ rp = X + (row_ok ? r : 0) * ld;
    const int64_t n0 = (int64_t)blockIdx.y * LP;

    f32x16 acc[NT];
    double sum[NT][16];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        acc[t] = f32x16{};
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) sum[t][reg] = 0.0;
    }
    int32_t x[16];
    float pp[NT * 4];
    int32_t neg = 0;
    int left = steps_per_chain;                     // steps until the chain ends
    load_row16<VEC>(x, rp, row_ok, 0, G, h);
    load_panel<NT>(pp, P, ldp, R, G, n0, 0, tid);
    for (int64_t g0 = 0; g0 < G; g0 += kStep) {
        float a[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            neg |= x[q];
            a[q] = (float)x[q];
        }
        stage_panel<NT>(psh, pp, tid);
        __syncthreads();
        if (g0 + kStep < G) {                       // the next step's loads fly during this step's products
            load_row16<VEC>(x, rp, row_ok, g0 + kStep, G, h);
            load_panel<NT>(pp, P, ldp, R, G, n0, g0 + kStep, tid);
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) {              // (mfma_device.h's mfma_steps, written out: as a call it changed this loop)
            const float* b = psh + (16 * h + s) * slice_stride(NT) + c;
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma(a[s], b[32 * t], acc[t]);
        }
        if (--left == 0 || g0 + kStep >= G) {       // the chain ends: its sums join the binary64 sums
            left = steps_per_chain;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) sum[t][reg] += (double)acc[t][reg];
                acc[t] = f32x16{};
            }
        }
        __syncthreads();
    }
    if (neg < 0) atomicOr(status, PROSSTT_AMD_MAPPING_NEGATIVE);
    double mt[NT], ct[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int64_t node = n0 + 32 * t + c;
        mt[t] = node < R ? exposure[node] : 0.0;
        ct[t] = node < R ? constant[node] : 0.0;
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t row = rbase + tile_row(reg, h);
        if (row < N) {
            const double si = size[row];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int64_t node = n0 + 32 * t + c;
                if (node < R) S[row * R + node] = (sum[t][reg] - si * mt[t]) + ct[t];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the finish

// The better of two candidates (value, node): a node of -1 is no candidate; the larger value, of equal values the lower node.
__device__ __forceinline__ void take_better(double& v, int& i, double ov, int oi)
{
    if (oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i))) {
        v = ov;
        i = oi;
    }
}

// log(sum exp(row[r] - top)) + top over the nodes [lo, hi): lane k adds the nodes lo + k, lo + k + 64, ... in ascending order.
__device__ __forceinline__ double log_sum_exp(const double* __restrict__ row, int64_t lo, int64_t hi, double top, int lane)
{
    double part = 0.0;
    for (int64_t r = lo + lane; r < hi; r += 64) part += exp(row[r] - top);
    return log(wave_sum(part)) + top;
}

__global__ __launch_bounds__(kThreads) void mapping_finish_kernel(const double* __restrict__ S, int64_t N, int64_t R,
                                                                  const int64_t* __restrict__ offsets, int64_t B,
                                                                  int32_t* __restrict__ best, double* __restrict__ best_score,
                                                                  double* __restrict__ lse, double* __restrict__ branch_lse,
                                                                  uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63;
    const int64_t cell = (int64_t)blockIdx.x * kFinishRows + (threadIdx.x >> 6);
    if (cell >= N) return;                          // (a whole wave: the shuffles below are among the lanes of one row)
    const double* __restrict__ row = S + cell * R;
    double v = 0.0;
    int i = -1;
    for (int64_t r = lane; r < R; r += 64) {
        const double sv = row[r];
        if (sv == sv) take_better(v, i, sv, (int)r);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        take_better(v, i, ov, oi);
    }
    const double top = i < 0 ? __builtin_nan("") : v;
    const double total = log_sum_exp(row, 0, R, top, lane);
    if (lane == 0) {
        best[cell] = i < 0 ? 0 : i;
        best_score[cell] = top;
        lse[cell] = total;
    }
    if (!branch_lse) return;
    uint32_t flags = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t from = offsets[b], to = offsets[b + 1];
        if (from < 0 || to < from || to > R || (b == 0 && from != 0) || (b == B - 1 && to != R))
            flags = PROSSTT_AMD_MAPPING_BRANCH_RANGE;
        const int64_t lo = from < 0 ? 0 : (from > R ? R : from);
        const int64_t hi = to < lo ? lo : (to > R ? R : to);
        double high = -__builtin_inf();
        for (int64_t r = lo + lane; r < hi; r += 64) high = fmax(high, row[r]);         // (fmax skips a NaN)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) high = fmax(high, __shfl_xor(high, off, 64));
        const double out = high == -__builtin_inf() ? high : log_sum_exp(row, lo, hi, high, lane);
        if (lane == 0) branch_lse[cell * B + b] = out;
    }
    if (flags && cell == 0 && lane == 0) atomicOr(status, flags);
}

// ------------------------------------------------------------------------------------------------------ the host

int check_sizes(int64_t N, int64_t G, int64_t R)
{
    if (cells_out_of_range(N)) return fail(ABI_EINVAL, "need 1 <= N < 2^31 (got %lld)", (long long)N);
    if (G < 1 || G >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 1 <= G < 2^31 (got %lld)", (long long)G);
    if (R < 1 || R > kMaxNodes)                     // (the node tiles are the grid's y, a tile holds at least 32 nodes)
        return fail(ABI_EINVAL, "need 1 <= R <= %lld nodes (got %lld)", (long long)kMaxNodes, (long long)R);
    return 0;
}

size_t scores_bytes(int64_t N, int64_t R) { return pad((size_t)N * (size_t)R * 8); }

}  // namespace

ABI_EXPORT const char* prosstt_amd_mapping_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_mapping_workspace_bytes(int64_t N, int64_t G, int64_t R, int64_t B, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, R)) return rc;
    if (B < 0 || B >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 0 <= B < 2^31 branches (got %lld)", (long long)B);
    *bytes = scores_bytes(N, R);
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_mapping_node_scores_tiled(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                                     const double* s, const float* P, int64_t ldp, int64_t R,
                                                     const double* m, const double* c, const int64_t* branch_offsets,
                                                     int64_t B, int64_t genes_per_chain, int32_t node_tile, void* ws,
                                                     uint64_t ws_bytes, int32_t* best, double* best_score, double* lse,
                                                     double* branch_lse, double* scores, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, R)) return rc;
    if (ld < G) return stride_below_row(ld, G);
    if (ldp < G) return fail(ABI_EINVAL, "panel stride %lld is below the row length %lld", (long long)ldp, (long long)G);
    if (genes_per_chain < 32 || genes_per_chain > PROSSTT_AMD_MAPPING_MAX_CHAIN || genes_per_chain % 32 != 0)
        return fail(ABI_EINVAL, "need genes_per_chain a multiple of 32 in 32 .. %d (got %lld)", PROSSTT_AMD_MAPPING_MAX_CHAIN,
                    (long long)genes_per_chain);
    if (node_tile < 0 || node_tile > 4) return fail(ABI_EINVAL, "need 0 <= node_tile <= 4 (got %d)", (int)node_tile);
    if (!X || !s || !P || !m || !c || !ws || !best || !best_score || !lse || !status || (branch_lse && !branch_offsets))
        return fail(ABI_EINVAL, "NULL argument");
    if (branch_lse && (B < 1 || B >= (int64_t(1) << 31)))
        return fail(ABI_EINVAL, "need 1 <= B < 2^31 branches (got %lld)", (long long)B);
    if ((uintptr_t)s % 8 != 0 || (uintptr_t)m % 8 != 0 || (uintptr_t)c % 8 != 0 || (uintptr_t)branch_offsets % 8 != 0 ||
        (uintptr_t)best_score % 8 != 0 || (uintptr_t)lse % 8 != 0 || (uintptr_t)branch_lse % 8 != 0 ||
        (uintptr_t)scores % 8 != 0)
        return fail(ABI_EINVAL, "s, m, c, branch_offsets, best_score, lse, branch_lse and scores must be 8-byte aligned");
    if ((uintptr_t)P % 4 != 0 || (uintptr_t)best % 4 != 0) return fail(ABI_EINVAL, "P and best must be 4-byte aligned");
    if ((uintptr_t)ws % 16 != 0) return fail(ABI_EINVAL, "the workspace is not 16-byte aligned");
    if (ws_bytes < scores_bytes(N, R)) return workspace_too_small(ws_bytes, scores_bytes(N, R));
    hipStream_t st = (hipStream_t)stream;
    double* S = scores ? scores : (double*)ws;
    // (two tiles: 240 vector registers, two waves per SIMD; three and four leave one wave per SIMD and lose: 10.6 ms against
    // 13.1 and 15.3 at 50 000 x 20 000 x 400)
    const int nt = node_tile ? node_tile : (int)clamp64(cdiv(R, 32), 1, 2);
    const int steps = (int)(genes_per_chain / kStep);
    with_instantiation(nt, aligned(X, ld, 4), [&](auto tiles, auto vec) {
        const dim3 grid((unsigned)cdiv(N, kRows), (unsigned)cdiv(R, 32 * tiles()));
        mapping_pass_kernel<tiles(), vec()><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, s, P, ldp, R, m, c, steps, S, status);
    });
    HIP_TRY(hipGetLastError());
    mapping_finish_kernel<<<dim3((unsigned)cdiv(N, kFinishRows)), dim3(kThreads), 0, st>>>(
        S, N, R, branch_offsets, B, best, best_score, lse, branch_lse, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_mapping_node_scores(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                               const double* s, const float* P, int64_t ldp, int64_t R, const double* m,
                                               const double* c, const int64_t* branch_offsets, int64_t B,
                                               int64_t genes_per_chain, void* ws, uint64_t ws_bytes, int32_t* best,
                                               double* best_score, double* lse, double* branch_lse, double* scores,
                                               uint32_t* status)
{
    return prosstt_amd_mapping_node_scores_tiled(stream, X, N, G, ld, s, P, ldp, R, m, c, branch_offsets, B, genes_per_chain,
                                                 0, ws, ws_bytes, best, best_score, lse, branch_lse, scores, status);
}
