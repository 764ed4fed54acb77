// libprosstt_amd_layout.so -- the epochs of a UMAP layout of the connectivity graph in their synchronous form
// (include/prosstt_amd_layout.h has the definition).  256 threads = 4 waves per block, 64-bit offsets, no scratch, no
// floating-point atomic: a sum is a lane's own ascending partial sum followed by a fixed xor shuffle tree.
//   layout_epoch_kernel<C, G>  one epoch, C coordinates, G lanes per row (4, 16, 64).  The row's items (entry x (1 + rate):
//                              slot 0 the attraction, slot s + 1 the negative sample s) are dealt round-robin, lane l taking
//                              items l, l + G, ..: an active entry's 1 + rate pair evaluations, a powf each, spread over
//                              1 + rate lanes instead of serialising in one, and consecutive lanes read the same p[e].
//                              Reads Y^n, writes Y^(n+1): the launch boundary is the epoch's barrier.
//   layout_negatives_kernel    the probe of the hash: k of (entry, sample) for a range of entries.
#include "../../../include/prosstt_amd_layout.h"

#define ABI_EINVAL PROSSTT_AMD_LAYOUT_EINVAL
#define ABI_EHIP PROSSTT_AMD_LAYOUT_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // check_csr, check_cells, stride_blocks
#include "../wave_reduce.h"               // group_sum, wave_sum, wave_min

#include <cmath>

namespace {

constexpr int kMaxEpochs = 4096;
constexpr int kMaxRate = 31;
#ifndef LAYOUT_UNROLL
#define LAYOUT_UNROLL 4
#endif
constexpr int kUnroll = LAYOUT_UNROLL;               // items of a lane in flight together (any value gives the same bits)

struct EpochParams {
    double n;           // the epoch, for the schedule's binary64 products
    uint64_t base;      // base_n of the hash
    float a, b, m2ab, g2b, alpha;
    int rate;
};

__host__ __device__ __forceinline__ uint64_t mix(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

inline uint64_t epoch_base(uint64_t seed, int epoch) { return mix(seed + 0x9E3779B97F4A7C15ull * (uint64_t)(epoch + 1)); }

// k of the definition: below N because (h >> 32) < 2^32
__device__ __forceinline__ int64_t negative_index(uint64_t base, uint64_t e, int s, int64_t N)
{
    const uint64_t h = mix(base ^ (32ull * e + (uint64_t)s));
    return (int64_t)(((h >> 32) * (uint64_t)N) >> 32);
}

template <int C, int G>
__global__ __launch_bounds__(kThreads) void layout_epoch_kernel(const int64_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ indices,
                                                                const double* __restrict__ p, const float* __restrict__ y0,
                                                                float* __restrict__ y1, int64_t N, EpochParams P)
{
    const int64_t row = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    const int sub = threadIdx.x % G;
    const bool ok = row < N;
    const int64_t begin = ok ? indptr[row] : 0, len = ok ? indptr[row + 1] - begin : 0;
    const int R = P.rate + 1;                         // items per entry
    float yi[C], acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        yi[c] = ok ? y0[row * C + c] : 0.0f;
        acc[c] = 0.0f;
    }
    // item t = sub, sub + G, ..: (q, slot) = (t / R, t % R), stepped without a division.  kUnroll items go through each
    // stage together, so that their loads of p, of the column and of the other end's position are in flight at once; a
    // lane still adds its terms in ascending item order (an item that yields no term adds +0, which changes no bit).
    int64_t q = sub / R;
    int slot = sub % R;
    const int dq = G / R, dslot = G % R;
    while (q < len) {
        int64_t e[kUnroll], j[kUnroll];
        int slots[kUnroll];
        bool live[kUnroll];
        double pe[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            live[u] = q < len;
            e[u] = begin + (live[u] ? q : 0);         // (a lane past its last item re-reads the row's first entry)
            slots[u] = slot;
            q += dq;
            slot += dslot;
            if (slot >= R) {
                slot -= R;
                ++q;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) pe[u] = p[e[u]];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            live[u] = live[u] && floor((P.n + 1.0) * pe[u]) > floor(P.n * pe[u]);
            j[u] = row;
            if (live[u]) j[u] = slots[u] == 0 ? (int64_t)indices[e[u]] : negative_index(P.base, (uint64_t)e[u], slots[u] - 1, N);
            live[u] = live[u] && (slots[u] == 0 || j[u] != row);
        }
        float other[kUnroll][C];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
            for (int c = 0; c < C; ++c) other[u][c] = y0[j[u] * C + c];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            float delta[C], d2 = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                delta[c] = yi[c] - other[u][c];
                d2 += delta[c] * delta[c];
            }
            float coef = 0.0f;
            if (live[u] && d2 > 0.0f) {
                const float pb = powf(d2, P.b);
                const float den = P.a * pb + 1.0f;
                coef = slots[u] == 0 ? (P.m2ab * (pb / d2)) / den : P.g2b / ((0.001f + d2) * den);
            }
            const float twice = slots[u] == 0 ? 2.0f : 1.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += live[u] ? twice * fminf(fmaxf(coef * delta[c], -4.0f), 4.0f) : 0.0f;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float sum = group_sum<G>(acc[c]);
        if (ok && sub == 0) y1[row * C + c] = yi[c] + P.alpha * sum;
    }
}

__global__ __launch_bounds__(kThreads) void layout_negatives_kernel(uint64_t base, int64_t e_begin, int64_t items, int rate,
                                                                    int64_t N, int32_t* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < items; t += stride)
        out[t] = (int32_t)negative_index(base, (uint64_t)(e_begin + t / rate), (int)(t % rate), N);
}

int choose_lanes(int64_t N, int64_t nnz, int rate)
{
    // measured at 50 000 rows: 64 lanes win at 141 items per mean row (2.1 x against 16 lanes) and still
    // at 24 (1.1 x), since the hub rows end an epoch; below 16 items per mean row, where three quarters of a 64-lane
    // group would idle on the mean row, 16 lanes stay the choice by that reasoning alone (not measured)
    return (nnz / N) * (rate + 1) < 16 ? 16 : 64;
}

template <int C, int G>
void launch_epoch(hipStream_t st, const int64_t* indptr, const int32_t* indices, const double* p, const float* src, float* dst,
                  int64_t N, const EpochParams& P)
{
    layout_epoch_kernel<C, G><<<dim3((unsigned)cdiv(N, kThreads / G)), dim3(kThreads), 0, st>>>(indptr, indices, p, src, dst,
                                                                                                 N, P);
}

template <int C>
bool launch_epoch_lanes(int g, hipStream_t st, const int64_t* indptr, const int32_t* indices, const double* p, const float* src,
                        float* dst, int64_t N, const EpochParams& P)
{
    switch (g) {
    case 4: launch_epoch<C, 4>(st, indptr, indices, p, src, dst, N, P); return true;
    case 16: launch_epoch<C, 16>(st, indptr, indices, p, src, dst, N, P); return true;
    case 64: launch_epoch<C, 64>(st, indptr, indices, p, src, dst, N, P); return true;
    default: return false;
    }
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_layout_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_layout_epochs(void* stream, const int64_t* indptr, const int32_t* indices, const double* p, int64_t N,
                                         int64_t nnz, int32_t c, float* y0, float* y1, int32_t epoch_begin, int32_t epoch_end,
                                         int32_t n_epochs, double a, double b, double gamma, double alpha0,
                                         int32_t negative_sample_rate, uint64_t seed, int32_t lanes_per_row) try
{
    if (int rc = check_csr(N, nnz, c)) return rc;
    if (n_epochs < 1 || n_epochs > kMaxEpochs) return fail(ABI_EINVAL, "need 1 <= n_epochs <= %d (got %d)", kMaxEpochs, (int)n_epochs);
    if (epoch_begin < 0 || epoch_begin > epoch_end || epoch_end > n_epochs)
        return fail(ABI_EINVAL, "need 0 <= epoch_begin <= epoch_end <= n_epochs (got %d, %d, %d)", (int)epoch_begin,
                    (int)epoch_end, (int)n_epochs);
    if (negative_sample_rate < 0 || negative_sample_rate > kMaxRate)
        return fail(ABI_EINVAL, "need 0 <= negative_sample_rate <= %d (got %d)", kMaxRate, (int)negative_sample_rate);
    if (!(a > 0.0) || !(b > 0.0) || !(gamma >= 0.0) || !(alpha0 > 0.0) || !std::isfinite(a) || !std::isfinite(b) ||
        !std::isfinite(gamma) || !std::isfinite(alpha0))
        return fail(ABI_EINVAL, "need finite a > 0, b > 0, gamma >= 0, alpha0 > 0 (got %g, %g, %g, %g)", a, b, gamma, alpha0);
    if (lanes_per_row != 0 && lanes_per_row != 4 && lanes_per_row != 16 && lanes_per_row != 64)
        return fail(ABI_EINVAL, "lanes_per_row must be 0, 4, 16 or 64 (got %d)", (int)lanes_per_row);
    if (!indptr || !indices || !p || !y0 || !y1) return fail(ABI_EINVAL, "NULL argument");
    if (y0 == y1) return fail(ABI_EINVAL, "y1 must not alias y0");
    const int g = lanes_per_row ? lanes_per_row : choose_lanes(N, nnz, negative_sample_rate);
    hipStream_t st = (hipStream_t)stream;
    EpochParams P;
    P.a = (float)a;
    P.b = (float)b;
    const float gamma32 = (float)gamma;
    P.m2ab = (float)(-2.0 * (double)P.a * (double)P.b);
    P.g2b = (float)(2.0 * (double)gamma32 * (double)P.b);
    P.rate = negative_sample_rate;
    const float* src = y0;
    float* dst = y1;
    for (int n = epoch_begin; n < epoch_end; ++n) {
        P.n = (double)n;
        P.base = epoch_base(seed, n);
        P.alpha = (float)(alpha0 * (1.0 - (double)n / (double)n_epochs));
        if (c == 2) launch_epoch_lanes<2>(g, st, indptr, indices, p, src, dst, N, P);
        else launch_epoch_lanes<3>(g, st, indptr, indices, p, src, dst, N, P);
        HIP_TRY(hipGetLastError());
        float* was = const_cast<float*>(src);
        src = dst;
        dst = was;
    }
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_layout_negatives(void* stream, uint64_t seed, int32_t epoch, int64_t e_begin, int64_t count,
                                            int32_t rate, int64_t N, int32_t* out) try
{
    if (int rc = check_cells(N)) return rc;
    if (epoch < 0 || epoch >= kMaxEpochs) return fail(ABI_EINVAL, "need 0 <= epoch < %d (got %d)", kMaxEpochs, (int)epoch);
    if (rate < 0 || rate > kMaxRate) return fail(ABI_EINVAL, "need 0 <= rate <= %d (got %d)", kMaxRate, (int)rate);
    if (e_begin < 0 || count < 0 || count > (int64_t(1) << 40) || e_begin > (int64_t(1) << 62))
        return fail(ABI_EINVAL, "need 0 <= e_begin <= 2^62 and 0 <= count <= 2^40 (got %lld, %lld)", (long long)e_begin,
                    (long long)count);
    if (!out) return fail(ABI_EINVAL, "NULL argument");
    const int64_t items = count * rate;
    if (items == 0) return 0;
    layout_negatives_kernel<<<dim3(stride_blocks(items)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        epoch_base(seed, epoch), e_begin, items, rate, N, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
