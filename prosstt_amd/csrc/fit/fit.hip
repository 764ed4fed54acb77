// libprosstt_amd_fit.so -- the count model's log-likelihood over a device count matrix for several candidate parameter
// pairs per gene (include/prosstt_amd_fit.h holds the definition; DESIGN section 22 the reasons).
//
// Kernels (256 threads = 4 waves each)
//   fit_loglik_kernel   a column kernel (column_device.h: a block owns a strip of 256 genes and a range of rows, a lane ONE
//                       gene; <true> stages tiles of 8 rows through LDS in 16-byte loads, <false> and the last, partial
//                       strip take 4-byte loads), here with up to kCand = 4 of the C candidates per block (blockIdx.z).
//                       The lane's candidates' (a, b - 1) and their sums stay in registers across the rows, and the term's
//                       code is there four times, not sixteen (what four genes per lane, count_summary's strip, times four
//                       candidates would make of the loop).
//                       The row's label and size factor are uniform over the block: scalar loads.  The row of means is
//                       loaded again only when the label differs from the previous row's (cells sorted by label, a
//                       device.PresentedCounts, load it once per run).  Per entry mu, the x = 0 test and lgamma(x + 1)
//                       are formed once; the lanes of a wave diverge between x = 0 (-(r L1) alone), 1 <= x <= 12 (one
//                       more log1p, a product and its log) and x > 12 (the Stirling form): the union of the paths a
//                       wave needs is what it executes.
//   fit_finish_kernel   adds the blocks' partial sums in ascending block order
// No atomics but the OR of a status bit.
#include "../../../include/prosstt_amd_fit.h"

#define ABI_EINVAL PROSSTT_AMD_FIT_EINVAL
#define ABI_EHIP PROSSTT_AMD_FIT_EHIP
#include "../abi_util.h"
#include "../column_device.h"

namespace {

constexpr int kCand = 4;                    // candidates per block
constexpr int kMaxC = PROSSTT_AMD_FIT_MAX_CANDIDATES;
constexpr double kLargest = 1e150;         // the largest size factor and the largest mean: their product cannot overflow

struct Geometry {
    int64_t strips = 0, row_blocks = 0, rows_per_block = 0, chunks = 0;
    size_t ll = 0, base = 0, bad = 0;       // offsets of the slabs [row_blocks][C][G], [row_blocks][G], [row_blocks][G]
    size_t bytes = 0;
};

// The blocking of the rows depends on (N, strips) alone, never on C.
Geometry geometry(int64_t N, int64_t G, int64_t C)
{
    Geometry g;
    g.strips = cdiv(G, kColumn);
    g.chunks = cdiv(C, kCand);
    const RowBlocking b = row_blocking(N, g.strips);
    g.rows_per_block = b.rows_per_block;
    g.row_blocks = b.row_blocks;
    const size_t cells = (size_t)g.row_blocks * (size_t)G;
    g.ll = 0;
    g.base = g.ll + pad(cells * (size_t)C * 8);
    g.bad = g.base + pad(cells * 8);
    g.bytes = g.bad + pad(cells * 4);
    return g;
}

// S(t) of the header: the Stirling series of lgamma(t) - ((t - 1/2) log t - t + log(2 pi) / 2), five terms (t >= 13: the
// sixth is below 1.1e-15).
__device__ __forceinline__ double stirling(double t)
{
    const double u = 1.0 / t;
    const double u2 = u * u;
    double s = 1.0 / 1680.0 - u2 * (1.0 / 1188.0);
    s = 1.0 / 1260.0 - u2 * s;
    s = 1.0 / 360.0 - u2 * s;
    s = 1.0 / 12.0 - u2 * s;
    return u * s;
}

// lgd(r, x) = lgamma(r + x) - lgamma(r) for r > 0, x >= 1, by the header's two forms.
__device__ __forceinline__ double lgd(double r, int32_t x)
{
    if (x <= 12) {
        if (r > 1e17) return (double)x * log(r);
        double p = r;
        for (int32_t j = 1; j < x; ++j) p *= r + (double)j;
        return log(p);
    }
    // 0 .. 16 by construction: r > 0 for the admissible parameters the kernel computes with, and whatever else r may be
    // (a NaN: fmax returns its other argument) the clamp leaves the value inside the range before the conversion
    const int32_t k = (int32_t)__builtin_ceil(__builtin_fmin(__builtin_fmax(16.0 - r, 0.0), 16.0));
    double p = 1.0;
    for (int32_t j = 0; j < k; ++j) p *= r + (double)j;
    const double z = r + (double)k;
    const double n = (double)(x - k);                                       // (>= -3: t = z + n >= 13 either way)
    const double t = z + n;
    const double main = n * log(t) + ((z - 0.5) * log1p(n / z) - n);
    return (main + (stirling(t) - stirling(z))) + log(p);
}

// The term of one entry with x >= 0 and mu > 0 for the candidate (a, bm1 = b - 1).
__device__ __forceinline__ double term(double mu, int32_t x, double a, double bm1)
{
    const double theta = a * mu + bm1;
    const double inv = 1.0 / theta;
    const double r = mu * inv;
    const double rl = r * log1p(theta);
    if (x == 0) return -rl;
    return (lgd(r, x) - rl) + (double)x * -log1p(inv);
}

// Finite with a >= 0, b >= 1 and a + (b - 1) > 0 (false for a NaN).
__device__ __forceinline__ bool admissible(double a, double b) { return column_admissible(a, b) && a + (b - 1.0) > 0.0; }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void fit_loglik_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G, int64_t ld,
                                                              const double* __restrict__ size,
                                                              const int32_t* __restrict__ labels, int32_t K,
                                                              const double* __restrict__ means, int64_t ldm,
                                                              const double* __restrict__ alpha,
                                                              const double* __restrict__ beta, int64_t C,
                                                              int64_t rows_per_block, double* __restrict__ llslab,
                                                              double* __restrict__ baseslab, uint32_t* __restrict__ badslab,
                                                              uint32_t* __restrict__ status)
{
    __shared__ int32_t tile[VEC ? kColumnTile : 1][kColumn];
    const ColumnLane lane = column_lane<VEC>(N, G, rows_per_block);
    const int64_t g = lane.g;
    const bool mine = lane.mine;
    const int64_t c0 = (int64_t)blockIdx.z * kCand;
    const int nc = (int)((C - c0 < kCand) ? C - c0 : kCand);
    const bool first = blockIdx.z == 0;                  // this block also forms base and bad

    // The candidates are judged HERE, before any arithmetic on them: an inadmissible or non-finite pair sets the status bit
    // and is replaced by (a, b - 1) = (0, 1), so that theta > 0 and r > 0 hold for everything the loop computes.
    double a[kCand], bm1[kCand], acc[kCand];
    uint32_t bad = 0, flags = 0;
#pragma unroll
    for (int c = 0; c < kCand; ++c) {
        a[c] = 0.0;
        bm1[c] = 1.0;                                            // (an absent candidate: theta = 1, and never added)
        acc[c] = 0.0;
        if (mine && c < nc) {
            const double av = alpha[(c0 + c) * G + g], bv = beta[(c0 + c) * G + g];
            if (admissible(av, bv)) {
                a[c] = av;
                bm1[c] = bv - 1.0;
            } else {
                flags |= PROSSTT_AMD_FIT_PARAMETER;
            }
        }
    }
    double base = 0.0, m = 0.0;
    int32_t neg = 0, have_row = -1;

    // where the lane's sums go, formed here so that the loop need not keep the kernel's arguments for it
    const size_t at = (size_t)blockIdx.y * (size_t)G + (size_t)(mine ? g : 0);
    double* ll_out = llslab + ((size_t)blockIdx.y * (size_t)C + (size_t)c0) * (size_t)G + (size_t)(mine ? g : 0);
    double* base_out = baseslab + at;
    uint32_t* bad_out = badslab + at;
    uint32_t* status_out = status;
    // (in vector registers from here on, not sunk below the loop: kept as scalar arguments, 10 to 18 of them spilled)
    asm volatile("" : "+v"(ll_out), "+v"(base_out), "+v"(bad_out), "+v"(status_out));

    // everything below counts rows from r0, in 32 bits
    const int32_t* __restrict__ lab = labels + lane.r0;
    const double* __restrict__ siz = size + lane.r0;
    const ColumnReader rd = column_reader(lane, X, ld);
    const int n_rows = rd.n_rows;
    const double* __restrict__ mcol = means + (mine ? g : 0);

#pragma unroll 1
    for (int rt = 0; rt < n_rows; rt += kColumnTile) {
        const int rows = (n_rows - rt < kColumnTile) ? n_rows - rt : kColumnTile;
        if (rd.staged) {
            __syncthreads();                              // the previous tile has been read
            column_stage(tile, rd, ld, rt, rows);
            __syncthreads();
        }
#pragma unroll 1
        for (int tr = 0; tr < rows; ++tr) {
            const int r = rt + tr;
            const int32_t k = lab[r];                     // uniform over the block, as is everything up to the entry
            if (k < 0) continue;
            if (k >= K) { flags |= PROSSTT_AMD_FIT_LABEL; continue; }
            const double s = siz[r];
            if (!(s > 0.0) || s > kLargest) { flags |= PROSSTT_AMD_FIT_SIZE; continue; }
            if (k != have_row) {
                have_row = k;
                m = mine ? mcol[(int64_t)k * ldm] : 0.0;
                if (!(m >= 0.0) || m > kLargest) { flags |= PROSSTT_AMD_FIT_MEAN; m = 0.0; }
            }
            const int32_t x = column_entry(tile, rd, ld, rt, tr);
            neg |= x;
            if (x < 0) continue;
            const double mu = s * m;                      // (finite: both factors are at most kLargest)
            if (!(mu > 0.0)) {                            // (mu = 0; a refused mean counts as 0 and the call as failed)
                bad += x > 0 ? 1u : 0u;
                continue;
            }
            if (first && x > 1) base += lgd(1.0, x);
#pragma unroll
            for (int c = 0; c < kCand; ++c)
                if (c < nc) acc[c] += term(mu, x, a[c], bm1[c]);
        }
    }

    if (mine) {
#pragma unroll
        for (int c = 0; c < kCand; ++c)
            if (c < nc) ll_out[(size_t)c * (size_t)G] = acc[c];
        if (first) {
            *base_out = base;
            *bad_out = bad;
        }
    }
    if (neg < 0) flags |= PROSSTT_AMD_FIT_NEGATIVE;
    if (flags) atomicOr(status_out, flags);
}

// One thread per (candidate, gene) and one per gene: i < C G adds ll's partial sums; C G <= i < (C + 1) G adds base's and
// bad's.
__global__ __launch_bounds__(kThreads) void fit_finish_kernel(const double* __restrict__ llslab,
                                                              const double* __restrict__ baseslab,
                                                              const uint32_t* __restrict__ badslab, int64_t G, int64_t C,
                                                              int64_t row_blocks, double* __restrict__ ll,
                                                              double* __restrict__ base, uint64_t* __restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t CG = C * G;
    if (i < CG) {
        double sum = 0.0;
        for (int64_t b = 0; b < row_blocks; ++b) sum += llslab[b * CG + i];
        ll[i] = sum;
    } else if (i < CG + G) {
        const int64_t g = i - CG;
        double sum = 0.0;
        uint64_t n = 0;
        for (int64_t b = 0; b < row_blocks; ++b) {
            sum += baseslab[b * G + g];
            n += badslab[b * G + g];
        }
        base[g] = sum;
        bad[g] = n;
    }
}

int check_sizes(int64_t N, int64_t G, int64_t C)
{
    if (int rc = column_matrix_refused(N, G)) return rc;
    if (C < 1 || C > kMaxC)
        return fail(PROSSTT_AMD_FIT_EINVAL, "need 1 <= C <= %d candidates (got %lld)", kMaxC, (long long)C);
    return column_finish_refused(G, kMaxC + 1);                      // (the finishing grid: (C + 1) G / 256 blocks, for any C)
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_fit_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_fit_workspace_bytes(int64_t N, int64_t G, int64_t C, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_FIT_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, C)) return rc;
    *bytes = geometry(N, G, C).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_fit_loglik(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, const double* size,
                                      const int32_t* labels, int64_t K, const double* means, int64_t ldm,
                                      const double* alpha, const double* beta, int64_t C, void* ws, uint64_t ws_bytes,
                                      double* ll, double* base, uint64_t* bad, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, C)) return rc;
    if (K < 1 || K >= (int64_t(1) << 31))
        return fail(PROSSTT_AMD_FIT_EINVAL, "need 1 <= K < 2^31 rows of means (got %lld)", (long long)K);
    if (ld < G) return stride_below_row(ld, G);
    if (ldm < G) return stride_below_row(ldm, G);
    if (!X || !size || !labels || !means || !alpha || !beta || !ll || !base || !bad || !status)
        return fail(PROSSTT_AMD_FIT_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, C);
    if (!ws || ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    double* llslab = (double*)(w + geo.ll);
    double* baseslab = (double*)(w + geo.base);
    uint32_t* badslab = (uint32_t*)(w + geo.bad);
    const dim3 grid((unsigned)geo.strips, (unsigned)geo.row_blocks, (unsigned)geo.chunks);
    const int64_t rows = geo.rows_per_block;
    if (aligned(X, ld, 4))
        fit_loglik_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, size, labels, (int32_t)K, means, ldm, alpha, beta, C, rows,
                                                                 llslab, baseslab, badslab, status);
    else
        fit_loglik_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, size, labels, (int32_t)K, means, ldm, alpha, beta, C, rows,
                                                                  llslab, baseslab, badslab, status);
    HIP_TRY(hipGetLastError());
    fit_finish_kernel<<<dim3((unsigned)cdiv((C + 1) * G, kThreads)), dim3(kThreads), 0, st>>>(
        llslab, baseslab, badslab, G, C, geo.row_blocks, ll, base, bad);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
