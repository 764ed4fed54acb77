// libprosstt_amd_fit.so -- the count model's log-likelihood over a device count matrix for several candidate parameter
// pairs per gene (include/prosstt_amd_fit.h holds the definition; DESIGN section 22 the reasons).
//
// Kernels (256 threads = 4 waves each)
//   fit_loglik_kernel   a block owns a strip of 256 genes, a range of rows and up to kCand = 4 of the C candidates
//                       (blockIdx.z).  In the arithmetic a lane owns ONE gene: its candidates' (a, b - 1) and their sums stay
//                       in registers across the rows, and the term's code is there four times, not sixteen (what four genes
//                       per lane, count_summary's strip, times four candidates would make of the loop).
//                       <true>  rows that start on 16 bytes: a tile of kTile rows goes through LDS -- wave w loads rows
//                               w and w + 4 of the tile, a lane 16 bytes (four genes) of each -- and every lane then
//                               reads its own gene's column of the tile (a last strip of fewer than 256 genes: as <false>)
//                       <false> any alignment: the lane loads its gene's entry of the row itself (4 bytes, coalesced)
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

namespace {

constexpr int kGenes = kThreads;            // genes per block: one per lane
constexpr int kCand = 4;                    // candidates per block
constexpr int kTile = 8;                    // rows of an LDS tile of the aligned kernel: two 16-byte loads per lane
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
    g.strips = cdiv(G, kGenes);
    g.chunks = cdiv(C, kCand);
    const int64_t rb = clamp64(kTargetBlocks / g.strips, 1, cdiv(N, kStripMinRows));
    g.rows_per_block = cdiv(N, rb);
    g.row_blocks = cdiv(N, g.rows_per_block);
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
__device__ __forceinline__ bool admissible(double a, double b)
{
    const double big = 1.7976931348623157e308;
    return a >= 0.0 && a <= big && b >= 1.0 && b <= big && a + (b - 1.0) > 0.0;
}

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
    __shared__ int32_t tile[VEC ? kTile : 1][kGenes];
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.x * kGenes;
    const int64_t g = gbase + tid;
    const bool mine = g < G;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = (r0 + rows_per_block < N) ? r0 + rows_per_block : N;
    const int64_t c0 = (int64_t)blockIdx.z * kCand;
    const int nc = (int)((C - c0 < kCand) ? C - c0 : kCand);
    const bool first = blockIdx.z == 0;                  // this block also forms base and bad
    const bool staged = VEC && gbase + kGenes <= G;      // (the last, partial strip reads as the unaligned kernel does)

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

    // the lane's part of a tile's loads: row (wave + 4 i) of the tile, genes 4 * (lane of the wave) .. + 3 of the strip
    const int lrow = tid >> 6, lcol = 4 * (tid & 63);

    // where the lane's sums go, formed here so that the loop need not keep the kernel's arguments for it
    const size_t at = (size_t)blockIdx.y * (size_t)G + (size_t)(mine ? g : 0);
    double* ll_out = llslab + ((size_t)blockIdx.y * (size_t)C + (size_t)c0) * (size_t)G + (size_t)(mine ? g : 0);
    double* base_out = baseslab + at;
    uint32_t* bad_out = badslab + at;
    uint32_t* status_out = status;
    // (in vector registers from here on, not sunk below the loop: kept as scalar arguments, 10 to 18 of them spilled)
    asm volatile("" : "+v"(ll_out), "+v"(base_out), "+v"(bad_out), "+v"(status_out));

    // everything below counts rows from r0, in 32 bits
    const int n_rows = (int)(r1 - r0);
    const int32_t* __restrict__ lab = labels + r0;
    const double* __restrict__ siz = size + r0;
    const int32_t* __restrict__ xcol = X + r0 * ld + (mine ? g : 0);        // the lane's own column (read when not staged)
    const int32_t* __restrict__ xtile = X + r0 * ld + gbase + lcol;         // the lane's 16 bytes of a staged row
    const double* __restrict__ mcol = means + (mine ? g : 0);

#pragma unroll 1
    for (int rt = 0; rt < n_rows; rt += kTile) {
        const int rows = (n_rows - rt < kTile) ? n_rows - rt : kTile;
        if (staged) {
            __syncthreads();                              // the previous tile has been read
#pragma unroll
            for (int i = 0; i < kTile / 4; ++i) {
                const int tr = lrow + 4 * i;
                if (tr < rows)
                    *reinterpret_cast<int4*>(&tile[tr][lcol]) = *reinterpret_cast<const int4*>(xtile + (int64_t)(rt + tr) * ld);
            }
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
            const int32_t x = staged ? tile[tr][tid] : (mine ? xcol[(int64_t)r * ld] : 0);
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
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_FIT_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (C < 1 || C > kMaxC)
        return fail(PROSSTT_AMD_FIT_EINVAL, "need 1 <= C <= %d candidates (got %lld)", kMaxC, (long long)C);
    if (G > ((int64_t(1) << 31) - 1) * kThreads / (kMaxC + 1))       // (the finishing grid: (C + 1) G / 256 blocks, for any C)
        return fail(PROSSTT_AMD_FIT_EINVAL, "too many genes for one launch (G = %lld)", (long long)G);
    return 0;
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
