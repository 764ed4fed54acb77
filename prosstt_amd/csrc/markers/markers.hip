// libprosstt_amd_markers.so -- per-group sums over the log-normalised count matrix (include/prosstt_amd_markers.h).
//
// Kernels (the definition and the order of the sums are in the header)
//   markers_table_kernel    one block of 1024 threads, thread k for group k: blocks per group, their prefix sum, and the
//                           table (group, first, last) of every block, so that the host never reads group_start
//   markers_pass_kernel     embed_moments_kernel's strip layout over one table entry: per gene the lane keeps S1, S2 in
//                           binary64 and the count sum and the non-zeros in integer registers, and stores them to slabs
//                           [blocks][G] at the end.  A[i][j] = log1p(X[i][j] * inv_size[i]) is embed's entry()
//   markers_finish_kernel   one thread per (group, gene): the group's blocks in ascending order
// There are no floating-point atomics: the results do not depend on scheduling, and equal inputs give equal bits.
#include "../../../include/prosstt_amd_markers.h"

#define ABI_EINVAL PROSSTT_AMD_MARKERS_EINVAL
#define ABI_EHIP PROSSTT_AMD_MARKERS_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, load_row4
#include "../log1p_entry.h"                 // entry(): the float32 log1p(x * inv), shared with embed/embed.hip

namespace {

constexpr int kMaxGroups = PROSSTT_AMD_MARKERS_MAX_GROUPS;     // = the threads of the table kernel's one block
constexpr int64_t kMaxGridY = 65535;

struct Geometry {
    int64_t rows_per_block = 0, max_blocks = 0, strips = 0;
    size_t first_at = 0, table_at = 0, nz_at = 0, cs_at = 0, s1_at = 0, s2_at = 0, bytes = 0;
};

// rows_per_block = 0: the strip kernels' rule for an n_sel x G matrix.  max_blocks bounds the blocks of any grouping:
// sum_k ceil(n_k / r) <= ceil(n_sel / r) + K.
Geometry geometry(int64_t n_sel, int64_t G, int64_t K, int64_t rows_per_block)
{
    Geometry g;
    g.rows_per_block = rows_per_block > 0 ? rows_per_block : (n_sel > 0 ? strip_geometry(n_sel, G).rows_per_block : 1);
    g.max_blocks = cdiv(n_sel, g.rows_per_block) + K;
    g.strips = cdiv(G, kStrip);
    const size_t cells = (size_t)g.max_blocks * (size_t)G;
    g.first_at = 0;
    g.table_at = g.first_at + pad((size_t)(K + 1) * 8);
    g.nz_at = g.table_at + pad((size_t)g.max_blocks * 16);
    g.cs_at = g.nz_at + pad(cells * 4);
    g.s1_at = g.cs_at + pad(cells * 8);
    g.s2_at = g.s1_at + pad(cells * 8);
    g.bytes = g.s2_at + pad(cells * 8);
    return g;
}

// ------------------------------------------------------------------------------------------------------ block table

// table[b] = (group, first, last, 0): block b sums the positions [first, last) of rows.  first_block[k]: the first block of
// group k; first_block[K]: the number of blocks, at most max_blocks.  Offsets that are not ascending from 0 to n_sel are
// clamped into [0, n_sel] (and the block count to max_blocks), and reported.
__global__ __launch_bounds__(kMaxGroups) void markers_table_kernel(const int64_t* __restrict__ group_start, int64_t K,
                                                                   int64_t n_sel, int64_t rows_per_block,
                                                                   int64_t max_blocks, int64_t* __restrict__ first_block,
                                                                   int4* __restrict__ table, uint32_t* __restrict__ status)
{
    __shared__ int64_t scan[kMaxGroups];
    __shared__ int64_t first_sh[kMaxGroups + 1];
    __shared__ int64_t lo_sh[kMaxGroups], hi_sh[kMaxGroups];
    const int k = threadIdx.x;
    int64_t lo = 0, hi = 0, nb = 0;
    if (k < K) {
        const int64_t a = group_start[k], b = group_start[k + 1];
        if (a < 0 || b < a || b > n_sel || (k == 0 && a != 0) || (k == K - 1 && b != n_sel))
            atomicOr(status, PROSSTT_AMD_MARKERS_GROUP_RANGE);
        lo = a < 0 ? 0 : (a > n_sel ? n_sel : a);
        hi = b < lo ? lo : (b > n_sel ? n_sel : b);
        nb = (hi - lo + rows_per_block - 1) / rows_per_block;
    }
    scan[k] = nb;
    __syncthreads();
    for (int off = 1; off < kMaxGroups; off <<= 1) {
        const int64_t v = k >= off ? scan[k - off] : 0;
        __syncthreads();
        scan[k] += v;
        __syncthreads();
    }
    const int64_t before = scan[k] - nb;            // the blocks of the groups below k
    if (k < K) {
        first_sh[k] = before < max_blocks ? before : max_blocks;
        lo_sh[k] = lo;
        hi_sh[k] = hi;
    }
    if (k == K - 1) first_sh[K] = scan[k] < max_blocks ? scan[k] : max_blocks;
    __syncthreads();
    if (k < K) first_block[k] = first_sh[k];
    if (k == K - 1) first_block[K] = first_sh[K];
    const int64_t total = first_sh[K];
    for (int64_t b = k; b < total; b += kMaxGroups) {
        int64_t left = 0, right = K - 1;            // the last group whose first block is at or below b: it holds b
        while (left < right) {
            const int64_t mid = (left + right + 1) >> 1;
            if (first_sh[mid] <= b) left = mid; else right = mid - 1;
        }
        const int64_t first = lo_sh[left] + (b - first_sh[left]) * rows_per_block;
        const int64_t last = first + rows_per_block < hi_sh[left] ? first + rows_per_block : hi_sh[left];
        table[b] = make_int4((int)left, (int)first, (int)last, 0);
    }
}

// ------------------------------------------------------------------------------------------------------ grouped pass

constexpr int kBatch = 4;                    // rows whose loads are in flight together

struct Sums {
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    unsigned long long cs[4] = {0, 0, 0, 0};        // (counts are >= 0: a negative one is reported and voids the outputs)
    int32_t nz[4] = {0, 0, 0, 0};
    int32_t neg = 0;
};

__device__ __forceinline__ void add_row4(Sums& t, const int32_t (&x)[4], float inv)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t.neg |= x[j];
        const double a = (double)entry(x[j], inv);
        t.s1[j] += a;
        t.s2[j] = __builtin_fma(a, a, t.s2[j]);
        t.cs[j] += (uint32_t)x[j];
        t.nz[j] += x[j] > 0;
    }
}

// The sums of the positions [first, last) of rows, in that order, over the lane's four genes.
template <bool VEC, bool WIDE>
__device__ __forceinline__ void sum_rows(Sums& t, uint32_t& flags, const int32_t* __restrict__ X, int64_t N, int64_t G,
                                         int64_t ld, const float* __restrict__ inv_size, const int32_t* __restrict__ rows,
                                         int first, int last, int64_t g0)
{
    int p = first;
    // kBatch rows at a time while there are as many and all lie in the matrix: their loads are issued together and the
    // sums take them in order
    for (; p + kBatch <= last; p += kBatch) {
        int64_t r[kBatch];
        bool ok = true;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            r[u] = rows[p + u];
            ok = ok && r[u] >= 0 && r[u] < N;
        }
        if (!ok) break;
        int32_t x[kBatch][4];
        float inv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            load_row4<VEC, WIDE>(x[u], X + r[u] * ld, g0, G);
            inv[u] = inv_size[r[u]];
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) add_row4(t, x[u], inv[u]);
    }
    // the last rows of the block, and everything from a batch on that holds a row outside the matrix: one by one
    for (; p < last; ++p) {
        const int64_t r = rows[p];
        if (r < 0 || r >= N) {
            flags = PROSSTT_AMD_MARKERS_ROW_RANGE;  // the row is not read
        } else {
            int32_t x[4];
            load_row4<VEC, WIDE>(x, X + r * ld, g0, G);
            add_row4(t, x, inv_size[r]);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void markers_pass_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G,
                                                                int64_t ld, const float* __restrict__ inv_size,
                                                                const int32_t* __restrict__ rows,
                                                                const int64_t* __restrict__ block_count,
                                                                const int4* __restrict__ table, int32_t* __restrict__ nzslab,
                                                                unsigned long long* __restrict__ csslab,
                                                                double* __restrict__ s1slab, double* __restrict__ s2slab,
                                                                uint32_t* __restrict__ status)
{
    if ((int64_t)blockIdx.y >= *block_count) return;
    const int4 e = table[blockIdx.y];               // (group, first, last): block-uniform, as are the row indices below
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.x * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const bool full = strip_whole(gbase, G);
    Sums t;
    uint32_t flags = 0;
    if (VEC && full)
        sum_rows<VEC, true>(t, flags, X, N, G, ld, inv_size, rows, e.y, e.z, g0);
    else
        sum_rows<VEC, false>(t, flags, X, N, G, ld, inv_size, rows, e.y, e.z, g0);
    const size_t at = (size_t)blockIdx.y * (size_t)G;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                   // (written out: see strip_device.h)
        const int64_t g = strip_gene<VEC>(g0, j);
        if (g < G) {
            nzslab[at + g] = t.nz[j];
            csslab[at + g] = t.cs[j];
            s1slab[at + g] = t.s1[j];
            s2slab[at + g] = t.s2[j];
        }
    }
    if (t.neg < 0) flags |= PROSSTT_AMD_MARKERS_NEGATIVE;
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(kThreads) void markers_finish_kernel(const int64_t* __restrict__ first_block,
                                                                  const int32_t* __restrict__ nzslab,
                                                                  const unsigned long long* __restrict__ csslab,
                                                                  const double* __restrict__ s1slab,
                                                                  const double* __restrict__ s2slab, int64_t G,
                                                                  int64_t* __restrict__ nz, int64_t* __restrict__ cs,
                                                                  double* __restrict__ S1, double* __restrict__ S2)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    const int64_t k = blockIdx.y;
    const int64_t b0 = first_block[k], b1 = first_block[k + 1];
    int64_t n = 0;
    unsigned long long c = 0;
    double a = 0.0, b = 0.0;
    for (int64_t i = b0; i < b1; ++i) {
        n += nzslab[i * G + g];
        c += csslab[i * G + g];
        a += s1slab[i * G + g];
        b += s2slab[i * G + g];
    }
    nz[k * G + g] = n;
    cs[k * G + g] = (int64_t)c;
    S1[k * G + g] = a;
    S2[k * G + g] = b;
}

int check_sizes(int64_t n_sel, int64_t G, int64_t K, int64_t rows_per_block)
{
    if (G < 1) return fail(PROSSTT_AMD_MARKERS_EINVAL, "need G >= 1 (got %lld)", (long long)G);
    if (n_sel < 0 || n_sel >= (int64_t(1) << 31))
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "need 0 <= n_sel < 2^31 (got %lld)", (long long)n_sel);
    if (K < 1 || K > kMaxGroups)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "need 1 <= K <= %d groups (got %lld)", kMaxGroups, (long long)K);
    if (rows_per_block < 0)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "need rows_per_block >= 0 (got %lld)", (long long)rows_per_block);
    const Geometry geo = geometry(n_sel, G, K, rows_per_block);
    if (geo.max_blocks > kMaxGridY)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "%lld selected rows in blocks of %lld and %lld groups need up to %lld blocks, "
                    "above the grid's %lld", (long long)n_sel, (long long)geo.rows_per_block, (long long)K,
                    (long long)geo.max_blocks, (long long)kMaxGridY);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_markers_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_markers_workspace_bytes(int64_t n_sel, int64_t G, int64_t K, int64_t rows_per_block,
                                                   uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_MARKERS_EINVAL, "NULL argument");
    if (int rc = check_sizes(n_sel, G, K, rows_per_block)) return rc;
    *bytes = geometry(n_sel, G, K, rows_per_block).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_markers_group_moments(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                                 const float* inv_size, const int32_t* rows, int64_t n_sel,
                                                 const int64_t* group_start, int64_t K, int64_t rows_per_block, void* ws,
                                                 uint64_t ws_bytes, int64_t* nz, int64_t* cs, double* S1, double* S2,
                                                 uint32_t* status) try
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (n_sel > N)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "%lld selected rows of %lld", (long long)n_sel, (long long)N);
    if (int rc = check_sizes(n_sel, G, K, rows_per_block)) return rc;
    if (!X || !inv_size || (!rows && n_sel > 0) || !group_start || !ws || !nz || !cs || !S1 || !S2 || !status)
        return fail(PROSSTT_AMD_MARKERS_EINVAL, "NULL argument");
    if ((uintptr_t)ws % 16 != 0) return fail(PROSSTT_AMD_MARKERS_EINVAL, "the workspace is not 16-byte aligned");
    const Geometry geo = geometry(n_sel, G, K, rows_per_block);
    if (ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    int64_t* first_block = (int64_t*)(base + geo.first_at);
    int4* table = (int4*)(base + geo.table_at);
    int32_t* nzslab = (int32_t*)(base + geo.nz_at);
    unsigned long long* csslab = (unsigned long long*)(base + geo.cs_at);
    double* s1slab = (double*)(base + geo.s1_at);
    double* s2slab = (double*)(base + geo.s2_at);

    markers_table_kernel<<<dim3(1), dim3(kMaxGroups), 0, st>>>(group_start, K, n_sel, geo.rows_per_block, geo.max_blocks,
                                                               first_block, table, status);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)geo.strips, (unsigned)geo.max_blocks);
    if (aligned(X, ld, 4))
        markers_pass_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, rows, first_block + K, table, nzslab,
                                                                   csslab, s1slab, s2slab, status);
    else
        markers_pass_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, inv_size, rows, first_block + K, table, nzslab,
                                                                    csslab, s1slab, s2slab, status);
    HIP_TRY(hipGetLastError());
    markers_finish_kernel<<<dim3((unsigned)cdiv(G, kThreads), (unsigned)K), dim3(kThreads), 0, st>>>(
        first_block, nzslab, csslab, s1slab, s2slab, G, nz, cs, S1, S2);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
