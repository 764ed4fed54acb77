// libprosstt_amd_trends.so -- weighted integer sums of the cells around the nodes of a lineage tree
// (include/prosstt_amd_trends.h).
//
// Kernels (the definition is in the header)
//   trends_table_kernel    one block of 1024 threads, 1024 nodes at a time: chunks per node, their running sum, and the
//                          table (first entry, node, entries) of every chunk, so that the host never reads indptr
//   trends_pass_kernel     markers_pass_kernel's strip layout over one table entry: per gene the lane keeps three 64-bit
//                          integer sums and stores them to the outputs (a node of one chunk) or to slabs [chunks][G]
//   trends_finish_kernel   one thread per (node, gene): the node's chunks added with carry
// Everything is integer arithmetic: the results do not depend on scheduling or on the cut into chunks.
#include "../../../include/prosstt_amd_trends.h"

#define ABI_EINVAL PROSSTT_AMD_TRENDS_EINVAL
#define ABI_EHIP PROSSTT_AMD_TRENDS_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, load_row4

namespace {

constexpr int kTableThreads = 1024;
constexpr int64_t kMaxRow = PROSSTT_AMD_TRENDS_MAX_ROW_ENTRIES;
constexpr int64_t kMaxGrid = (int64_t(1) << 31) - 1;
constexpr int64_t kMaxGridY = 65535;
constexpr int kOne = PROSSTT_AMD_TRENDS_ONE;

struct alignas(16) Chunk {
    long long first;        // the chunk's first entry of indices / weights
    int node;
    int count;              // its entries, 1 .. entries_per_block
};

struct Geometry {
    int64_t entries_per_block = 0, max_chunks = 0, strips = 0;
    size_t first_at = 0, table_at = 0, s1_at = 0, lo_at = 0, hi_at = 0, bytes = 0;
};

// entries_per_block = 0: about kTargetBlocks blocks over all strips, a function of nnz and G alone.  max_chunks bounds the
// chunks of any CSR matrix of these sizes: sum_r ceil(n_r / e) <= ceil(nnz / e) + R.
Geometry geometry(int64_t R, int64_t G, int64_t nnz, int64_t entries_per_block)
{
    Geometry g;
    g.strips = cdiv(G, kStrip);
    g.entries_per_block = entries_per_block > 0
                              ? entries_per_block
                              : clamp64(cdiv(nnz * g.strips, kTargetBlocks), 64, int64_t(1) << 20);
    g.max_chunks = cdiv(nnz, g.entries_per_block) + R;
    const size_t cells = (size_t)g.max_chunks * (size_t)G;
    g.first_at = 0;
    g.table_at = g.first_at + pad((size_t)(R + 1) * 8);
    g.s1_at = g.table_at + pad((size_t)g.max_chunks * sizeof(Chunk));
    g.lo_at = g.s1_at + pad(cells * 8);
    g.hi_at = g.lo_at + pad(cells * 8);
    g.bytes = g.hi_at + pad(cells * 8);
    return g;
}

// ------------------------------------------------------------------------------------------------------ chunk table

// table[c] = (first, node, count): chunk c sums the entries [first, first + count) of its node.  first_chunk[r]: the first
// chunk of node r; first_chunk[R]: the number of chunks, at most max_chunks.  Offsets that do not ascend from 0 to nnz are
// clamped into [0, nnz] (and the chunk numbers to max_chunks), and reported, as is a row of more than kMaxRow entries.
__global__ __launch_bounds__(kTableThreads) void trends_table_kernel(const int64_t* __restrict__ indptr, int64_t R, int64_t nnz,
                                                                     int64_t entries_per_block, int64_t max_chunks,
                                                                     int64_t* __restrict__ first_chunk,
                                                                     Chunk* __restrict__ table, uint32_t* __restrict__ status)
{
    __shared__ int64_t scan[kTableThreads];
    const int k = threadIdx.x;
    int64_t carry = 0;                              // the chunks of the nodes below this round's: equal in every thread
    for (int64_t base = 0; base < R; base += kTableThreads) {
        const int64_t r = base + k;
        int64_t lo = 0, hi = 0, nb = 0;
        if (r < R) {
            const int64_t a = indptr[r], b = indptr[r + 1];
            if (a < 0 || b < a || b > nnz || (r == 0 && a != 0) || (r == R - 1 && b != nnz) || b - a > kMaxRow)
                atomicOr(status, PROSSTT_AMD_TRENDS_ROW_RANGE);
            lo = a < 0 ? 0 : (a > nnz ? nnz : a);
            hi = b < lo ? lo : (b > nnz ? nnz : b);
            nb = (hi - lo + entries_per_block - 1) / entries_per_block;
        }
        scan[k] = nb;
        __syncthreads();
        for (int off = 1; off < kTableThreads; off <<= 1) {
            const int64_t v = k >= off ? scan[k - off] : 0;
            __syncthreads();
            scan[k] += v;
            __syncthreads();
        }
        const int64_t before = carry + scan[k] - nb;
        if (r < R) {
            first_chunk[r] = before < max_chunks ? before : max_chunks;
            for (int64_t c = 0; c < nb && before + c < max_chunks; ++c) {
                const int64_t first = lo + c * entries_per_block;
                const int64_t left = hi - first;
                Chunk e;
                e.first = first;
                e.node = (int)r;
                e.count = (int)(left < entries_per_block ? left : entries_per_block);
                table[before + c] = e;
            }
        }
        carry += scan[kTableThreads - 1];
        __syncthreads();                            // scan is written again in the next round
    }
    if (k == 0) first_chunk[R] = carry < max_chunks ? carry : max_chunks;
}

// ------------------------------------------------------------------------------------------------------ the pass

constexpr int kBatch = 4;                    // rows whose loads are in flight together

struct Sums {
    unsigned long long s1[4] = {0, 0, 0, 0};        // sum q x
    unsigned long long a[4] = {0, 0, 0, 0};         // sum q (x^2 mod 2^32)
    unsigned long long b[4] = {0, 0, 0, 0};         // sum q (x^2 >> 32)
    int32_t neg = 0;
};

// (counts are >= 0: a negative one is reported and voids the outputs; it is summed as its 32-bit pattern)
__device__ __forceinline__ void add_row4(Sums& t, const int32_t (&x)[4], uint32_t q)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        t.neg |= x[j];
        const uint32_t ux = (uint32_t)x[j];
        const unsigned long long sq = (unsigned long long)ux * ux;
        t.s1[j] += (unsigned long long)q * ux;
        t.a[j] += (unsigned long long)q * (uint32_t)sq;
        t.b[j] += (unsigned long long)q * (uint32_t)(sq >> 32);
    }
}

// The sums of the entries [first, last), over the lane's four genes.
template <bool VEC, bool WIDE>
__device__ __forceinline__ void sum_entries(Sums& t, uint32_t& flags, const int32_t* __restrict__ X, int64_t N, int64_t G,
                                            int64_t ld, const int32_t* __restrict__ indices,
                                            const int32_t* __restrict__ weights, int64_t first, int64_t last, int64_t g0)
{
    int64_t p = first;
    // kBatch entries at a time while there are as many and all are admissible: their loads are issued together
    for (; p + kBatch <= last; p += kBatch) {
        int64_t r[kBatch];
        int32_t q[kBatch];
        bool ok = true;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            r[u] = indices[p + u];
            q[u] = weights[p + u];
            ok = ok && r[u] >= 0 && r[u] < N && q[u] >= 0 && q[u] <= kOne;
        }
        if (!ok) break;
        int32_t x[kBatch][4];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) load_row4<VEC, WIDE>(x[u], X + r[u] * ld, g0, G);
#pragma unroll
        for (int u = 0; u < kBatch; ++u) add_row4(t, x[u], (uint32_t)q[u]);
    }
    // the last entries of the chunk, and everything from a batch on that holds an inadmissible entry: one by one
    for (; p < last; ++p) {
        const int64_t r = indices[p];
        const int32_t q = weights[p];
        if (r < 0 || r >= N) {
            flags |= PROSSTT_AMD_TRENDS_INDEX_RANGE;            // the row is not read
        } else if (q < 0 || q > kOne) {
            flags |= PROSSTT_AMD_TRENDS_WEIGHT_RANGE;
        } else {
            int32_t x[4];
            load_row4<VEC, WIDE>(x, X + r * ld, g0, G);
            add_row4(t, x, (uint32_t)q);
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void trends_pass_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G, int64_t ld,
                                                               const int32_t* __restrict__ indices,
                                                               const int32_t* __restrict__ weights, int64_t R,
                                                               const int64_t* __restrict__ first_chunk,
                                                               const Chunk* __restrict__ table,
                                                               unsigned long long* __restrict__ s1slab,
                                                               unsigned long long* __restrict__ loslab,
                                                               unsigned long long* __restrict__ hislab,
                                                               int64_t* __restrict__ S1, unsigned long long* __restrict__ S2,
                                                               uint32_t* __restrict__ status)
{
    if ((int64_t)blockIdx.x >= first_chunk[R]) return;
    const Chunk e = table[blockIdx.x];              // block-uniform, as are the entries below
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.y * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const bool full = strip_whole(gbase, G);
    Sums t;
    uint32_t flags = 0;
    if (VEC && full)
        sum_entries<VEC, true>(t, flags, X, N, G, ld, indices, weights, e.first, e.first + e.count, g0);
    else
        sum_entries<VEC, false>(t, flags, X, N, G, ld, indices, weights, e.first, e.first + e.count, g0);
    // a node of one chunk is finished here
    const bool alone = first_chunk[e.node + 1] - first_chunk[e.node] == 1;
    const size_t at = (alone ? (size_t)e.node : (size_t)blockIdx.x) * (size_t)G;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t g = strip_gene<VEC>(g0, j);
        if (g < G) {
            // S2 = a + b 2^32 in 128 bits
            const unsigned long long lo = t.a[j] + (t.b[j] << 32);
            const unsigned long long hi = (t.b[j] >> 32) + (lo < t.a[j] ? 1u : 0u);
            if (alone) {
                S1[at + g] = (int64_t)t.s1[j];
                S2[2 * (at + g)] = lo;
                S2[2 * (at + g) + 1] = hi;
            } else {
                s1slab[at + g] = t.s1[j];
                loslab[at + g] = lo;
                hislab[at + g] = hi;
            }
        }
    }
    if (t.neg < 0) flags |= PROSSTT_AMD_TRENDS_NEGATIVE;
    if (flags) atomicOr(status, flags);
}

__global__ __launch_bounds__(kThreads) void trends_finish_kernel(const int64_t* __restrict__ first_chunk,
                                                                 const unsigned long long* __restrict__ s1slab,
                                                                 const unsigned long long* __restrict__ loslab,
                                                                 const unsigned long long* __restrict__ hislab, int64_t G,
                                                                 int64_t* __restrict__ S1, unsigned long long* __restrict__ S2)
{
    const int64_t g = (int64_t)blockIdx.y * kThreads + threadIdx.x;
    if (g >= G) return;
    const int64_t r = blockIdx.x;
    const int64_t c0 = first_chunk[r], c1 = first_chunk[r + 1];
    if (c1 - c0 == 1) return;                       // the pass wrote it
    unsigned long long s = 0, lo = 0, hi = 0;
    for (int64_t c = c0; c < c1; ++c) {
        const size_t at = (size_t)c * (size_t)G + (size_t)g;
        s += s1slab[at];
        const unsigned long long l = loslab[at];
        lo += l;
        hi += hislab[at] + (lo < l ? 1u : 0u);
    }
    const size_t at = (size_t)r * (size_t)G + (size_t)g;
    S1[at] = (int64_t)s;
    S2[2 * at] = lo;
    S2[2 * at + 1] = hi;
}

int check_sizes(int64_t R, int64_t G, int64_t nnz, int64_t entries_per_block)
{
    if (G < 1 || G > kMaxGridY * kThreads)          // (the finish kernel's grid)
        return fail(ABI_EINVAL, "need 1 <= G <= %lld (got %lld)", (long long)(kMaxGridY * kThreads), (long long)G);
    if (R < 1 || R > kMaxGrid) return fail(ABI_EINVAL, "need 1 <= R < 2^31 nodes (got %lld)", (long long)R);
    if (nnz < 0) return fail(ABI_EINVAL, "need nnz >= 0 (got %lld)", (long long)nnz);
    if (entries_per_block < 0)
        return fail(ABI_EINVAL, "need entries_per_block >= 0 (got %lld)", (long long)entries_per_block);
    const Geometry geo = geometry(R, G, nnz, entries_per_block);
    if (geo.max_chunks > kMaxGrid)
        return fail(ABI_EINVAL, "%lld entries in chunks of %lld and %lld nodes need up to %lld blocks, above the grid's %lld",
                    (long long)nnz, (long long)geo.entries_per_block, (long long)R, (long long)geo.max_chunks,
                    (long long)kMaxGrid);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_trends_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_trends_workspace_bytes(int64_t R, int64_t G, int64_t nnz, int64_t entries_per_block,
                                                  uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_sizes(R, G, nnz, entries_per_block)) return rc;
    *bytes = geometry(R, G, nnz, entries_per_block).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_trends_node_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                            const int64_t* indptr, const int32_t* indices, const int32_t* weights, int64_t R,
                                            int64_t nnz, int64_t entries_per_block, void* ws, uint64_t ws_bytes, int64_t* S1,
                                            uint64_t* S2, uint32_t* status) try
{
    if (cells_out_of_range(N)) return fail(ABI_EINVAL, "need 1 <= N < 2^31 (got %lld)", (long long)N);
    if (int rc = check_sizes(R, G, nnz, entries_per_block)) return rc;
    if (ld < G) return stride_below_row(ld, G);
    if (!X || !indptr || ((!indices || !weights) && nnz > 0) || !ws || !S1 || !S2 || !status)
        return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)indptr % 8 != 0 || (uintptr_t)S1 % 8 != 0 || (uintptr_t)S2 % 8 != 0)
        return fail(ABI_EINVAL, "indptr, S1 and S2 must be 8-byte aligned");
    if ((uintptr_t)ws % 16 != 0) return fail(ABI_EINVAL, "the workspace is not 16-byte aligned");
    const Geometry geo = geometry(R, G, nnz, entries_per_block);
    if (ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    int64_t* first_chunk = (int64_t*)(base + geo.first_at);
    Chunk* table = (Chunk*)(base + geo.table_at);
    unsigned long long* s1slab = (unsigned long long*)(base + geo.s1_at);
    unsigned long long* loslab = (unsigned long long*)(base + geo.lo_at);
    unsigned long long* hislab = (unsigned long long*)(base + geo.hi_at);
    unsigned long long* S2w = (unsigned long long*)S2;

    trends_table_kernel<<<dim3(1), dim3(kTableThreads), 0, st>>>(indptr, R, nnz, geo.entries_per_block, geo.max_chunks,
                                                                 first_chunk, table, status);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)geo.max_chunks, (unsigned)geo.strips);
    if (aligned(X, ld, 4))
        trends_pass_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, indices, weights, R, first_chunk, table, s1slab,
                                                                  loslab, hislab, S1, S2w, status);
    else
        trends_pass_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, indices, weights, R, first_chunk, table, s1slab,
                                                                   loslab, hislab, S1, S2w, status);
    HIP_TRY(hipGetLastError());
    trends_finish_kernel<<<dim3((unsigned)R, (unsigned)cdiv(G, kThreads)), dim3(kThreads), 0, st>>>(
        first_chunk, s1slab, loslab, hislab, G, S1, S2w);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
