// libprosstt_amd_evaluate.so -- exact sums over all pairs of cells, binned by the pair of true classes
// (include/prosstt_amd_evaluate.h has the definition, the tables and the 64-bit bound).  256 threads = 4 waves per block,
// 64-bit offsets, no scratch, no floating point, no atomic but the status word's atomicOr.
//   evaluate_table_kernel   one block: the row blocks and the column chunks of every class, from `offsets`
//   evaluate_pass_kernel    <false>: the pair counts, <true>: the pair moments.  dpt_concordance_kernel's plan (two rows per
//                           thread 256 apart, a tile of 256 columns through LDS read as a broadcast, groups of 16 columns) over
//                           one row block and one chunk, whose class pair is block-uniform
//   evaluate_fold_kernel    <false>: int64, <true>: 128 bits.  One block per class pair adds its blocks' partial sums
#include "../../../include/prosstt_amd_evaluate.h"

#define ABI_EINVAL PROSSTT_AMD_EVALUATE_EINVAL
#define ABI_EHIP PROSSTT_AMD_EVALUATE_EHIP
#include "../abi_util.h"
#include "../wave_reduce.h"

#include <climits>

namespace {

constexpr int kTile = PROSSTT_AMD_EVALUATE_TILE;
constexpr int kRowsPerThread = 2;
constexpr int kBlockRows = kThreads * kRowsPerThread;
constexpr int kUnroll = 16;                                  // columns of a group of the pair loop
constexpr int kMaxClasses = PROSSTT_AMD_EVALUATE_MAX_CLASSES;
constexpr int kMaxDepth = PROSSTT_AMD_EVALUATE_MAX_DEPTH;
constexpr int kMaxTiles = PROSSTT_AMD_EVALUATE_MAX_TILES_PER_BLOCK;
constexpr int kCountWords = PROSSTT_AMD_EVALUATE_COUNT_WORDS;
constexpr int kMomentSums = PROSSTT_AMD_EVALUATE_MOMENT_SUMS;
constexpr int kMaxWords = kMomentSums;                       // 64-bit words of a block's partial, either pass
constexpr int64_t kMaxGridX = (int64_t(1) << 31) - 1;
constexpr int64_t kMaxGridY = 65535;
constexpr int64_t kWorkingBlocks = 4096;                     // the default tiles_per_block aims at this many blocks
static_assert(kTile == kThreads, "a thread stages one column of a tile");
static_assert(kBlockRows == PROSSTT_AMD_EVALUATE_BLOCK_ROWS, "the header names the block's rows");
static_assert(kMaxClasses == 64, "J2 lies in LDS as 64 x 64 words and a column's word holds 64 c2");
static_assert(kCountWords <= kMaxWords, "the workspace holds kMaxWords words per block");
// the header's bound: 512 rows x 256 T columns x (2 MAX_DEPTH)^2 < 2^63
static_assert((unsigned long long)kBlockRows * kTile * kMaxTiles <= (1ull << 63) / (4ull * kMaxDepth * kMaxDepth),
              "a block's partial sum fits 64 bits");

// rows [first, first + count) of class cls: a row block (count <= 512) or a column chunk (count <= 256 tiles_per_block)
struct alignas(16) Span {
    long long first;
    int cls;
    int count;
};

struct Geometry {
    int tiles_per_block = 0;
    int64_t max_row_blocks = 0, max_chunks = 0;
    size_t first_rows_at = 0, first_chunks_at = 0, rows_at = 0, chunks_at = 0, part_at = 0, bytes = 0;
};

Geometry geometry(int64_t N, int K, int tiles_per_block)
{
    Geometry g;
    const int64_t tiles = cdiv(N, kTile), row_blocks = cdiv(N, kBlockRows);
    int64_t t = tiles_per_block;
    if (t == 0) {
        t = clamp64(row_blocks * tiles / kWorkingBlocks, 1, kMaxTiles);
        const int64_t fit = cdiv(tiles, kMaxGridY - K);      // the fewest tiles per chunk that the grid's y holds
        t = t < fit ? fit : t;                               // (at most 2^23 / 65 471 = 129 < kMaxTiles)
    }
    g.tiles_per_block = (int)t;
    g.max_row_blocks = row_blocks + K;
    g.max_chunks = cdiv(N, kTile * t) + K;
    g.first_rows_at = 0;
    g.first_chunks_at = g.first_rows_at + pad((size_t)(kMaxClasses + 1) * 8);
    g.rows_at = g.first_chunks_at + pad((size_t)(kMaxClasses + 1) * 8);
    g.chunks_at = g.rows_at + pad((size_t)g.max_row_blocks * sizeof(Span));
    g.part_at = g.chunks_at + pad((size_t)g.max_chunks * sizeof(Span));
    g.bytes = g.part_at + pad((size_t)g.max_row_blocks * (size_t)g.max_chunks * kMaxWords * 8);
    return g;
}

int check_sizes(int64_t N, int32_t K, int32_t tiles_per_block)
{
    if (N < 2 || N >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 2 <= N < 2^31 (got %lld)", (long long)N);
    if (K < 1 || K > kMaxClasses) return fail(ABI_EINVAL, "need 1 <= K <= %d classes (got %d)", kMaxClasses, (int)K);
    if (tiles_per_block < 0 || tiles_per_block > kMaxTiles)
        return fail(ABI_EINVAL, "need 0 <= tiles_per_block <= %d (got %d)", kMaxTiles, (int)tiles_per_block);
    const Geometry g = geometry(N, K, tiles_per_block);
    if (g.max_chunks > kMaxGridY)
        return fail(ABI_EINVAL, "%lld cells in chunks of %d tiles need up to %lld chunks, above the grid's %lld: raise tiles_per_block",
                    (long long)N, g.tiles_per_block, (long long)g.max_chunks, (long long)kMaxGridY);
    if (g.max_row_blocks > kMaxGridX) return fail(ABI_EINVAL, "too many row blocks for one launch");
    return 0;
}

// ------------------------------------------------------------------------------------------------------- the tables

// rows[b] and chunks[c]: the spans of the definition, class after class; first_rows[p] / first_chunks[p]: the first span of
// class p, and at [K] their number, at most max_row_blocks / max_chunks.  Offsets that do not ascend from 0 to N are clamped
// into [0, N] (and the span numbers to their bounds), and reported.
__global__ __launch_bounds__(kThreads) void evaluate_table_kernel(const int64_t* __restrict__ offsets, int64_t N, int K,
                                                                  int64_t chunk_cells, int64_t max_row_blocks,
                                                                  int64_t max_chunks, int64_t* __restrict__ first_rows,
                                                                  int64_t* __restrict__ first_chunks, Span* __restrict__ rows,
                                                                  Span* __restrict__ chunks, uint32_t* __restrict__ status)
{
    __shared__ int64_t lo[kMaxClasses], hi[kMaxClasses], rows0[kMaxClasses + 1], chunks0[kMaxClasses + 1];
    const int k = threadIdx.x;
    if (k < K) {
        const int64_t a = offsets[k], b = offsets[k + 1];
        if (a < 0 || b < a || b > N || (k == 0 && a != 0) || (k == K - 1 && b != N))
            atomicOr(status, PROSSTT_AMD_EVALUATE_OFFSETS_RANGE);
        lo[k] = a < 0 ? 0 : (a > N ? N : a);
        hi[k] = b < lo[k] ? lo[k] : (b > N ? N : b);
    }
    __syncthreads();
    if (k == 0) {
        int64_t r = 0, c = 0;
        for (int p = 0; p < K; ++p) {
            rows0[p] = r;
            chunks0[p] = c;
            r += (hi[p] - lo[p] + kBlockRows - 1) / kBlockRows;
            c += (hi[p] - lo[p] + chunk_cells - 1) / chunk_cells;
        }
        rows0[K] = r;
        chunks0[K] = c;
    }
    __syncthreads();
    if (k <= K) {
        first_rows[k] = rows0[k] < max_row_blocks ? rows0[k] : max_row_blocks;
        first_chunks[k] = chunks0[k] < max_chunks ? chunks0[k] : max_chunks;
    }
    for (int p = 0; p < K; ++p) {
        for (int64_t e = rows0[p] + k; e < rows0[p + 1] && e < max_row_blocks; e += kThreads) {
            const int64_t first = lo[p] + (e - rows0[p]) * kBlockRows, left = hi[p] - first;
            Span s;
            s.first = first;
            s.cls = p;
            s.count = (int)(left < kBlockRows ? left : kBlockRows);
            rows[e] = s;
        }
        for (int64_t e = chunks0[p] + k; e < chunks0[p + 1] && e < max_chunks; e += kThreads) {
            const int64_t first = lo[p] + (e - chunks0[p]) * chunk_cells, left = hi[p] - first;
            Span s;
            s.first = first;
            s.cls = p;
            s.count = (int)(left < chunk_cells ? left : chunk_cells);
            chunks[e] = s;
        }
    }
}

// --------------------------------------------------------------------------------------------------------- the pass

__device__ __forceinline__ int32_t sign_of(int32_t d)
{
    // (spelled out as in dpt.hip: min(max(d, -1), 1) becomes two compares and two selects otherwise)
    int32_t s;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(s) : "v"(d));
    return s;
}

__device__ __forceinline__ int32_t min3(int32_t a, int32_t b, int32_t c) { return min(min(a, b), c); }

// What a thread keeps of one of its rows, and what a pair adds to it: add(the column's two staged words, J2 in LDS, J[p][q],
// whether the pair counts).  In the loop without index compares `keep` is the constant true and its selects fold away.
template <bool MOMENTS>
struct Row;

template <>
struct Row<false> {
    int32_t a = 0, b = 0;                                    // the row's values
    int32_t s = 0, p = 0, a2 = 0, b2 = 0;                    // at most 256 tiles_per_block <= 2^20 in size each

    __device__ __forceinline__ void add(int2 col, const int32_t*, int32_t, bool keep = true)
    {
        const int32_t sa = sign_of(a - col.x), sb = sign_of(b - col.y);
        const int32_t t = keep ? __mul24(sa, sb) : 0;
        s += t;
        p += __mul24(t, t);
        a2 += keep ? __mul24(sa, sa) : 0;
        b2 += keep ? __mul24(sb, sb) : 0;
    }
    __device__ __forceinline__ void end_tile() {}
    __device__ __forceinline__ void words(unsigned long long (&w)[kMaxWords]) const
    {
        w[0] += (unsigned long long)(long long)s;            // (two's complement: the class pair's total fits int64)
        w[1] += (unsigned long long)(long long)p;
        w[2] += (unsigned long long)(long long)a2;
        w[3] += (unsigned long long)(long long)b2;
    }
};

template <>
struct Row<true> {
    int32_t h = 0, h2 = 0, c2 = 0;                           // the row's depths and its second-tree branch
    uint32_t td = 0, td2 = 0;                                // sum d and sum d2 of the tile: below 2^25
    unsigned long long d = 0, d2 = 0, dd = 0, d2d2 = 0, dd2 = 0;

    // col.x: the column's h; col.y: its h2 in the low 16 bits and 64 c2 above them
    __device__ __forceinline__ void add(int2 col, const int32_t* j2, int32_t j, bool keep = true)
    {
        const int32_t hc2 = col.y & 0xffff;
        const int32_t m = min3(h, col.x, j), m2 = min3(h2, hc2, j2[(col.y >> 16) + c2]);
        uint32_t x = (uint32_t)(h + col.x - 2 * m), y = (uint32_t)(h2 + hc2 - 2 * m2);
        x = keep ? x : 0;
        y = keep ? y : 0;
        td += x;
        td2 += y;
        dd += (unsigned long long)x * x;
        d2d2 += (unsigned long long)y * y;
        dd2 += (unsigned long long)x * y;
    }
    __device__ __forceinline__ void end_tile()
    {
        d += td;
        d2 += td2;
        td = td2 = 0;
    }
    __device__ __forceinline__ void words(unsigned long long (&w)[kMaxWords]) const
    {
        w[0] += d;
        w[1] += d2;
        w[2] += dd;
        w[3] += d2d2;
        w[4] += dd2;
    }
};

// x, y: (a, b) of the counts; (h, h2) of the moments, whose c2 is `z`.  J and J2 belong to the moments.
template <bool MOMENTS>
__global__ __launch_bounds__(kThreads) void evaluate_pass_kernel(const int32_t* __restrict__ x, const int32_t* __restrict__ y,
                                                                 const int32_t* __restrict__ z, const int32_t* __restrict__ J,
                                                                 const int32_t* __restrict__ J2, int K, int K2,
                                                                 const int64_t* __restrict__ first_rows,
                                                                 const int64_t* __restrict__ first_chunks,
                                                                 const Span* __restrict__ rows, const Span* __restrict__ chunks,
                                                                 int64_t max_row_blocks, unsigned long long* __restrict__ part,
                                                                 uint32_t* __restrict__ status)
{
    constexpr int kWords = MOMENTS ? kMomentSums : kCountWords;
    __shared__ int2 cols[kTile];
    __shared__ int32_t key[kTile];                           // the column's place in its tile; INT_MIN: inadmissible
    __shared__ int32_t j2[MOMENTS ? kMaxClasses * kMaxClasses : 1];
    __shared__ int32_t tile_bad[kThreads / 64];              // per wave: the tile holds an inadmissible column (moments)
    __shared__ unsigned long long waves[kThreads / 64][kMaxWords];
    if ((int64_t)blockIdx.x >= first_rows[K] || (int64_t)blockIdx.y >= first_chunks[K]) return;
    const Span r = rows[blockIdx.x], c = chunks[blockIdx.y];            // block-uniform, as is everything derived from them
    const int tid = threadIdx.x;
    unsigned long long* mine = part + ((int64_t)blockIdx.y * max_row_blocks + blockIdx.x) * kMaxWords;
    const bool diagonal = r.cls == c.cls;
    if (r.cls > c.cls) return;                               // (the fold reads no partial below the diagonal)
    if (diagonal && c.first + c.count <= r.first) {          // the chunk lies wholly before the rows
        if (tid < kWords) mine[tid] = 0;
        return;
    }
    uint32_t flags = 0;
    int32_t j = 0;
    if constexpr (MOMENTS) {
        // J2 at c2_j 64 + c2_i (symmetric: either order of the source); entries beyond K2 are never addressed
        for (int e = tid; e < kMaxClasses * kMaxClasses; e += kThreads) {
            const int cj = e / kMaxClasses, ci = e % kMaxClasses;
            j2[e] = cj < K2 && ci < K2 ? min(max(J2[cj * K2 + ci], 0), kMaxDepth) : kMaxDepth;
        }
        j = min(max(J[r.cls * K + c.cls], 0), kMaxDepth);
    }
    Row<MOMENTS> row[kRowsPerThread];
    bool live[kRowsPerThread];
    int64_t at[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        const int i = k * kThreads + tid;
        live[k] = i < r.count;
        at[k] = r.first + i;
        if (!live[k]) continue;
        if constexpr (MOMENTS) {
            const int32_t h = x[at[k]], h2 = y[at[k]], c2 = z[at[k]];
            uint32_t bad = 0;
            if ((uint32_t)h > (uint32_t)kMaxDepth || (uint32_t)h2 > (uint32_t)kMaxDepth) bad |= PROSSTT_AMD_EVALUATE_DEPTH_RANGE;
            if ((uint32_t)c2 >= (uint32_t)K2) bad |= PROSSTT_AMD_EVALUATE_BRANCH_RANGE;
            flags |= bad;
            live[k] = bad == 0;                              // (an inadmissible row stays at depth 0 on branch 0 and is dropped)
            if (live[k]) {
                row[k].h = h;
                row[k].h2 = h2;
                row[k].c2 = c2;
            }
        } else {
            row[k].a = x[at[k]];
            row[k].b = y[at[k]];
        }
    }
    const int64_t row_end = r.first + kBlockRows;
    for (int64_t col0 = c.first; col0 < c.first + c.count; col0 += kTile) {
        const int64_t left = c.first + c.count - col0;
        const int cnt = (int)(left < kTile ? left : kTile);
        if (diagonal && col0 + cnt <= r.first) continue;     // the tile lies wholly before the rows
        __syncthreads();                                     // the previous tile has been read
        int bad = 0;
        if (tid < cnt) {
            int2 w = make_int2(x[col0 + tid], y[col0 + tid]);
            if constexpr (MOMENTS) {
                const int32_t c2 = z[col0 + tid];
                if ((uint32_t)w.x > (uint32_t)kMaxDepth || (uint32_t)w.y > (uint32_t)kMaxDepth) bad |= PROSSTT_AMD_EVALUATE_DEPTH_RANGE;
                if ((uint32_t)c2 >= (uint32_t)K2) bad |= PROSSTT_AMD_EVALUATE_BRANCH_RANGE;
                w = bad ? make_int2(0, 0) : make_int2(w.x, w.y | (c2 * kMaxClasses) << 16);
            }
            cols[tid] = w;
            key[tid] = bad ? INT_MIN : tid;
        }
        flags |= bad;
        bool masked = diagonal && col0 < row_end;            // the tile meets the rows
        if constexpr (MOMENTS) {
            // (not __syncthreads_or: that is an LDS atomic.  A ballot per wave, four plain stores, four reads)
            const int wave_bad = __any(bad);
            if (tid % 64 == 0) tile_bad[tid / 64] = wave_bad;
        }
        __syncthreads();
        if constexpr (MOMENTS)                               // or holds an inadmissible column
            masked = masked || (tile_bad[0] | tile_bad[1] | tile_bad[2] | tile_bad[3]) != 0;
        if (!masked) {
            // (groups of kUnroll columns with a constant trip count: the reads of a group are in flight together)
            int g = 0;
            for (; g + kUnroll <= cnt; g += kUnroll) {
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int2 w = cols[g + u];
#pragma unroll
                    for (int k = 0; k < kRowsPerThread; ++k) row[k].add(w, j2, j);
                }
            }
            for (; g < cnt; ++g) {
                const int2 w = cols[g];
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) row[k].add(w, j2, j);
            }
        } else {
            // a pair counts if its column is admissible and, in a block of one class, lies after its row: key > rel.  row -
            // col0 lies in (-2^31, 2^31); off the diagonal every admissible column counts.
            int32_t rel[kRowsPerThread];
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) rel[k] = diagonal ? (int32_t)(at[k] - col0) : -1;
            for (int g = 0; g < cnt; ++g) {
                const int2 w = cols[g];
                const int32_t place = key[g];
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) row[k].add(w, j2, j, place > rel[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) row[k].end_tile();
    }
    // the block's sums: the thread's live rows, the wave, the four waves
    unsigned long long w[kMaxWords] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k)
        if (live[k]) row[k].words(w);
#pragma unroll
    for (int i = 0; i < kWords; ++i) {
        w[i] = wave_sum(w[i]);
        if (tid % 64 == 0) waves[tid / 64][i] = w[i];
    }
    __syncthreads();
    if (tid < kWords) mine[tid] = waves[0][tid] + waves[1][tid] + waves[2][tid] + waves[3][tid];
    if (flags) atomicOr(status, flags);
}

// --------------------------------------------------------------------------------------------------------- the fold

// One block per class pair (p, q) = blockIdx.x / K, blockIdx.x % K: the partial sums of its row blocks x chunks, each thread
// its share in (low, high) with carry, then a tree over the threads in LDS.  WIDE: out holds (low, high) per sum, else the
// low word (an int64).  Writes nothing once a status bit is set.
template <bool WIDE>
__global__ __launch_bounds__(kThreads) void evaluate_fold_kernel(const unsigned long long* __restrict__ part, int K,
                                                                 const int64_t* __restrict__ first_rows,
                                                                 const int64_t* __restrict__ first_chunks,
                                                                 int64_t max_row_blocks, const uint32_t* __restrict__ status,
                                                                 unsigned long long* __restrict__ out)
{
    constexpr int kWords = WIDE ? kMomentSums : kCountWords;
    __shared__ unsigned long long lo[kThreads], hi[kThreads];
    if (*status != 0) return;                                // (block-uniform)
    const int tid = threadIdx.x;
    const int p = blockIdx.x / K, q = blockIdx.x % K;
    unsigned long long* mine = out + (int64_t)blockIdx.x * kWords * (WIDE ? 2 : 1);
    if (p > q) {
        if (tid < kWords * (WIDE ? 2 : 1)) mine[tid] = 0;
        return;
    }
    const int64_t r0 = first_rows[p], nr = first_rows[p + 1] - r0, c0 = first_chunks[q], nc = first_chunks[q + 1] - c0;
    unsigned long long l[kWords], h[kWords];
#pragma unroll
    for (int i = 0; i < kWords; ++i) l[i] = h[i] = 0;
    for (int64_t cc = 0; cc < nc; ++cc) {
        const unsigned long long* line = part + ((c0 + cc) * max_row_blocks + r0) * kMaxWords;
        for (int64_t rr = tid; rr < nr; rr += kThreads) {
#pragma unroll
            for (int i = 0; i < kWords; ++i) {
                const unsigned long long v = line[rr * kMaxWords + i];
                l[i] += v;
                h[i] += l[i] < v ? 1u : 0u;
            }
        }
    }
    for (int i = 0; i < kWords; ++i) {
        __syncthreads();                                     // the previous sum has been read
        lo[tid] = l[i];
        hi[tid] = h[i];
        __syncthreads();
        for (int off = kThreads / 2; off > 0; off >>= 1) {
            if (tid < off) {
                const unsigned long long v = lo[tid + off];
                lo[tid] += v;
                hi[tid] += hi[tid + off] + (lo[tid] < v ? 1u : 0u);
            }
            __syncthreads();
        }
        if (tid == 0) {
            if (WIDE) {
                mine[2 * i] = lo[0];
                mine[2 * i + 1] = hi[0];
            } else {
                mine[i] = lo[0];
            }
        }
    }
}

template <bool MOMENTS>
int run(hipStream_t st, const int32_t* x, const int32_t* y, const int32_t* z, const int64_t* offsets, const int32_t* J,
        const int32_t* J2, int64_t N, int K, int K2, int tiles_per_block, void* workspace, uint64_t bytes, void* out,
        uint32_t* status)
{
    if (!x || !y || !offsets || !workspace || !out || !status) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)workspace % 16 != 0) return fail(ABI_EINVAL, "the workspace must be 16-byte aligned");
    if ((uintptr_t)offsets % 8 != 0 || (uintptr_t)out % 8 != 0) return fail(ABI_EINVAL, "offsets and the output must be 8-byte aligned");
    const Geometry g = geometry(N, K, tiles_per_block);
    if (bytes < g.bytes) return workspace_too_small(bytes, g.bytes);
    char* base = (char*)workspace;
    int64_t* first_rows = (int64_t*)(base + g.first_rows_at);
    int64_t* first_chunks = (int64_t*)(base + g.first_chunks_at);
    Span* rows = (Span*)(base + g.rows_at);
    Span* chunks = (Span*)(base + g.chunks_at);
    unsigned long long* part = (unsigned long long*)(base + g.part_at);
    evaluate_table_kernel<<<dim3(1), dim3(kThreads), 0, st>>>(offsets, N, K, (int64_t)g.tiles_per_block * kTile, g.max_row_blocks,
                                                             g.max_chunks, first_rows, first_chunks, rows, chunks, status);
    HIP_TRY(hipGetLastError());
    evaluate_pass_kernel<MOMENTS><<<dim3((unsigned)g.max_row_blocks, (unsigned)g.max_chunks), dim3(kThreads), 0, st>>>(
        x, y, z, J, J2, K, K2, first_rows, first_chunks, rows, chunks, g.max_row_blocks, part, status);
    HIP_TRY(hipGetLastError());
    evaluate_fold_kernel<MOMENTS><<<dim3((unsigned)(K * K)), dim3(kThreads), 0, st>>>(
        part, K, first_rows, first_chunks, g.max_row_blocks, status, (unsigned long long*)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_evaluate_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_evaluate_workspace_bytes(int64_t N, int32_t K, int32_t tiles_per_block, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, K, tiles_per_block)) return rc;
    *bytes = geometry(N, K, tiles_per_block).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_evaluate_pair_counts(void* stream, const int32_t* a, const int32_t* b, const int64_t* offsets, int64_t N,
                                                int32_t K, int32_t tiles_per_block, void* workspace, uint64_t bytes,
                                                int64_t* counts, uint32_t* status) try
{
    if (int rc = check_sizes(N, K, tiles_per_block)) return rc;
    return run<false>((hipStream_t)stream, a, b, nullptr, offsets, nullptr, nullptr, N, K, 0, tiles_per_block, workspace, bytes,
                      counts, status);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_evaluate_pair_moments(void* stream, const int32_t* h, const int32_t* h2, const int32_t* c2,
                                                 const int64_t* offsets, const int32_t* J, const int32_t* J2, int64_t N, int32_t K,
                                                 int32_t K2, int32_t tiles_per_block, void* workspace, uint64_t bytes,
                                                 uint64_t* moments, uint32_t* status) try
{
    if (int rc = check_sizes(N, K, tiles_per_block)) return rc;
    if (K2 < 1 || K2 > kMaxClasses) return fail(ABI_EINVAL, "need 1 <= K2 <= %d branches (got %d)", kMaxClasses, (int)K2);
    if (!c2 || !J || !J2) return fail(ABI_EINVAL, "NULL argument");
    return run<true>((hipStream_t)stream, h, h2, c2, offsets, J, J2, N, K, K2, tiles_per_block, workspace, bytes, moments, status);
}
ABI_CATCH
