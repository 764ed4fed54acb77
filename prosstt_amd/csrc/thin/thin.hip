// libprosstt_amd_thin.so -- binomial thinning of a device count matrix by THIN-1 (include/prosstt_amd_thin.h).
//
// Kernel (256 threads = 4 waves)
//   thin_interval_kernel<VEC>   count_summary's strip layout: a block owns a strip of 1024 genes over a range of rows and a
//                               lane owns four genes, whose half of the hash key it forms once.  Per row everything that
//                               depends on the cell is block-uniform and formed once: the id, the cell half of the key, lo, hi
//                               and the number of planes.  A zero count costs its load and its store.  A non-zero count is
//                               evaluated bit-sliced, 64 trials per step: the hash word of each needed plane, the comparator
//                               for lo and for hi, a population count.  VEC: rows are read and written in 16-byte pieces.
// Integer arithmetic only, no LDS, no atomic but the OR of a status bit.  Every loop's trip count is bounded before the loop:
// the rows by the block's range, the words of an entry by PROSSTT_AMD_THIN_MAX_COUNT / 64 = 2^18 (a count outside
// [0, 2^24] is never drawn), the planes by 16.
#include "../../../include/prosstt_amd_thin.h"

#define ABI_EINVAL PROSSTT_AMD_THIN_EINVAL
#define ABI_EHIP PROSSTT_AMD_THIN_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's genes, load_row4

namespace {

// ------------------------------------------------------------------------------------------------ THIN-1: the hash

constexpr uint64_t kCellSalt = 0xE7037ED1A0B428DBull;
constexpr uint64_t kGeneSalt = 0xA0761D6478BD642Full;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint32_t kGrid = PROSSTT_AMD_THIN_GRID;
constexpr int32_t kMaxCount = PROSSTT_AMD_THIN_MAX_COUNT;

__device__ __forceinline__ uint64_t mix(uint64_t z)      // the splitmix64 finaliser (layout.hip's mix)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

__device__ __forceinline__ uint64_t cell_key(uint64_t seed, uint64_t cell) { return mix(seed ^ mix(cell + kCellSalt)); }
__device__ __forceinline__ uint64_t gene_key(uint64_t gene) { return mix(gene + kGeneSalt); }

// What a row's interval asks of every entry: block-uniform.
struct Interval {
    uint32_t lo, hi;
    int planes;              // 16 - the number of trailing zeros of (lo | hi) mod 65536; 0 when that is 0
    bool cmp_lo, cmp_hi;     // does the bound have a bit below 2^16?  (0 and 65536 compare without a plane)
};

__device__ __forceinline__ Interval interval_of(uint32_t lo, uint32_t hi)
{
    Interval v;
    v.lo = lo;
    v.hi = hi;
    const uint32_t m = (lo | hi) & (kGrid - 1);
    v.planes = m ? 16 - __builtin_ctz(m) : 0;
    v.cmp_lo = (lo & (kGrid - 1)) != 0;
    v.cmp_hi = (hi & (kGrid - 1)) != 0;
    return v;
}

// One plane of the comparison U < k: two integer operations after the hash.
__device__ __forceinline__ void compare_plane(bool bit, uint64_t W, uint64_t& lt, uint64_t& eq)
{
    if (bit) {
        lt |= eq & ~W;
        eq &= W;
    } else {
        eq &= ~W;
    }
}

// y of an entry with 1 <= x <= 2^24 and key K, for an interval with at least one plane.
__device__ __forceinline__ int32_t thin_entry(uint32_t x, uint64_t K, const Interval& v)
{
    const uint32_t words = (x + 63u) >> 6;                     // 1 .. 2^18: x was checked against kMaxCount
    const uint64_t lo_all = (v.lo >> 16) ? ~0ull : 0ull;       // a bound of 65536: every trial is below it
    const uint64_t hi_all = (v.hi >> 16) ? ~0ull : 0ull;
    uint64_t base = K;                                         // K + kGolden * 16 w
    uint32_t y = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < words; ++w) {
        uint64_t lt_lo = lo_all, eq_lo = ~0ull, lt_hi = hi_all, eq_hi = ~0ull;
        uint64_t c = base;
#pragma unroll 1
        for (int b = 0; b < v.planes; ++b) {                   // planes <= 16
            c += kGolden;
            const uint64_t W = mix(c);
            if (v.cmp_lo) compare_plane((v.lo >> (15 - b)) & 1u, W, lt_lo, eq_lo);
            if (v.cmp_hi) compare_plane((v.hi >> (15 - b)) & 1u, W, lt_hi, eq_hi);
        }
        uint64_t in = lt_hi & ~lt_lo;
        if (w + 1 == words && (x & 63u)) in &= (1ull << (x & 63u)) - 1ull;
        y += (uint32_t)__popcll(in);
        base += 16ull * kGolden;
    }
    return (int32_t)y;
}

// The lane's four entries of a row of an output: one 16-byte store for VEC on a whole strip, else 4-byte stores below `end`.
template <bool VEC>
__device__ __forceinline__ void store_row4(const int32_t (&y)[4], int32_t* __restrict__ rp, int64_t g0, int64_t end, bool whole)
{
    if (VEC && whole) {
        *reinterpret_cast<int4*>(rp + g0) = make_int4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t g = strip_gene<VEC>(g0, j);
            if (g < end) rp[g] = y[j];
        }
    }
}

struct ThinArgs {
    const int32_t* X;
    int64_t N, G, ld;
    uint64_t seed;
    const int64_t* cell_ids;
    int64_t cell_offset, gene_offset;
    uint32_t lo_all, hi_all;
    const uint32_t* lo_table;
    const uint32_t* hi_table;
    int32_t* Y;
    int64_t ldy;
    int32_t* R;
    int64_t ldr;
    int64_t rows_per_block;
    uint32_t* status;
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void thin_interval_kernel(ThinArgs a)
{
    const int tid = threadIdx.x;
    const int64_t gbase = (int64_t)blockIdx.x * kStrip;
    const int64_t g0 = strip_g0<VEC>(gbase, tid);
    const int64_t r0 = (int64_t)blockIdx.y * a.rows_per_block;
    const int64_t r1 = (r0 + a.rows_per_block < a.N) ? r0 + a.rows_per_block : a.N;
    const bool full = strip_whole(gbase, a.G);

    uint64_t kg[4];                                            // the gene halves of the lane's keys
#pragma unroll
    for (int j = 0; j < 4; ++j) kg[j] = gene_key((uint64_t)(a.gene_offset + strip_gene<VEC>(g0, j)));

    uint32_t flags = 0;
#pragma unroll 1
    for (int64_t r = r0; r < r1; ++r) {
        // block-uniform: the cell, its half of the key, its interval
        const uint64_t cell = a.cell_ids ? (uint64_t)a.cell_ids[r] : (uint64_t)(a.cell_offset + r);
        uint32_t lo = a.lo_table ? a.lo_table[r] : a.lo_all;
        uint32_t hi = a.hi_table ? a.hi_table[r] : a.hi_all;
        const bool refused = lo > hi || hi > kGrid;            // (one value for all was refused on the host)
        if (refused) {
            flags |= PROSSTT_AMD_THIN_RANGE;
            lo = hi = 0;
        }
        const Interval v = interval_of(lo, hi);
        const bool all = v.planes == 0 && hi == kGrid && lo == 0;       // without a plane the part is x or 0
        const uint64_t kc = cell_key(a.seed, cell);

        int32_t x[4], y[4], rest[4];
        load_row4<VEC>(x, a.X + r * a.ld, g0, a.G, full);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int32_t c = x[j];
            y[j] = 0;
            rest[j] = 0;
            if (c == 0) continue;
            if (c < 0 || c > kMaxCount) {                      // never drawn: 0 in both outputs
                flags |= c < 0 ? PROSSTT_AMD_THIN_NEGATIVE : PROSSTT_AMD_THIN_OVER;
                continue;
            }
            if (refused) continue;
            if (v.planes == 0) y[j] = all ? c : 0;
            else y[j] = thin_entry((uint32_t)c, mix(kc ^ kg[j]), v);
            rest[j] = c - y[j];
        }
        store_row4<VEC>(y, a.Y + r * a.ldy, g0, a.G, full);
        if (a.R) store_row4<VEC>(rest, a.R + r * a.ldr, g0, a.G, full);
    }
    if (flags) atomicOr(a.status, flags);
}

// The rows of a block.  A count-matrix reader takes about a thousand blocks in all (strip_geometry), which suits a pass that
// is bound by memory.  Here a lane's time is the number of words of its entries, and genes differ in that by orders of
// magnitude: with 980 rows per block at 50 000 x 20 000 the block that owns the most expressed gene ran for the whole 13 ms
// of a one-plane split.  Blocks of 16 rows spread every strip over the device; the gene halves of the keys, formed once per
// block, are then 3 % of a row's hashes.  (More rows only where N / 16 would pass the grid's 65 535.)
constexpr int kThinRows = 16;
constexpr int64_t kMaxGridY = 65535;

struct Plan {
    bool vec;
    StripGeometry grid;
};

int check_sizes(int64_t N, int64_t G, int64_t ld, int64_t ldy, bool with_r, int64_t ldr)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_THIN_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (ldy < G) return stride_below_row(ldy, G);
    if (with_r && ldr < G) return stride_below_row(ldr, G);
    return 0;
}

Plan plan_of(int64_t N, int64_t G, const int32_t* X, int64_t ld, const int32_t* Y, int64_t ldy, const int32_t* R, int64_t ldr)
{
    Plan p;
    p.vec = aligned(X, ld, 4) && aligned(Y, ldy, 4) && (!R || aligned(R, ldr, 4));
    p.grid.strips = cdiv(G, kStrip);
    p.grid.rows_per_block = cdiv(N, kMaxGridY) > kThinRows ? cdiv(N, kMaxGridY) : kThinRows;
    p.grid.row_blocks = cdiv(N, p.grid.rows_per_block);
    return p;
}

// Do the bytes of two matrices of N rows of G counts meet?
bool overlap(const int32_t* A, int64_t lda, const int32_t* B, int64_t ldb, int64_t N, int64_t G)
{
    const uintptr_t a0 = (uintptr_t)A, a1 = a0 + 4 * (uintptr_t)((N - 1) * lda + G);
    const uintptr_t b0 = (uintptr_t)B, b1 = b0 + 4 * (uintptr_t)((N - 1) * ldb + G);
    return a0 < b1 && b0 < a1;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_thin_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_thin_plan(int64_t N, int64_t G, const int32_t* X, int64_t ld, const int32_t* Y, int64_t ldy,
                                     const int32_t* R, int64_t ldr, int32_t* vec, int64_t* strips, int64_t* row_blocks,
                                     int64_t* rows_per_block) try
{
    if (!vec || !strips || !row_blocks || !rows_per_block) return fail(PROSSTT_AMD_THIN_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, ld, ldy, R != nullptr, ldr)) return rc;
    const Plan p = plan_of(N, G, X, ld, Y, ldy, R, ldr);
    *vec = p.vec ? 1 : 0;
    *strips = p.grid.strips;
    *row_blocks = p.grid.row_blocks;
    *rows_per_block = p.grid.rows_per_block;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_thin_interval(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, uint64_t seed,
                                         const int64_t* cell_ids, int64_t cell_offset, int64_t gene_offset, uint32_t lo_all,
                                         uint32_t hi_all, const uint32_t* lo_table, const uint32_t* hi_table, int32_t* Y,
                                         int64_t ldy, int32_t* R, int64_t ldr, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, ld, ldy, R != nullptr, ldr)) return rc;
    if (!X || !Y || !status) return fail(PROSSTT_AMD_THIN_EINVAL, "NULL argument");
    if (cell_offset < 0 || gene_offset < 0)
        return fail(PROSSTT_AMD_THIN_EINVAL, "cell_offset and gene_offset must be >= 0 (got %lld, %lld)", (long long)cell_offset,
                    (long long)gene_offset);
    const uint32_t lo = lo_table ? 0u : lo_all, hi = hi_table ? kGrid : hi_all;
    if (lo > kGrid || hi > kGrid || (!lo_table && !hi_table && lo > hi))
        return fail(PROSSTT_AMD_THIN_EINVAL, "need 0 <= lo <= hi <= 65536 (got lo = %u, hi = %u)", lo_all, hi_all);
    if (overlap(X, ld, Y, ldy, N, G) || (R && overlap(X, ld, R, ldr, N, G)))
        return fail(PROSSTT_AMD_THIN_EINVAL, "an output overlaps the input: thinning in place is not provided");
    if (R && overlap(Y, ldy, R, ldr, N, G)) return fail(PROSSTT_AMD_THIN_EINVAL, "the two outputs overlap");
    const Plan p = plan_of(N, G, X, ld, Y, ldy, R, ldr);
    const ThinArgs a{X, N, G, ld, seed, cell_ids, cell_offset, gene_offset, lo_all, hi_all, lo_table, hi_table, Y, ldy, R, ldr,
                     p.grid.rows_per_block, status};
    const dim3 grid((unsigned)p.grid.strips, (unsigned)p.grid.row_blocks);
    if (p.vec) thin_interval_kernel<true><<<grid, dim3(kThreads), 0, (hipStream_t)stream>>>(a);
    else thin_interval_kernel<false><<<grid, dim3(kThreads), 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
