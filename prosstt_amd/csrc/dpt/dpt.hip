// libprosstt_amd_dpt.so -- diffusion pseudotime and its first branching (include/prosstt_amd_dpt.h has the definition).  256
// threads = 4 waves per block, 64-bit offsets, no scratch and no atomic.
//   dpt_rows_kernel         one thread per (source, cell): blockIdx.y is the source, so the weights and the source's
//                           coordinates are uniform across the block (scalar loads).
//   dpt_concordance_kernel  the sign products over all pairs, pure integer.  A block owns 512 rows (two per thread, 256 apart,
//                           so that two independent chains are in flight), one slab of column tiles and one sequence pair of
//                           the batch.  A tile's (ru, rv) pairs go through LDS, and every lane reads the same column at a time
//                           (a broadcast read of 8 bytes).  Five vector instructions per pair: two subtractions, two medians of
//                           three and a 24-bit multiply-add.  A tile wholly below or above the block's rows adds to lower or
//                           upper as a whole; the (at most two) tiles that meet the block's rows compare column and row.
//   dpt_reduce_kernel       the slabs' int32 partial sums into int64, one thread per (sequence pair, row).
#include "../../../include/prosstt_amd_dpt.h"

#define ABI_EINVAL PROSSTT_AMD_DPT_EINVAL
#define ABI_EHIP PROSSTT_AMD_DPT_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // check_cells, default_slabs

#include <cmath>

namespace {

constexpr int kTile = PROSSTT_AMD_DPT_TILE;
constexpr int kMaxSlabs = PROSSTT_AMD_DPT_MAX_SLABS;
constexpr int kMaxBatch = PROSSTT_AMD_DPT_MAX_BATCH;
constexpr int kMaxSources = PROSSTT_AMD_DPT_MAX_SOURCES;
constexpr int kRowsPerThread = 2;
constexpr int kBlockRows = kThreads * kRowsPerThread;
constexpr int kUnroll = 16;                    // columns of a group of the pair loop
static_assert(kTile == kThreads, "a thread stages one column of a tile");
static_assert(kBlockRows == PROSSTT_AMD_DPT_BLOCK_ROWS, "the header names the block's rows");

int check_concordance(int64_t N, int32_t batch, int32_t slabs)
{
    if (int rc = check_cells(N)) return rc;
    if (batch < 1 || batch > kMaxBatch) return fail(ABI_EINVAL, "need 1 <= batch <= %d (got %d)", kMaxBatch, (int)batch);
    if (slabs < 0 || slabs > kMaxSlabs) return fail(ABI_EINVAL, "need 0 <= slabs <= %d (got %d)", kMaxSlabs, (int)slabs);
    return 0;
}

// How the pairs are cut and how large the slabs' partial sums are.
struct Plan {
    int slabs = 0;
    int64_t tiles_per_slab = 0, row_blocks = 0;
    size_t bytes = 0;
};

Plan make_plan(int64_t N, int batch, int slabs)
{
    Plan p;
    const int64_t tiles = cdiv(N, kTile);
    p.row_blocks = cdiv(N, kBlockRows);
    p.slabs = slabs ? slabs : default_slabs(p.row_blocks * batch, tiles, kMaxSlabs);
    p.tiles_per_slab = cdiv(tiles, p.slabs);
    p.bytes = pad((size_t)batch * (size_t)p.slabs * 2 * (size_t)N * 4);      // (lower, upper) int32 per pair, slab and row
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- rows

__global__ __launch_bounds__(kThreads) void dpt_rows_kernel(const double* __restrict__ vectors, int64_t ld,
                                                            const double* __restrict__ weights, int64_t N, int n_dcs,
                                                            const int64_t* __restrict__ sources, double* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t s = sources[blockIdx.y];            // block-uniform
    if (j >= N) return;
    const int64_t at = (int64_t)blockIdx.y * N + j;
    if ((uint64_t)s >= (uint64_t)N) {                 // (nothing is read out of bounds)
        out[at] = NAN;
        return;
    }
    const double* ps = vectors + s * ld;
    const double* pj = vectors + j * ld;
    double acc = 0.0;
    for (int l = 0; l < n_dcs; ++l) {
        const double t = weights[l] * (ps[l] - pj[l]);
        acc = acc + t * t;
    }
    out[at] = sqrt(acc);
}

// --------------------------------------------------------------------------------------------------------- concordance

// s of the definition for the row's ranks (ur, vr) and the column's c
__device__ __forceinline__ int32_t pair_sign(int32_t ur, int32_t vr, int2 c)
{
    // (the median is spelled out: the compiler turns min(max(d, -1), 1) into two compares and two selects, nine instructions
    // per pair and a scalar register pair per compare)
    int32_t a, b;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(a) : "v"(ur - c.x));
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(b) : "v"(vr - c.y));
    return __mul24(a, b);
}

__global__ __launch_bounds__(kThreads) void dpt_concordance_kernel(const int32_t* __restrict__ ru, const int32_t* __restrict__ rv,
                                                                   int64_t N, int64_t tiles_per_slab, int32_t* __restrict__ part)
{
    __shared__ int2 cols[kTile];
    const int64_t slab = blockIdx.y, pair = blockIdx.z;
    const int32_t* u = ru + pair * N;
    const int32_t* v = rv + pair * N;
    const int64_t row0 = (int64_t)blockIdx.x * kBlockRows;
    int64_t row[kRowsPerThread];
    int32_t ur[kRowsPerThread], vr[kRowsPerThread], lower[kRowsPerThread], upper[kRowsPerThread];
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        row[k] = row0 + k * kThreads + threadIdx.x;
        ur[k] = row[k] < N ? u[row[k]] : 0;
        vr[k] = row[k] < N ? v[row[k]] : 0;
        lower[k] = upper[k] = 0;
    }
    const int64_t tiles = (N + kTile - 1) / kTile;
    const int64_t tile_begin = slab * tiles_per_slab;
    const int64_t tile_end = tile_begin + tiles_per_slab < tiles ? tile_begin + tiles_per_slab : tiles;
    for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
        const int64_t col0 = tile * kTile;
        const int cnt = (int)(N - col0 < kTile ? N - col0 : kTile);
        __syncthreads();                              // the previous tile has been read
        if ((int)threadIdx.x < cnt) cols[threadIdx.x] = make_int2(u[col0 + threadIdx.x], v[col0 + threadIdx.x]);
        __syncthreads();
        int32_t t[kRowsPerThread];
#pragma unroll
        for (int k = 0; k < kRowsPerThread; ++k) t[k] = 0;
        const bool below = col0 + kTile <= row0, above = col0 >= row0 + kBlockRows;      // block-uniform
        if (below || above) {
            // (groups of kUnroll columns with a constant trip count: the reads of a group are in flight together)
            int j = 0;
            for (; j + kUnroll <= cnt; j += kUnroll) {
#pragma unroll
                for (int g = 0; g < kUnroll; ++g) {
                    const int2 c = cols[j + g];
#pragma unroll
                    for (int k = 0; k < kRowsPerThread; ++k) t[k] += pair_sign(ur[k], vr[k], c);
                }
            }
            for (; j < cnt; ++j) {
                const int2 c = cols[j];
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) t[k] += pair_sign(ur[k], vr[k], c);
            }
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) {
                if (below) lower[k] += t[k];
                else upper[k] += t[k];
            }
        } else {
            // the tile meets the block's rows: columns before the row go to lower, the others to upper (s of the row
            // with itself is 0).  row - col0 lies in (-256, 512).
            int32_t before[kRowsPerThread], rel[kRowsPerThread];
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) {
                before[k] = 0;
                rel[k] = (int32_t)(row[k] - col0);
            }
            for (int j = 0; j < cnt; ++j) {
                const int2 c = cols[j];
#pragma unroll
                for (int k = 0; k < kRowsPerThread; ++k) {
                    const int32_t s = pair_sign(ur[k], vr[k], c);
                    t[k] += s;
                    before[k] += j < rel[k] ? s : 0;
                }
            }
#pragma unroll
            for (int k = 0; k < kRowsPerThread; ++k) {
                lower[k] += before[k];
                upper[k] += t[k] - before[k];
            }
        }
    }
    const int64_t base = (pair * gridDim.y + slab) * 2;
#pragma unroll
    for (int k = 0; k < kRowsPerThread; ++k) {
        if (row[k] >= N) continue;
        part[base * N + row[k]] = lower[k];
        part[(base + 1) * N + row[k]] = upper[k];
    }
}

__global__ __launch_bounds__(kThreads) void dpt_reduce_kernel(const int32_t* __restrict__ part, int64_t N, int slabs,
                                                              int64_t* __restrict__ lower, int64_t* __restrict__ upper)
{
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x, pair = blockIdx.y;
    if (r >= N) return;
    int64_t lo = 0, up = 0;
    for (int s = 0; s < slabs; ++s) {
        const int64_t base = (pair * slabs + s) * 2;
        lo += part[base * N + r];
        up += part[(base + 1) * N + r];
    }
    lower[pair * N + r] = lo;
    upper[pair * N + r] = up;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_dpt_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_dpt_workspace_bytes(int64_t N, int32_t batch, int32_t slabs, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_concordance(N, batch, slabs)) return rc;
    *bytes = make_plan(N, batch, slabs).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_dpt_rows(void* stream, const double* vectors, int64_t row_stride, const double* weights, int64_t N,
                                    int64_t n_dcs, const int64_t* sources, int64_t n_sources, double* out) try
{
    if (int rc = check_cells(N)) return rc;
    if (n_dcs < 1 || n_dcs >= N) return fail(ABI_EINVAL, "need 1 <= n_dcs < N (got %lld)", (long long)n_dcs);
    if (row_stride < n_dcs) return stride_below_row(row_stride, n_dcs);
    if (n_sources < 1 || n_sources > kMaxSources)
        return fail(ABI_EINVAL, "need 1 <= n_sources <= %d (got %lld)", kMaxSources, (long long)n_sources);
    if (!vectors || !weights || !sources || !out) return fail(ABI_EINVAL, "NULL argument");
    if ((const void*)out == (const void*)vectors) return fail(ABI_EINVAL, "out must not alias vectors");
    dpt_rows_kernel<<<dim3((unsigned)cdiv(N, kThreads), (unsigned)n_sources), dim3(kThreads), 0, (hipStream_t)stream>>>(
        vectors, row_stride, weights, N, (int)n_dcs, sources, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_dpt_concordance(void* stream, const int32_t* ru, const int32_t* rv, int64_t N, int32_t batch,
                                           int32_t slabs, void* workspace, uint64_t bytes, int64_t* lower, int64_t* upper) try
{
    if (int rc = check_concordance(N, batch, slabs)) return rc;
    // (not graph_util.h's check_workspace: the alias refusal stands between the workspace's two, and their order stays)
    if (!ru || !rv || !workspace || !lower || !upper) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)workspace % 16 != 0) return fail(ABI_EINVAL, "the workspace must be 16-byte aligned");
    if (lower == upper) return fail(ABI_EINVAL, "lower and upper must not alias each other");
    const Plan p = make_plan(N, batch, slabs);
    if (bytes < p.bytes) return workspace_too_small(bytes, p.bytes);
    hipStream_t st = (hipStream_t)stream;
    dpt_concordance_kernel<<<dim3((unsigned)p.row_blocks, (unsigned)p.slabs, (unsigned)batch), dim3(kThreads), 0, st>>>(
        ru, rv, N, p.tiles_per_slab, (int32_t*)workspace);
    HIP_TRY(hipGetLastError());
    dpt_reduce_kernel<<<dim3((unsigned)cdiv(N, kThreads), (unsigned)batch), dim3(kThreads), 0, st>>>(
        (const int32_t*)workspace, N, p.slabs, lower, upper);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
