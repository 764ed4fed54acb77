// libprosstt_amd_knn.so -- exact k nearest neighbours of the rows of an N x d f32 panel (include/prosstt_amd_knn.h).
//
// The search runs over chunks of chunk_rows query cells; per chunk two kernels (256 threads = 4 waves each):
//   knn_distance_kernel  a block owns a 64 x 64 tile of (query, candidate) pairs.  Per slice of 32 coordinates it stages
//                        both 64 x 32 pieces of P in LDS, coordinate-major (wave w loads coordinates 8w .. 8w + 7 of row
//                        `lane`, so a store's 64 lanes write 64 consecutive floats), and each lane reads its four queries
//                        and its four candidates of a coordinate with one ds_read_b128 each.  A lane keeps a 4 x 4 block
//                        of accumulators across the slices: acc += (q - c) * (q - c), a separate subtract, multiply and
//                        add in ascending coordinate (-ffp-contract=off).  The tile goes to the slab [rows_p][Np] of the
//                        workspace with 16-byte stores, the diagonal like any other entry.  rows_p and Np are the chunk
//                        and N rounded up to 64: whole tiles are stored, and what lies past N is never read back.
//   knn_select_kernel    one block per query row of the slab.  Radix select on the 32 bits of d2, most significant byte
//                        first: each of four passes over the row counts the byte of the keys that match the prefix so far
//                        in a 256-bin histogram in LDS (integer atomics: counts do not depend on order; a wave first adds
//                        the lanes that share its first lane's bin in one atomic, since the top bytes of a row are nearly
//                        all equal), and a block prefix sum picks the bin that holds the k-th key.  That gives T, the bit
//                        pattern of the k-th smallest d2, and the number of keys below T.  A last pass in ascending j
//                        gathers every key below T (any order) and the lowest-indexed keys equal to T (block prefix sum
//                        over consecutive segments) until k are held; a bitonic sort of the 64-bit keys bits << 32 | j in
//                        LDS orders them, and the row is written to index and sqdist.  The self pair is skipped.
// There are no floating-point atomics and every key of a row is distinct: equal inputs give equal bits for any chunking.
#include "../../../include/prosstt_amd_knn.h"

#define ABI_EINVAL PROSSTT_AMD_KNN_EINVAL
#define ABI_EHIP PROSSTT_AMD_KNN_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // check_workspace

namespace {

constexpr int kTile = 64;                      // queries and candidates of a distance block
constexpr int kSlice = 32;                     // coordinates staged at a time
constexpr int kMaxD = 128;
constexpr int kMaxK = 1024;
constexpr int kSeg = 4 * kThreads;             // entries of a slab row that the select block reads per step
constexpr int64_t kSlabTarget = int64_t(192) << 20;     // bytes: the slab stays inside the 256 MiB last-level cache
constexpr int64_t kSlabMaxEntries = int64_t(1) << 40;
constexpr int64_t kMaxGridY = 65535;

struct Geometry {
    int64_t chunk = 0;       // query rows per chunk
    int64_t rows_p = 0;      // the chunk rounded up to whole tiles
    int64_t np = 0;          // N rounded up to whole tiles: the slab's row stride
    size_t bytes = 0;
};

int64_t default_chunk(int64_t N)
{
    const int64_t np = cdiv(N, kTile) * kTile;
    const int64_t rows = kSlabTarget / (4 * np) / kTile * kTile;     // whole tiles, at least one
    return rows < kTile ? (kTile < N ? kTile : N) : (rows < N ? rows : N);
}

// 0 and the geometry, or the refusal of a bad size
int geometry(int64_t N, int64_t d, int64_t k, int64_t chunk_rows, Geometry* g)
{
    if (N < 2 || N >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 2 <= N < 2^31 (got %lld)", (long long)N);
    if (d < 1 || d > kMaxD) return fail(ABI_EINVAL, "need 1 <= d <= %d (got %lld)", kMaxD, (long long)d);
    const int64_t kmax = N - 1 < kMaxK ? N - 1 : kMaxK;
    if (k < 1 || k > kmax) return fail(ABI_EINVAL, "need 1 <= k <= min(N - 1, %d) = %lld (got %lld)", kMaxK,
                                       (long long)kmax, (long long)k);
    if (chunk_rows < 0 || chunk_rows > N)
        return fail(ABI_EINVAL, "need 0 <= chunk_rows <= N (got %lld)", (long long)chunk_rows);
    g->chunk = chunk_rows ? chunk_rows : default_chunk(N);
    g->rows_p = cdiv(g->chunk, kTile) * kTile;
    g->np = cdiv(N, kTile) * kTile;
    if (g->rows_p > kSlabMaxEntries / g->np)
        return fail(ABI_EINVAL, "a slab of %lld x %lld distances is above 2^40 entries: pass a smaller chunk_rows",
                    (long long)g->rows_p, (long long)g->np);
    g->bytes = pad((size_t)g->rows_p * (size_t)g->np * 4);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------- distances

// Coordinates c .. c + 7 of one row (zeros outside the panel); `row` is a valid row even when !row_ok.
template <bool VEC>
__device__ __forceinline__ void load8(float (&v)[8], const float* __restrict__ P, int64_t ld, int64_t row, bool row_ok,
                                      int64_t c, int64_t d)
{
    const float* __restrict__ rp = P + row * ld;
    if (VEC && row_ok && c + 8 <= d) {
        const float4 a = *reinterpret_cast<const float4*>(rp + c);
        const float4 b = *reinterpret_cast<const float4*>(rp + c + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (row_ok && c + q < d) ? rp[c + q] : 0.0f;
    }
}

// One coordinate of the tile: the lane's 4 queries against its 4 candidates.
__device__ __forceinline__ void accumulate(float (&acc)[4][4], const float* __restrict__ qs, const float* __restrict__ cs,
                                           int c, int ty, int tx)
{
    const float4 a = *reinterpret_cast<const float4*>(qs + c * kTile + 4 * ty);
    const float4 b = *reinterpret_cast<const float4*>(cs + c * kTile + 4 * tx);
    const float q[4] = {a.x, a.y, a.z, a.w};
    const float p[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float t = q[r] - p[s];
            acc[r][s] += t * t;
        }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void knn_distance_kernel(const float* __restrict__ P, int64_t N, int64_t d,
                                                                int64_t ld, int64_t q0, float* __restrict__ slab,
                                                                int64_t np)
{
    __shared__ __attribute__((aligned(16))) float qs[kSlice * kTile];
    __shared__ __attribute__((aligned(16))) float cs[kSlice * kTile];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, tx = tid & 15, ty = tid >> 4;
    const int64_t ct = blockIdx.x, qt = blockIdx.y;   // consecutive blocks share their queries and walk the candidates
    const int64_t qrow = q0 + qt * kTile + lane, crow = ct * kTile + lane;
    const bool q_ok = qrow < N, c_ok = crow < N;
    const int64_t qr = q_ok ? qrow : 0, cr = c_ok ? crow : 0;

    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[r][s] = 0.0f;
    float qv[8], cv[8];
    load8<VEC>(qv, P, ld, qr, q_ok, 8 * w, d);
    load8<VEC>(cv, P, ld, cr, c_ok, 8 * w, d);
    for (int64_t c0 = 0; c0 < d; c0 += kSlice) {
        __syncthreads();                              // the previous slice has been read
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            qs[(8 * w + q) * kTile + lane] = qv[q];
            cs[(8 * w + q) * kTile + lane] = cv[q];
        }
        __syncthreads();
        if (c0 + kSlice < d) {                        // the next slice's loads fly during this slice's arithmetic
            load8<VEC>(qv, P, ld, qr, q_ok, c0 + kSlice + 8 * w, d);
            load8<VEC>(cv, P, ld, cr, c_ok, c0 + kSlice + 8 * w, d);
        }
        if (c0 + kSlice <= d) {
#pragma unroll
            for (int c = 0; c < kSlice; ++c) accumulate(acc, qs, cs, c, ty, tx);
        } else {
            const int cn = (int)(d - c0);
#pragma unroll 2
            for (int c = 0; c < cn; ++c) accumulate(acc, qs, cs, c, ty, tx);
        }
    }
    float* __restrict__ out = slab + (qt * kTile + 4 * ty) * np + ct * kTile + 4 * tx;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        *reinterpret_cast<float4*>(out + r * np) = make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
}

// ---------------------------------------------------------------------------------------------------------- selection

// Inclusive prefix sum of v over the block's 256 threads; total: the block's sum.  wsum: 4 words of LDS that no other
// call uses until the call after next (the callers alternate between two).
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wsum, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    const uint32_t s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
    total = s0 + s1 + s2 + s3;
    return v + (wave > 0 ? s0 : 0u) + (wave > 1 ? s1 : 0u) + (wave > 2 ? s2 : 0u);
}

// The lane's four entries j0 .. j0 + 3 of a slab row (rows are 16-byte aligned and padded to whole tiles past N).
__device__ __forceinline__ void load_entries(uint32_t (&b)[4], const uint32_t* __restrict__ row, int64_t j0, int64_t N)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (j0 < N) v = *reinterpret_cast<const uint4*>(row + j0);
    b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
}

__global__ __launch_bounds__(kThreads) void knn_select_kernel(const uint32_t* __restrict__ slab, int64_t np, int64_t N,
                                                              int64_t q0, int k, int n_sort, int32_t* __restrict__ index,
                                                              uint32_t* __restrict__ sqdist)
{
    __shared__ unsigned long long keys[kMaxK];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wsum[2][4];
    __shared__ uint32_t sel[2];
    __shared__ uint32_t n_below;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t i = q0 + blockIdx.x;
    const uint32_t* __restrict__ row = slab + (int64_t)blockIdx.x * np;
    const int64_t segs = (N + kSeg - 1) / kSeg;

    hist[tid] = 0u;
    for (int r = tid; r < n_sort; r += kThreads) keys[r] = ~0ull;
    if (tid == 0) n_below = 0u;
    __syncthreads();

    // T = prefix after four passes: the bits of the k-th smallest d2; below: keys under T; k_rem: keys equal to T to take
    uint32_t prefix = 0u, k_rem = (uint32_t)k, below = 0u;
    int par = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        for (int64_t s = 0; s < segs; ++s) {
            const int64_t j0 = s * kSeg + 4 * tid;
            uint32_t b[4];
            load_entries(b, row, j0, N);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t j = j0 + e;
                if (j < N && j != i && (uint32_t)((uint64_t)b[e] >> (shift + 8)) == prefix) {
                    const uint32_t bin = (b[e] >> shift) & 255u;
                    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)bin);
                    const unsigned long long same = __ballot(bin == first);
                    if (bin != first)
                        atomicAdd(&hist[bin], 1u);
                    else if (lane == __builtin_ctzll(same))
                        atomicAdd(&hist[first], (uint32_t)__builtin_popcountll(same));
                }
            }
        }
        __syncthreads();
        const uint32_t h = hist[tid];
        uint32_t total;
        const uint32_t incl = block_scan(h, wsum[par], total);
        par ^= 1;
        const uint32_t excl = incl - h;
        if (excl < k_rem && k_rem <= incl) {          // one bin holds the k_rem-th key
            sel[0] = (uint32_t)tid;
            sel[1] = excl;
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        k_rem -= sel[1];
        below += sel[1];
        hist[tid] = 0u;
        __syncthreads();
    }

    const uint32_t T = prefix, need = k_rem;
    uint32_t eq_base = 0u;                            // keys equal to T met so far (the same in every thread)
    for (int64_t s = 0; s < segs; ++s) {
        const int64_t j0 = s * kSeg + 4 * tid;
        uint32_t b[4];
        load_entries(b, row, j0, N);
        bool eq[4];
        uint32_t ne = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t j = j0 + e;
            const bool ok = j < N && j != i;
            if (ok && b[e] < T) {
                const uint32_t pos = atomicAdd(&n_below, 1u);
                if (pos < below) keys[pos] = ((unsigned long long)b[e] << 32) | (uint32_t)j;
            }
            eq[e] = ok && b[e] == T;
            ne += eq[e] ? 1u : 0u;
        }
        if (eq_base < need) {                         // block-uniform
            uint32_t total;
            uint32_t r = eq_base + block_scan(ne, wsum[par], total) - ne;
            par ^= 1;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (eq[e]) {
                    if (r < need) keys[below + r] = ((unsigned long long)T << 32) | (uint32_t)(j0 + e);
                    ++r;
                }
            eq_base += total;
        }
    }

    // bitonic sort of keys[0 .. n_sort): the k keys and the padding of all ones behind them
    for (int size = 2; size <= n_sort; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (n_sort >> 1); t += kThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == ((lo & size) == 0)) {
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
        }
    __syncthreads();
    for (int r = tid; r < k; r += kThreads) {
        const unsigned long long key = keys[r];
        index[i * k + r] = (int32_t)(uint32_t)key;
        sqdist[i * k + r] = (uint32_t)(key >> 32);
    }
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_knn_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_knn_workspace_bytes(int64_t N, int64_t d, int64_t k, int64_t chunk_rows, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_KNN_EINVAL, "NULL argument");
    Geometry g;
    if (int rc = geometry(N, d, k, chunk_rows, &g)) return rc;
    *bytes = g.bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_knn_search(void* stream, const float* P, int64_t N, int64_t d, int64_t ld, int64_t k,
                                      int64_t chunk_rows, int32_t* index, float* sqdist, void* ws, uint64_t ws_bytes) try
{
    Geometry g;
    if (int rc = geometry(N, d, k, chunk_rows, &g)) return rc;
    if (ld < d) return stride_below_row(ld, d);
    if (!P || !index || !sqdist) return fail(PROSSTT_AMD_KNN_EINVAL, "NULL argument");
    if (int rc = check_workspace(ws, ws_bytes, g.bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* slab = (float*)ws;
    const int64_t ctiles = g.np / kTile;
    const bool vec = aligned(P, ld, 4);
    int n_sort = 1;
    while (n_sort < k) n_sort <<= 1;
    for (int64_t q0 = 0; q0 < N; q0 += g.chunk) {
        const int64_t rows = q0 + g.chunk < N ? g.chunk : N - q0;
        const int64_t qtiles = cdiv(rows, kTile);
        for (int64_t t0 = 0; t0 < qtiles; t0 += kMaxGridY) {        // (one launch unless chunk_rows is above 4 million)
            const dim3 grid((unsigned)ctiles, (unsigned)(qtiles - t0 < kMaxGridY ? qtiles - t0 : kMaxGridY));
            float* part = slab + t0 * kTile * g.np;
            if (vec)
                knn_distance_kernel<true><<<grid, dim3(kThreads), 0, st>>>(P, N, d, ld, q0 + t0 * kTile, part, g.np);
            else
                knn_distance_kernel<false><<<grid, dim3(kThreads), 0, st>>>(P, N, d, ld, q0 + t0 * kTile, part, g.np);
            HIP_TRY(hipGetLastError());
        }
        knn_select_kernel<<<dim3((unsigned)rows), dim3(kThreads), 0, st>>>((const uint32_t*)slab, g.np, N, q0, (int)k,
                                                                           n_sort, index, (uint32_t*)sqdist);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
ABI_CATCH
