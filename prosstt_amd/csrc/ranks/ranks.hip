// libprosstt_amd_ranks.so -- rank sums over the log-normalised count matrix (include/prosstt_amd_ranks.h).
//
// Kernels (the definition is in the header; the index arithmetic of the sort and of the fold is ranks_index.h)
//   ranks_emit_kernel   a block owns a strip of 1024 genes over 16 positions of rows: it forms the entries row by row
//                       (embed's entry()), keeps their bit patterns in an LDS tile [16][1024 + 4] and writes, per gene, the 16
//                       keys and group payloads into the gene's segment of the workspace
//   ranks_sort_kernel   one digit of the radix sort, one block per segment: histogram, exclusive scan, stable scatter
//   ranks_fold_kernel   one block per sorted segment: a walk up (P[start of the run]) and a walk down (P[end of the run],
//                       the runs' lengths), sums per group in LDS, then plain stores of Q[.][j] and T[j]
// Each sort pass is a launch of its own: no block reads through its L1 what another launch-mate stored.  There are no
// floating-point atomics and no floating-point arithmetic after entry().
#include "../../../include/prosstt_amd_ranks.h"

#define ABI_EINVAL PROSSTT_AMD_RANKS_EINVAL
#define ABI_EHIP PROSSTT_AMD_RANKS_EHIP
#include "../abi_util.h"
#include "../strip_device.h"              // the lane's column, load_row4
#include "../log1p_entry.h"                 // entry(): the float32 log1p(x * inv), shared with embed/embed.hip
#include "ranks_index.h"

namespace {

namespace ix = ranks_index;

static_assert(ix::kBlock == kThreads && ix::kSortTile == PROSSTT_AMD_RANKS_SORT_TILE, "one tile size in header and source");

constexpr int kMaxGroups = PROSSTT_AMD_RANKS_MAX_GROUPS;
constexpr int64_t kMaxRows = PROSSTT_AMD_RANKS_MAX_ROWS;
constexpr int64_t kMaxGridY = 65535;
constexpr int64_t kWorkspaceTarget = (int64_t(1) << 30) - 1024;      // the four arrays' padding is below 1024 bytes
constexpr int kEmitRows = 16;               // positions per block of the emit kernel
constexpr int kTileLd = kStrip + 4;         // the LDS tile's row stride in keys: 16-byte rows, and a column's 16 keys
                                            // fall on banks 4 apart (2-way at the worst) when the tile is read transposed
constexpr int kBatch = 4;                   // rows whose loads are in flight together

struct Geometry {
    int64_t genes_per_pass = 0, entries = 0;
    size_t key_at[2] = {0, 0}, pay_at[2] = {0, 0}, bytes = 0;
};

Geometry geometry(int64_t n_sel, int64_t G, int64_t genes_per_pass)
{
    Geometry g;
    g.genes_per_pass = genes_per_pass > 0 ? (genes_per_pass < G ? genes_per_pass : G)
                                          : clamp64(kWorkspaceTarget / (12 * (n_sel > 0 ? n_sel : 1)), 1, G);
    g.entries = g.genes_per_pass * n_sel;
    g.key_at[0] = 0;
    g.key_at[1] = g.key_at[0] + pad((size_t)g.entries * 4);
    g.pay_at[0] = g.key_at[1] + pad((size_t)g.entries * 4);
    g.pay_at[1] = g.pay_at[0] + pad((size_t)g.entries * 2);
    g.bytes = g.pay_at[1] + pad((size_t)g.entries * 2);
    return g;
}

// ------------------------------------------------------------------------------------------------------------- emit

// The keys of the positions [q0, q0 + nrows) over the lane's four genes, into the tile.  Returns the or of the counts.
template <bool VEC, bool WIDE>
__device__ __forceinline__ int32_t fill_tile(uint32_t* __restrict__ tile, uint32_t& flags, const int32_t* __restrict__ X,
                                             int64_t N, int64_t ld, const float* __restrict__ inv_size,
                                             const int32_t* __restrict__ rows, int64_t q0, int nrows, int64_t g, int col,
                                             int64_t end)
{
    int32_t neg = 0;
    for (int r = 0; r < nrows; r += kBatch) {
        int32_t x[kBatch][4];
        float inv[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int64_t row = r + u < nrows ? (int64_t)rows[q0 + r + u] : 0;          // block-uniform
            const bool ok = row >= 0 && row < N;
            if (!ok) flags |= PROSSTT_AMD_RANKS_ROW_RANGE;                               // the row is not read
            if (ok && r + u < nrows) {
                load_row4<VEC, WIDE>(x[u], X + row * ld, g, end);
                inv[u] = inv_size[row];
            } else {
                x[u][0] = x[u][1] = x[u][2] = x[u][3] = 0;
                inv[u] = 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (r + u >= nrows) break;
            uint32_t key[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                neg |= x[u][j];
                key[j] = __float_as_uint(entry(x[u][j], inv[u]));
            }
            uint32_t* at = tile + (r + u) * kTileLd;
            if (VEC) {
                *reinterpret_cast<uint4*>(at + col) = make_uint4(key[0], key[1], key[2], key[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) at[col + 256 * j] = key[j];
            }
        }
    }
    return neg;
}

// Block (x, y): the positions [16 x, 16 x + 16) of rows over the genes [g_first + 1024 y, ...) below g_end (a chunk of
// genes).  keys / pays: the chunk's segments, gene g's at (g - g_first) * n_sel.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void ranks_emit_kernel(const int32_t* __restrict__ X, int64_t N, int64_t ld,
                                                              const float* __restrict__ inv_size,
                                                              const int32_t* __restrict__ rows, int64_t n_sel,
                                                              const int64_t* __restrict__ group_start, int64_t K,
                                                              int64_t g_first, int64_t g_end, uint32_t* __restrict__ keys,
                                                              uint16_t* __restrict__ pays, uint32_t* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint32_t tile[kEmitRows * kTileLd];
    __shared__ uint16_t group_sh[kEmitRows];
    const int tid = threadIdx.x;
    const int64_t q0 = (int64_t)blockIdx.x * kEmitRows;
    const int64_t gbase = g_first + (int64_t)blockIdx.y * kStrip;
    const int nrows = (int)(n_sel - q0 < kEmitRows ? n_sel - q0 : kEmitRows);
    uint32_t flags = 0;
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int64_t k = tid; k < K; k += kThreads) {
            const int64_t a = group_start[k], b = group_start[k + 1];
            if (a < 0 || b < a || b > n_sel || (k == 0 && a != 0) || (k == K - 1 && b != n_sel))
                flags |= PROSSTT_AMD_RANKS_GROUP_RANGE;
        }
    }
    if (tid < nrows) {
        // the last group whose offset is at or below the position: always one of [0, K), whatever group_start holds
        const int64_t q = q0 + tid;
        int64_t left = 0, right = K - 1;
        while (left < right) {
            const int64_t mid = (left + right + 1) >> 1;
            if (group_start[mid] <= q) left = mid; else right = mid - 1;
        }
        group_sh[tid] = (uint16_t)left;
    }
    const int col = strip_col<VEC>(tid);
    const int64_t g = gbase + col;
    int32_t neg;
    if (VEC && strip_whole(gbase, g_end))
        neg = fill_tile<VEC, true>(tile, flags, X, N, ld, inv_size, rows, q0, nrows, g, col, g_end);
    else
        neg = fill_tile<VEC, false>(tile, flags, X, N, ld, inv_size, rows, q0, nrows, g, col, g_end);
    if (neg < 0) flags |= PROSSTT_AMD_RANKS_NEGATIVE;
    if (flags) atomicOr(status, flags);
    __syncthreads();
    // transposed: 16 consecutive threads write the 16 positions of one gene
    const int r = tid % kEmitRows, sub = tid / kEmitRows;
    if (r < nrows) {
        const uint16_t group = group_sh[r];
        for (int c = sub; c < kStrip; c += kThreads / kEmitRows) {
            const int64_t gene = gbase + c;
            if (gene >= g_end) break;
            const int64_t at = (gene - g_first) * n_sel + q0 + r;
            keys[at] = tile[r * kTileLd + c];
            pays[at] = group;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- sort

// The lanes of this wave that hold an entry with this lane's digit.
__device__ __forceinline__ uint64_t wave_peers(uint32_t digit, bool valid)
{
    uint64_t bit_ballot[ix::kDigitBits];
#pragma unroll
    for (int b = 0; b < ix::kDigitBits; ++b) bit_ballot[b] = __ballot((digit >> b) & 1u);
    return ix::peers(digit, bit_ballot, __ballot(valid));
}

// Block x sorts segment x (n entries at x * n) by the 8 key bits from `shift` up, stably, from (kin, pin) to (kout, pout).
__global__ __launch_bounds__(kThreads) void ranks_sort_kernel(const uint32_t* __restrict__ kin,
                                                              const uint16_t* __restrict__ pin,
                                                              uint32_t* __restrict__ kout, uint16_t* __restrict__ pout,
                                                              int64_t n, int shift)
{
    __shared__ uint32_t base[ix::kDigits];
    __shared__ uint32_t scan[ix::kDigits];
    __shared__ uint32_t offsets[ix::kSlots * ix::kDigits];
    __shared__ uint8_t counts[ix::kSlots * ix::kDigits];
    const int tid = threadIdx.x, lane = tid % ix::kWave, wave = tid / ix::kWave;
    const int64_t segment = (int64_t)blockIdx.x * n;
    kin += segment; pin += segment; kout += segment; pout += segment;
    const int64_t tiles = (n + ix::kSortTile - 1) / ix::kSortTile;
    base[tid] = 0;
#pragma unroll
    for (int s = 0; s < ix::kSlots; ++s) counts[s * ix::kDigits + tid] = 0;
    __syncthreads();
    // the histogram of the segment's digits: one integer LDS add per wave and distinct digit
    for (int64_t tile = 0; tile < tiles; ++tile) {
        uint32_t key[ix::kItems];
        bool valid[ix::kItems];
#pragma unroll
        for (int i = 0; i < ix::kItems; ++i) {
            const int64_t p = ix::sort_position(tile, i, tid);
            valid[i] = p < n;
            key[i] = valid[i] ? kin[p] : 0u;
        }
#pragma unroll
        for (int i = 0; i < ix::kItems; ++i) {
            const uint32_t d = ix::digit_of(key[i], shift);
            const uint64_t peer_lanes = wave_peers(d, valid[i]);
            if (valid[i] && ix::leads(peer_lanes, lane)) atomicAdd(&base[d], (uint32_t)ix::bits_set(peer_lanes));
        }
    }
    __syncthreads();
    // its exclusive scan: base[d] = the entries with a lower digit
    const uint32_t mine = base[tid];
    scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < ix::kDigits; off <<= 1) {
        const uint32_t v = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    base[tid] = scan[tid] - mine;
    __syncthreads();
    // the stable scatter, tile by tile in position order
    for (int64_t tile = 0; tile < tiles; ++tile) {
        uint32_t key[ix::kItems];
        uint16_t pay[ix::kItems];
        bool valid[ix::kItems];
        uint64_t peer_lanes[ix::kItems];
#pragma unroll
        for (int i = 0; i < ix::kItems; ++i) {
            const int64_t p = ix::sort_position(tile, i, tid);
            valid[i] = p < n;
            key[i] = valid[i] ? kin[p] : 0u;
            pay[i] = valid[i] ? pin[p] : (uint16_t)0;
        }
#pragma unroll
        for (int i = 0; i < ix::kItems; ++i) {
            const uint32_t d = ix::digit_of(key[i], shift);
            peer_lanes[i] = wave_peers(d, valid[i]);
            if (valid[i] && ix::leads(peer_lanes[i], lane))
                counts[ix::count_slot(i, wave, d)] = (uint8_t)ix::bits_set(peer_lanes[i]);
        }
        __syncthreads();
        ix::tile_offsets(counts, offsets, base, tid);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < ix::kItems; ++i) {
            if (!valid[i]) continue;
            const uint32_t to = ix::destination(offsets, i, wave, ix::digit_of(key[i], shift), peer_lanes[i], lane);
            if ((int64_t)to < n) {              // (true by construction: the offsets are the segment's own histogram)
                kout[to] = key[i];
                pout[to] = pay[i];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------- fold

// Block x folds the sorted segment x of gene g_first + x.  reference: -1 (every position counts) or a group.
__global__ __launch_bounds__(kThreads) void ranks_fold_kernel(const uint32_t* __restrict__ keys,
                                                              const uint16_t* __restrict__ pays, int64_t n, int64_t K,
                                                              int64_t reference, int64_t g_first, int64_t G,
                                                              int64_t* __restrict__ Q, int64_t* __restrict__ T)
{
    __shared__ unsigned long long q_sh[kMaxGroups];
    __shared__ unsigned long long t_sh;
    // per wave and tile parity (a tile's words are read while the next tile's are written): ranks_index.h says what they hold
    __shared__ int32_t total_sh[2][ix::kWaves], count_sh[2][ix::kWaves], end_sh[2][ix::kWaves];
    const int tid = threadIdx.x, lane = tid % ix::kWave, wave = tid / ix::kWave;
    const int64_t segment = (int64_t)blockIdx.x * n;
    keys += segment; pays += segment;
    const int64_t tiles = (n + ix::kBlock - 1) / ix::kBlock;
    for (int64_t k = tid; k < K; k += kThreads) q_sh[k] = 0;
    if (tid == 0) t_sh = 0;
    __syncthreads();

    // up: P[start of p's run] is the largest P at a run's first position at or below p
    int32_t counted = 0, start_carry = ix::kNoStart;
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const int buf = (int)(tile & 1);
        const int64_t p = ix::fold_position(tile, tid);
        const bool valid = p < n;
        const uint32_t key = valid ? keys[p] : 0u;
        const uint32_t group = valid ? pays[p] : 0u;
        const bool head = valid && (p == 0 || keys[p - 1] != key);
        const bool member = valid && (reference < 0 || (int64_t)group == reference);
        const uint64_t members = __ballot(member);
        const int32_t local = ix::start_count_local(__ballot(head), members, lane);
        if (lane == ix::kWave - 1) {
            total_sh[buf][wave] = ix::bits_set(members);
            count_sh[buf][wave] = local;
        }
        __syncthreads();
        const int32_t own = ix::lifted(local, counted + ix::count_before(total_sh[buf], wave));
        const int32_t below = ix::start_count_below(total_sh[buf], count_sh[buf], wave, counted, start_carry);
        if (valid) atomicAdd(&q_sh[group < (uint32_t)K ? group : 0u], (unsigned long long)(own > below ? own : below));
        start_carry = ix::start_count_below(total_sh[buf], count_sh[buf], ix::kWaves, counted, start_carry);
        counted += ix::count_before(total_sh[buf], ix::kWaves);
    }
    const int32_t members_total = counted;
    __syncthreads();                        // (the walk down begins on the parity the walk up ended on)

    // down: the end of p's run is the least end of a run at or above p, and P[end] the least P there; a run's first position
    // knows the run's length
    int32_t after = 0, end_carry = ix::kNoEnd, count_carry = ix::kNoEnd;
    for (int64_t tile = tiles - 1; tile >= 0; --tile) {
        const int buf = (int)(tile & 1);
        const int64_t p = ix::fold_position(tile, tid);
        const bool valid = p < n;
        const uint32_t key = valid ? keys[p] : 0u;
        const uint32_t group = valid ? pays[p] : 0u;
        const bool head = valid && (p == 0 || keys[p - 1] != key);
        const bool tail = valid && (p == n - 1 || keys[p + 1] != key);
        const bool member = valid && (reference < 0 || (int64_t)group == reference);
        const uint64_t members = __ballot(member);
        const uint64_t tails = __ballot(tail);
        const int32_t end_local = ix::end_local(tails, tile, wave, lane);
        const int32_t most = ix::end_count_local(tails, members, lane);
        if (lane == 0) {
            total_sh[buf][wave] = ix::bits_set(members);
            end_sh[buf][wave] = end_local;
            count_sh[buf][wave] = most;
        }
        __syncthreads();
        const int32_t end_far = ix::end_above(end_sh[buf], wave, end_carry);
        const int32_t run_end = end_local < end_far ? end_local : end_far;
        const int32_t p_end = most != ix::kNoStart
                                  ? members_total - (after + ix::count_after(total_sh[buf], wave) + most)
                                  : ix::end_count_above(total_sh[buf], count_sh[buf], wave, after, members_total, count_carry);
        if (valid) {
            atomicAdd(&q_sh[group < (uint32_t)K ? group : 0u], (unsigned long long)p_end);
            const int64_t t = (int64_t)run_end - p;
            if (head && t > 1) atomicAdd(&t_sh, (unsigned long long)ix::tie_term(t));
        }
        count_carry = ix::end_count_above(total_sh[buf], count_sh[buf], -1, after, members_total, count_carry);
        end_carry = ix::end_above(end_sh[buf], -1, end_carry);
        after += ix::count_after(total_sh[buf], -1);
    }
    __syncthreads();
    const int64_t gene = g_first + blockIdx.x;
    for (int64_t k = tid; k < K; k += kThreads) Q[k * G + gene] = (int64_t)q_sh[k];
    if (tid == 0) T[gene] = (int64_t)t_sh;
}

int check_sizes(int64_t n_sel, int64_t G, int64_t genes_per_pass)
{
    if (G < 1) return fail(PROSSTT_AMD_RANKS_EINVAL, "need G >= 1 (got %lld)", (long long)G);
    if (n_sel < 0 || n_sel > kMaxRows)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "need 0 <= n_sel <= 2^20 (got %lld)", (long long)n_sel);
    if (genes_per_pass < 0)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "need genes_per_pass >= 0 (got %lld)", (long long)genes_per_pass);
    const Geometry geo = geometry(n_sel, G, genes_per_pass);
    if (cdiv(geo.genes_per_pass, kStrip) > kMaxGridY)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "genes_per_pass = %lld is above the grid's %lld strips of %d genes",
                    (long long)geo.genes_per_pass, (long long)kMaxGridY, kStrip);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_ranks_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_ranks_workspace_bytes(int64_t n_sel, int64_t G, int64_t genes_per_pass, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_RANKS_EINVAL, "NULL argument");
    if (int rc = check_sizes(n_sel, G, genes_per_pass)) return rc;
    *bytes = geometry(n_sel, G, genes_per_pass).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_ranks_rank_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                           const float* inv_size, const int32_t* rows, int64_t n_sel,
                                           const int64_t* group_start, int64_t K, int64_t reference,
                                           int64_t genes_per_pass, void* ws, uint64_t ws_bytes, int64_t* Q, int64_t* T,
                                           uint32_t* status) try
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (n_sel > N)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "%lld selected rows of %lld", (long long)n_sel, (long long)N);
    if (K < 1 || K > kMaxGroups)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "need 1 <= K <= %d groups (got %lld)", kMaxGroups, (long long)K);
    if (reference < -1 || reference >= K)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "need -1 <= reference < K = %lld (got %lld)", (long long)K, (long long)reference);
    if (int rc = check_sizes(n_sel, G, genes_per_pass)) return rc;
    if (!X || !inv_size || (!rows && n_sel > 0) || !group_start || !ws || !Q || !T || !status)
        return fail(PROSSTT_AMD_RANKS_EINVAL, "NULL argument");
    if ((uintptr_t)ws % 16 != 0) return fail(PROSSTT_AMD_RANKS_EINVAL, "the workspace is not 16-byte aligned");
    const Geometry geo = geometry(n_sel, G, genes_per_pass);
    if (ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    uint32_t* key[2] = {(uint32_t*)(base + geo.key_at[0]), (uint32_t*)(base + geo.key_at[1])};
    uint16_t* pay[2] = {(uint16_t*)(base + geo.pay_at[0]), (uint16_t*)(base + geo.pay_at[1])};

    for (int64_t g0 = 0; g0 < G; g0 += geo.genes_per_pass) {
        const int64_t g1 = g0 + geo.genes_per_pass < G ? g0 + geo.genes_per_pass : G;
        const unsigned genes = (unsigned)(g1 - g0);
        if (n_sel > 0) {
            const dim3 grid((unsigned)cdiv(n_sel, kEmitRows), (unsigned)cdiv(g1 - g0, kStrip));
            // 16-byte loads need the strips of this chunk to begin on a multiple of four genes
            if (aligned(X, ld, 4) && g0 % 4 == 0)
                ranks_emit_kernel<true><<<grid, dim3(kThreads), 0, st>>>(X, N, ld, inv_size, rows, n_sel, group_start, K, g0,
                                                                         g1, key[0], pay[0], status);
            else
                ranks_emit_kernel<false><<<grid, dim3(kThreads), 0, st>>>(X, N, ld, inv_size, rows, n_sel, group_start, K, g0,
                                                                          g1, key[0], pay[0], status);
            HIP_TRY(hipGetLastError());
            for (int pass = 0; pass < 4; ++pass) {          // an even number of passes: the sorted copy is copy 0 again
                ranks_sort_kernel<<<dim3(genes), dim3(kThreads), 0, st>>>(key[pass & 1], pay[pass & 1], key[~pass & 1],
                                                                          pay[~pass & 1], n_sel, 8 * pass);
                HIP_TRY(hipGetLastError());
            }
        }
        ranks_fold_kernel<<<dim3(genes), dim3(kThreads), 0, st>>>(key[0], pay[0], n_sel, K, reference, g0, G, Q, T);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
ABI_CATCH
