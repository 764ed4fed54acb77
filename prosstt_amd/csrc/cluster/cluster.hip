// libprosstt_amd_cluster.so -- Louvain clustering of the connectivities of a kNN graph (include/prosstt_amd_cluster.h has
// the definition).  256 threads = 4 waves per block, 64-bit offsets.  Every sum of weights is an int64 and every atomic an
// integer atomic, so no result depends on the order in which lanes arrive; binary64 appears in the quantisation and in
// the gain alone.
//   cluster_quantize_kernel        16 lanes per row: u = floor(w 2^32 + 0.5) and the row's sum k.  Checks the weights.
//   cluster_sweep_group_kernel<G>  G = 16 or 64 lanes per row of at most G entries.  A lane holds one (c_j, u_ij) in
//                                  registers; its e is the sum of the weights of the group's lanes with its community,
//                                  read lane by lane with shuffles; the best is a xor-shuffle reduction on (gain
//                                  descending, community ascending).  No LDS.
//   cluster_sweep_table_kernel     a block per row of at most 512 entries: an open-addressing table of 1024 (community,
//                                  int64 sum) slots in LDS, claimed with an integer compare-and-swap and added to with an
//                                  integer add; then the slots are scanned for the best.
//   cluster_sweep_range_kernel     a block per row of any length: passes over ranges of 2048 community ids between the
//                                  row's lowest and highest, each with a directly indexed int64 array and a presence
//                                  bitmap in LDS; a thread carries its best across the passes.
//   cluster_totals_kernel          16 lanes per row: the row's weight inside its community, then one 64-bit integer atomic
//                                  each on in[c_i] and tot[c_i].
//   cluster_emit_kernel            16 lanes per row: the key c'_i << 32 | c'_j of every stored entry.
//   cluster_fold_kernel            a thread per eight consecutive sorted entries: sums what shares an output entry, then
//                                  one 64-bit integer atomic; heads of runs write indices, first heads of rows indptr.
#include "../../../include/prosstt_amd_cluster.h"

#define ABI_EINVAL PROSSTT_AMD_CLUSTER_EINVAL
#define ABI_EHIP PROSSTT_AMD_CLUSTER_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // check_workspace, stride_blocks
#include "../wave_reduce.h"               // group_sum, wave_sum, wave_min

#include <climits>
#include <cmath>

namespace {

constexpr int kRowLanes = 16;                        // lanes per row of the quantise, totals and emit kernels
constexpr int kTableSlots = 1024;                    // of the LDS table: twice the entries of the longest row it takes
constexpr int kTableRow = PROSSTT_AMD_CLUSTER_TABLE_ROW;
constexpr int kRange = 2048;                         // community ids per pass of the range kernel
constexpr int kFoldRun = 8;                          // sorted entries per thread of the fold
constexpr uint32_t kBadGraph = PROSSTT_AMD_CLUSTER_BAD_GRAPH, kBadCommunity = PROSSTT_AMD_CLUSTER_BAD_COMMUNITY,
                   kBadBins = PROSSTT_AMD_CLUSTER_BAD_BINS;

typedef unsigned long long u64;

int check_level(int64_t n, int64_t nnz)
{
    if (n < 1 || n >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 1 <= n < 2^31 (got %lld)", (long long)n);
    if (nnz < 1 || nnz >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 1 <= nnz < 2^31 (got %lld)", (long long)nnz);
    return 0;
}

// (begin, length) of row i, or an empty row and BAD_GRAPH
__device__ __forceinline__ void row_bounds(const int64_t* __restrict__ indptr, int64_t i, int64_t nnz, int64_t& begin,
                                           int64_t& len, uint32_t& bad)
{
    begin = indptr[i];
    len = indptr[i + 1] - begin;
    if (begin < 0 || len < 0 || begin > nnz || len > nnz - begin) {
        bad |= kBadGraph;
        begin = 0;
        len = 0;
    }
}

// -------------------------------------------------------------------------------------------------------- quantisation

__global__ __launch_bounds__(kThreads) void cluster_quantize_kernel(const int64_t* __restrict__ indptr,
                                                                    const double* __restrict__ W, int64_t N, int64_t nnz,
                                                                    int64_t* __restrict__ u, int64_t* __restrict__ k,
                                                                    uint32_t* __restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = t / kRowLanes;
    const int sub = (int)(t % kRowLanes);
    const bool ok = row < N;
    int64_t begin = 0, len = 0;
    uint32_t bad = 0u;
    if (ok) row_bounds(indptr, row, nnz, begin, len, bad);
    int64_t acc = 0;
    for (int64_t e = begin + sub; e < begin + len; e += kRowLanes) {
        const double w = W[e];
        int64_t q = 0;
        if (w >= 0.0 && w <= 1.0) q = (int64_t)floor(w * 4294967296.0 + 0.5);
        else bad |= PROSSTT_AMD_CLUSTER_BAD_WEIGHT;
        u[e] = q;
        acc += q;
    }
    acc = group_sum<kRowLanes>(acc);
    if (ok && sub == 0) k[row] = acc;
    if (bad) atomicOr(status, bad);
}

// --------------------------------------------------------------------------------------------------------------- sweep

struct Sweep {
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* u;
    const int64_t* k;
    const int32_t* rows;
    const int32_t* c;
    const int64_t* tot;
    int32_t* c_new;
    uint32_t* moved;
    uint32_t* status;
    int64_t n, nnz, first, count;      // this launch takes rows[first .. first + count)
    double gamma, m2;
    int parity;
};

__device__ __forceinline__ double gain(int64_t e, double kd, int64_t T, double gamma, double m2)
{
    return (double)e - (gamma * (kd * (double)T)) / m2;
}

// is (g, d) before (g2, d2) in the order "gain descending, community ascending"?
__device__ __forceinline__ bool before(double g, int32_t d, double g2, int32_t d2) { return g > g2 || (g == g2 && d < d2); }

__device__ __forceinline__ bool is_candidate(int32_t d, int32_t ci, int parity) { return parity == 0 ? d < ci : d > ci; }

template <int G>
__device__ __forceinline__ void group_best(double& g, int32_t& d)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const double g2 = __shfl_xor(g, off, 64);
        const int32_t d2 = __shfl_xor(d, off, 64);
        if (before(g2, d2, g, d)) {
            g = g2;
            d = d2;
        }
    }
}

// the node of row r of this launch, its community and its row; false (and nothing to do) for a row beyond the launch's
// or a bad one
__device__ __forceinline__ bool sweep_row(const Sweep& a, int64_t r, int max_len, int32_t& i, int32_t& ci, int64_t& begin,
                                          int64_t& len, uint32_t& bad)
{
    if (r >= a.count) return false;
    i = a.rows[a.first + r];
    if ((uint32_t)i >= (uint64_t)a.n) {
        bad |= kBadGraph;
        return false;
    }
    ci = a.c[i];
    if ((uint32_t)ci >= (uint64_t)a.n) {
        bad |= kBadCommunity;
        a.c_new[i] = ci;
        return false;
    }
    row_bounds(a.indptr, i, a.nnz, begin, len, bad);
    if (max_len > 0 && len > max_len) {
        bad |= kBadBins;
        len = max_len;
    }
    return true;
}

// entry e of node i's row: its community and weight if it counts (j != i, everything in range)
__device__ __forceinline__ bool sweep_entry(const Sweep& a, int64_t e, int32_t i, int32_t& cj, int64_t& uj, uint32_t& bad)
{
    const int32_t j = a.indices[e];
    if ((uint32_t)j >= (uint64_t)a.n) {
        bad |= kBadGraph;
        return false;
    }
    if (j == i) return false;
    cj = a.c[j];
    if ((uint32_t)cj >= (uint64_t)a.n) {
        bad |= kBadCommunity;
        return false;
    }
    uj = a.u[e];
    return true;
}

template <int G>
__global__ __launch_bounds__(kThreads) void cluster_sweep_group_kernel(Sweep a)
{
    const int sub = threadIdx.x % G;
    const int64_t r = (int64_t)blockIdx.x * (kThreads / G) + threadIdx.x / G;
    int32_t i = 0, ci = 0;
    int64_t begin = 0, len = 0;
    uint32_t bad = 0u;
    const bool ok = sweep_row(a, r, G, i, ci, begin, len, bad);          // (uniform within the group)
    if (!ok) len = 0;
    int32_t cj = -1;
    int64_t uj = 0;
    bool valid = false;
    if (sub < len) valid = sweep_entry(a, begin + sub, i, cj, uj, bad);
    if (!valid) {
        cj = -1;
        uj = 0;
    }
    // e: the weight of the group's lanes that share this lane's community (lanes without an entry share -1 and add 0)
    int64_t e = 0;
    // (a wave's row is the wave's: its length is uniform and bounds the loop; four rows of 16 lanes take all 16 steps)
    const int steps = G == 64 ? __builtin_amdgcn_readfirstlane((int)len) : G;
    for (int m = 0; m < steps; ++m) {
        const int32_t cm = __shfl(cj, m, G);
        const int64_t um = __shfl(uj, m, G);
        if (cm == cj) e += um;
    }
    const int64_t e_stay = group_sum<G>(valid && cj == ci ? uj : 0);
    const double kd = ok ? (double)a.k[i] : 0.0;
    double g = -INFINITY;
    int32_t d = INT_MAX;
    if (valid && cj != ci && is_candidate(cj, ci, a.parity)) {
        g = gain(e, kd, a.tot[cj], a.gamma, a.m2);
        d = cj;
    }
    group_best<G>(g, d);
    bool move = false;
    if (ok && sub == 0) {
        const double stay = gain(e_stay, kd, a.tot[ci] - a.k[i], a.gamma, a.m2);
        move = g > stay;
        a.c_new[i] = move ? d : ci;
    }
    const int movers = __popcll(__ballot(move));
    if ((threadIdx.x & 63) == 0 && movers) atomicAdd(a.moved, (uint32_t)movers);
    if (bad) atomicOr(a.status, bad);
}

// the block's best of every thread's (g, d); valid in thread 0
__device__ __forceinline__ void block_best(double& g, int32_t& d, double* sg, int32_t* sd)
{
    group_best<64>(g, d);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sg[wave] = g;
        sd[wave] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kThreads / 64; ++w)
            if (before(sg[w], sd[w], g, d)) {
                g = sg[w];
                d = sd[w];
            }
}

__device__ __forceinline__ void block_decide(const Sweep& a, int32_t i, int32_t ci, double kd, double g, int32_t d,
                                             int64_t e_stay)
{
    const double stay = gain(e_stay, kd, a.tot[ci] - a.k[i], a.gamma, a.m2);
    const bool move = g > stay;
    a.c_new[i] = move ? d : ci;
    if (move) atomicAdd(a.moved, 1u);
}

__global__ __launch_bounds__(kThreads) void cluster_sweep_table_kernel(Sweep a)
{
    __shared__ int32_t keys[kTableSlots];
    __shared__ u64 vals[kTableSlots];
    __shared__ double sg[kThreads / 64];
    __shared__ int32_t sd[kThreads / 64];
    __shared__ u64 s_stay;
    int32_t i = 0, ci = 0;
    int64_t begin = 0, len = 0;
    uint32_t bad = 0u;
    const bool ok = sweep_row(a, blockIdx.x, kTableRow, i, ci, begin, len, bad);     // (block-uniform)
    if (!ok) {
        if (bad && threadIdx.x == 0) atomicOr(a.status, bad);
        return;
    }
    for (int s = threadIdx.x; s < kTableSlots; s += kThreads) {
        keys[s] = -1;
        vals[s] = 0;
    }
    if (threadIdx.x == 0) s_stay = 0;
    __syncthreads();
    for (int64_t t = threadIdx.x; t < len; t += kThreads) {
        int32_t cj;
        int64_t uj;
        if (!sweep_entry(a, begin + t, i, cj, uj, bad)) continue;
        uint32_t s = ((uint32_t)cj * 2654435761u) >> 22;                 // 10 bits
        for (int probe = 0; probe < kTableSlots; ++probe) {              // (at most 512 communities: a slot is found)
            const int32_t seen = atomicCAS(&keys[s], -1, cj);
            if (seen == -1 || seen == cj) {
                atomicAdd(&vals[s], (u64)uj);
                break;
            }
            s = (s + 1) & (kTableSlots - 1);
        }
    }
    __syncthreads();
    const double kd = (double)a.k[i];
    double g = -INFINITY;
    int32_t d = INT_MAX;
    for (int s = threadIdx.x; s < kTableSlots; s += kThreads) {
        const int32_t dd = keys[s];
        if (dd < 0) continue;
        if (dd == ci) {
            s_stay = vals[s];                                            // (one slot holds c_i)
        } else if (is_candidate(dd, ci, a.parity)) {
            const double gg = gain((int64_t)vals[s], kd, a.tot[dd], a.gamma, a.m2);
            if (before(gg, dd, g, d)) {
                g = gg;
                d = dd;
            }
        }
    }
    block_best(g, d, sg, sd);                                            // (its barrier also publishes s_stay)
    if (threadIdx.x == 0) block_decide(a, i, ci, kd, g, d, (int64_t)s_stay);
    if (bad) atomicOr(a.status, bad);
}

__global__ __launch_bounds__(kThreads) void cluster_sweep_range_kernel(Sweep a)
{
    __shared__ u64 sums[kRange];
    __shared__ uint32_t present[kRange / 32];
    __shared__ double sg[kThreads / 64];
    __shared__ int32_t sd[kThreads / 64];
    __shared__ u64 s_stay;
    __shared__ int32_t s_lo, s_hi;
    int32_t i = 0, ci = 0;
    int64_t begin = 0, len = 0;
    uint32_t bad = 0u;
    const bool ok = sweep_row(a, blockIdx.x, 0, i, ci, begin, len, bad);             // (block-uniform)
    if (!ok) {
        if (bad && threadIdx.x == 0) atomicOr(a.status, bad);
        return;
    }
    if (threadIdx.x == 0) {
        s_stay = 0;
        s_lo = INT_MAX;
        s_hi = -1;
    }
    __syncthreads();
    {   // the lowest and the highest community of the row's entries
        int32_t lo = INT_MAX, hi = -1;
        for (int64_t t = threadIdx.x; t < len; t += kThreads) {
            int32_t cj;
            int64_t uj;
            if (!sweep_entry(a, begin + t, i, cj, uj, bad)) continue;
            lo = cj < lo ? cj : lo;
            hi = cj > hi ? cj : hi;
        }
        if (hi >= 0) {
            atomicMin(&s_lo, lo);
            atomicMax(&s_hi, hi);
        }
    }
    __syncthreads();
    const int64_t lowest = s_lo, highest = s_hi;
    const double kd = (double)a.k[i];
    double g = -INFINITY;
    int32_t d = INT_MAX;
    uint32_t unused = 0u;                                                // (the entries were checked in the pass above)
    for (int64_t base = lowest; base <= highest; base += kRange) {
        for (int s = threadIdx.x; s < kRange; s += kThreads) sums[s] = 0;
        if (threadIdx.x < kRange / 32) present[threadIdx.x] = 0u;
        __syncthreads();
        for (int64_t t = threadIdx.x; t < len; t += kThreads) {
            int32_t cj;
            int64_t uj;
            if (!sweep_entry(a, begin + t, i, cj, uj, unused)) continue;
            const int64_t s = (int64_t)cj - base;
            if (s < 0 || s >= kRange) continue;
            atomicAdd(&sums[s], (u64)uj);
            atomicOr(&present[s >> 5], 1u << (s & 31));
        }
        __syncthreads();
        for (int s = threadIdx.x; s < kRange; s += kThreads) {
            if (!((present[s >> 5] >> (s & 31)) & 1u)) continue;
            const int32_t dd = (int32_t)(base + s);
            if (dd == ci) {
                s_stay = sums[s];
            } else if (is_candidate(dd, ci, a.parity)) {
                const double gg = gain((int64_t)sums[s], kd, a.tot[dd], a.gamma, a.m2);
                if (before(gg, dd, g, d)) {
                    g = gg;
                    d = dd;
                }
            }
        }
        __syncthreads();
    }
    block_best(g, d, sg, sd);
    if (threadIdx.x == 0) block_decide(a, i, ci, kd, g, d, (int64_t)s_stay);
    if (bad) atomicOr(a.status, bad);
}

// -------------------------------------------------------------------------------------------------------------- totals

__global__ __launch_bounds__(kThreads) void cluster_totals_kernel(const int64_t* __restrict__ indptr,
                                                                  const int32_t* __restrict__ indices,
                                                                  const int64_t* __restrict__ u, const int64_t* __restrict__ k,
                                                                  int64_t n, int64_t nnz, const int32_t* __restrict__ c,
                                                                  u64* __restrict__ tot, u64* __restrict__ in,
                                                                  uint32_t* __restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = t / kRowLanes;
    const int sub = (int)(t % kRowLanes);
    bool ok = row < n;
    int64_t begin = 0, len = 0;
    int32_t ci = 0;
    uint32_t bad = 0u;
    if (ok) {
        ci = c[row];
        if ((uint32_t)ci >= (uint64_t)n) {
            bad |= kBadCommunity;
            ok = false;
        } else {
            row_bounds(indptr, row, nnz, begin, len, bad);
        }
    }
    int64_t acc = 0;
    for (int64_t e = begin + sub; e < begin + len; e += kRowLanes) {
        const int32_t j = indices[e];
        if ((uint32_t)j >= (uint64_t)n) {
            bad |= kBadGraph;
            continue;
        }
        if (c[j] == ci) acc += u[e];
    }
    acc = group_sum<kRowLanes>(acc);
    if (ok && sub == 0) {
        atomicAdd(&in[ci], (u64)acc);
        atomicAdd(&tot[ci], (u64)k[row]);
    }
    if (bad) atomicOr(status, bad);
}

// --------------------------------------------------------------------------------------------------------- aggregation

__global__ __launch_bounds__(kThreads) void cluster_emit_kernel(const int64_t* __restrict__ indptr,
                                                                const int32_t* __restrict__ indices, int64_t n, int64_t nnz,
                                                                const int32_t* __restrict__ cnew, int64_t n_new,
                                                                int64_t* __restrict__ keys, uint32_t* __restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t row = t / kRowLanes;
    const int sub = (int)(t % kRowLanes);
    if (row >= n) return;
    int64_t begin = 0, len = 0;
    uint32_t bad = 0u;
    row_bounds(indptr, row, nnz, begin, len, bad);
    int64_t a = cnew[row];
    if (a < 0 || a >= n_new) {
        bad |= kBadCommunity;
        a = 0;
    }
    for (int64_t e = begin + sub; e < begin + len; e += kRowLanes) {
        const int32_t j = indices[e];
        int64_t b = 0;
        if ((uint32_t)j >= (uint64_t)n) {
            bad |= kBadGraph;
        } else {
            b = cnew[j];
            if (b < 0 || b >= n_new) {
                bad |= kBadCommunity;
                b = 0;
            }
        }
        keys[e] = (a << 32) | b;
    }
    if (bad) atomicOr(status, bad);
}

__global__ __launch_bounds__(kThreads) void cluster_fold_kernel(const int64_t* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                                const int64_t* __restrict__ pos, const int64_t* __restrict__ u,
                                                                int64_t M, int64_t n_new, int64_t nnz_new,
                                                                int64_t* __restrict__ indptr, int32_t* __restrict__ indices,
                                                                u64* __restrict__ u_new, uint32_t* __restrict__ status)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads * kFoldRun;
    uint32_t bad = 0u;
    for (int64_t p0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kFoldRun; p0 < M; p0 += stride) {
        int64_t held = -1;              // the output entry whose sum this thread holds
        u64 acc = 0;
        const int64_t p1 = p0 + kFoldRun < M ? p0 + kFoldRun : M;
        for (int64_t p = p0; p < p1; ++p) {
            const int64_t o = pos[p] - 1;
            const u64 src = (u64)perm[p];
            if (o < 0 || o >= nnz_new || src >= (u64)M) {
                bad |= PROSSTT_AMD_CLUSTER_BAD_SORT;
                continue;
            }
            if (o != held) {
                if (held >= 0) atomicAdd(&u_new[held], acc);
                held = o;
                acc = 0;
            }
            acc += (u64)u[src];
            const int64_t key = sorted[p];
            const int64_t prior = p > 0 ? sorted[p - 1] : int64_t(-1);
            if (p == 0 || prior != key) {                                // the head of its run
                indices[o] = (int32_t)(uint32_t)key;
                // (the two indptr loops of sorted_runs.h's fold, written out: as shared functions they changed this kernel)
                const int64_t row = key >> 32, prev = p > 0 ? prior >> 32 : int64_t(-1);
                for (int64_t r = prev < -1 ? 0 : prev + 1; r <= row && r <= n_new; ++r) indptr[r] = o;
            }
            if (p == M - 1) {                                            // the last entry closes every row behind it
                const int64_t row = key >> 32;
                for (int64_t r = row < -1 ? 0 : row + 1; r <= n_new; ++r) indptr[r] = nnz_new;
            }
        }
        if (held >= 0) atomicAdd(&u_new[held], acc);
    }
    if (bad) atomicOr(status, bad);
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_cluster_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_cluster_workspace_bytes(int64_t n, int64_t nnz, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_level(n, nnz)) return rc;
    *bytes = pad((size_t)nnz * 8);
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_cluster_quantize(void* stream, const int64_t* indptr, const int32_t* indices, const double* W,
                                            int64_t N, int64_t nnz, int64_t* u, int64_t* k, uint32_t* status) try
{
    if (int rc = check_level(N, nnz)) return rc;
    if (N < 3) return fail(ABI_EINVAL, "need 3 <= N (got %lld)", (long long)N);
    if (nnz >= (int64_t(1) << 30)) return fail(ABI_EINVAL, "need nnz < 2^30 (got %lld)", (long long)nnz);
    if (!indptr || !indices || !W || !u || !k || !status) return fail(ABI_EINVAL, "NULL argument");
    cluster_quantize_kernel<<<dim3((unsigned)cdiv(N, kThreads / kRowLanes)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        indptr, W, N, nnz, u, k, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_cluster_sweep(void* stream, const int64_t* indptr, const int32_t* indices, const int64_t* u,
                                         const int64_t* k, int64_t n, int64_t nnz, const int32_t* rows, int64_t n16,
                                         int64_t n64, int64_t n512, const int32_t* c, const int64_t* tot, int64_t M2,
                                         double gamma, int32_t parity, int32_t path, int32_t* c_new, uint32_t* moved,
                                         uint32_t* status) try
{
    if (int rc = check_level(n, nnz)) return rc;
    if (!indptr || !indices || !u || !k || !rows || !c || !tot || !c_new || !moved || !status)
        return fail(ABI_EINVAL, "NULL argument");
    if (c_new == c) return fail(ABI_EINVAL, "c_new must not alias c");
    if (!(0 <= n16 && n16 <= n64 && n64 <= n512 && n512 <= n))
        return fail(ABI_EINVAL, "need 0 <= n16 <= n64 <= n512 <= n (got %lld, %lld, %lld)", (long long)n16, (long long)n64,
                    (long long)n512);
    if (M2 < 1) return fail(ABI_EINVAL, "need M2 >= 1 (got %lld)", (long long)M2);
    if (!(gamma > 0.0) || gamma == INFINITY) return fail(ABI_EINVAL, "the resolution must be a positive finite number");
    if (parity != 0 && parity != 1) return fail(ABI_EINVAL, "parity must be 0 or 1 (got %d)", (int)parity);
    if (path < 0 || path > PROSSTT_AMD_CLUSTER_PATH_RANGE) return fail(ABI_EINVAL, "path must be 0 .. 4 (got %d)", (int)path);
    // rows[bound[p - 1] .. bound[p]) go to path p
    int64_t bound[5] = {0, n16, n64, n512, n};
    if (path != PROSSTT_AMD_CLUSTER_PATH_AUTO) {
        if (bound[path] != n)
            return fail(ABI_EINVAL, "path %d holds rows of at most %d entries: %lld rows are longer", (int)path,
                        path == 1 ? 16 : (path == 2 ? 64 : kTableRow), (long long)(n - bound[path]));
        for (int p = 0; p < 5; ++p) bound[p] = p < path ? 0 : n;
    }
    Sweep a{indptr, indices, u, k, rows, c, tot, c_new, moved, status, n, nnz, 0, 0, gamma, (double)M2, (int)parity};
    hipStream_t st = (hipStream_t)stream;
    for (int p = 1; p <= 4; ++p) {
        a.first = bound[p - 1];
        a.count = bound[p] - bound[p - 1];
        if (a.count == 0) continue;
        const dim3 block(kThreads);
        switch (p) {
        case 1: cluster_sweep_group_kernel<16><<<dim3((unsigned)cdiv(a.count, kThreads / 16)), block, 0, st>>>(a); break;
        case 2: cluster_sweep_group_kernel<64><<<dim3((unsigned)cdiv(a.count, kThreads / 64)), block, 0, st>>>(a); break;
        case 3: cluster_sweep_table_kernel<<<dim3((unsigned)a.count), block, 0, st>>>(a); break;
        default: cluster_sweep_range_kernel<<<dim3((unsigned)a.count), block, 0, st>>>(a); break;
        }
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_cluster_totals(void* stream, const int64_t* indptr, const int32_t* indices, const int64_t* u,
                                          const int64_t* k, int64_t n, int64_t nnz, const int32_t* c, int64_t* tot,
                                          int64_t* in, uint32_t* status) try
{
    if (int rc = check_level(n, nnz)) return rc;
    if (!indptr || !indices || !u || !k || !c || !tot || !in || !status) return fail(ABI_EINVAL, "NULL argument");
    if (tot == in) return fail(ABI_EINVAL, "tot must not alias in");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(tot, 0, (size_t)n * 8, st));
    HIP_TRY(hipMemsetAsync(in, 0, (size_t)n * 8, st));
    cluster_totals_kernel<<<dim3((unsigned)cdiv(n, kThreads / kRowLanes)), dim3(kThreads), 0, st>>>(
        indptr, indices, u, k, n, nnz, c, (u64*)tot, (u64*)in, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_cluster_aggregate_emit(void* stream, const int64_t* indptr, const int32_t* indices, int64_t n,
                                                  int64_t nnz, const int32_t* cnew, int64_t n_new, void* ws,
                                                  uint64_t ws_bytes, uint32_t* status) try
{
    if (int rc = check_level(n, nnz)) return rc;
    if (n_new < 1 || n_new > n) return fail(ABI_EINVAL, "need 1 <= n_new <= n (got %lld)", (long long)n_new);
    if (!indptr || !indices || !cnew || !status) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_workspace(ws, ws_bytes, pad((size_t)nnz * 8))) return rc;
    cluster_emit_kernel<<<dim3((unsigned)cdiv(n, kThreads / kRowLanes)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        indptr, indices, n, nnz, cnew, n_new, (int64_t*)ws, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_cluster_aggregate_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm,
                                                  const int64_t* pos, const int64_t* u, int64_t nnz, int64_t n_new,
                                                  int64_t nnz_new, int64_t* indptr_new, int32_t* indices_new, int64_t* u_new,
                                                  uint32_t* status) try
{
    if (int rc = check_level(n_new, nnz)) return rc;
    if (nnz_new < 1 || nnz_new > nnz) return fail(ABI_EINVAL, "need 1 <= nnz_new <= nnz (got %lld)", (long long)nnz_new);
    if (!sorted_keys || !perm || !pos || !u || !indptr_new || !indices_new || !u_new || !status)
        return fail(ABI_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(u_new, 0, (size_t)nnz_new * 8, st));
    cluster_fold_kernel<<<dim3(stride_blocks(cdiv(nnz, kFoldRun))), dim3(kThreads), 0, st>>>(
        sorted_keys, perm, pos, u, nnz, n_new, nnz_new, indptr_new, indices_new, (u64*)u_new, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
