// libprosstt_amd_tsne.so -- exact t-SNE of the cells (include/prosstt_amd_tsne.h has the definition).  256 threads = 4 waves
// per block, 64-bit offsets, no scratch and no atomic: a sum is a lane's own ascending partial sum followed by a fixed xor
// shuffle tree, in which both lanes of a pair add the same two numbers, so all lanes of a wave hold the same bits.
//   tsne_affinities_kernel   one wave per row.  The row's k <= 1024 shifted distances stay in LDS, lane-strided (entry c is
//                            lane c & 63's: kept in registers, the unrolled exp, log and division of 16 slots spilled
//                            scalar registers).  Each of the 64 evaluations of H is two wave reductions.  Checks the values.
//   tsne_fold_kernel         sorted_runs.h's fold of the sorted entries into P: a run adds up, and 2 N divides the sum.
//   tsne_pair_kernel<C, ABS> the repulsion.  A block owns 512 rows (two per thread, 256 apart, so that two independent
//                            chains are in flight) and one slab of column tiles.  A tile's positions go through LDS, and
//                            every lane reads the same column at a time (a broadcast read).  Ten vector instructions per
//                            pair at C = 2.  ABS also sums |q q delta|.
//   tsne_zsum_kernel         z_i over the slabs and their sum per block of rows.
//   tsne_row_kernel<C, STEP> one wave per row: the attraction over the row's entries of P, R_i over the slabs, Z over the
//                            blocks of tsne_zsum_kernel, the gradient; STEP applies the update rule instead of storing it.
//   tsne_objective_kernel<C> one wave per row.
#include "../../../include/prosstt_amd_tsne.h"

#define ABI_EINVAL PROSSTT_AMD_TSNE_EINVAL
#define ABI_EHIP PROSSTT_AMD_TSNE_EHIP
#include "../abi_util.h"
#include "../graph_util.h"                // the refusals and grid rules of the graph libraries, symmetrize_fold
#include "../sorted_runs.h"               // fold_sorted_runs
#include "../wave_reduce.h"               // group_sum, wave_sum, wave_min

#include <cmath>

namespace {

constexpr int kMaxK = 1024;
constexpr int kBisections = 64;
constexpr int kTile = PROSSTT_AMD_TSNE_TILE;
constexpr int kMaxSlabs = PROSSTT_AMD_TSNE_MAX_SLABS;
constexpr int kRowsPerThread = 2;
constexpr int kBlockRows = kThreads * kRowsPerThread;
constexpr int kZBlocks = 256;                  // at most this many partial sums of Z
constexpr int32_t kMaxIteration = 1 << 30;

// How the repulsion is cut and where its partial sums lie in the workspace.
struct Plan {
    int slabs = 0;
    int64_t tiles_per_slab = 0, row_blocks = 0;
    int zblocks = 0;
    int64_t zblock_rows = 0;
    size_t z_off = 0, r_off = 0, abs_off = 0, zb_off = 0, bytes = 0;
};

Plan make_plan(int64_t N, int c, int slabs)
{
    Plan p;
    const int64_t tiles = cdiv(N, kTile);
    p.row_blocks = cdiv(N, kBlockRows);
    p.slabs = slabs ? slabs : default_slabs(p.row_blocks, tiles, kMaxSlabs);
    p.tiles_per_slab = cdiv(tiles, p.slabs);
    p.zblocks = (int)clamp64(cdiv(N, 4 * kThreads), 1, kZBlocks);
    p.zblock_rows = cdiv(cdiv(N, p.zblocks), kThreads) * kThreads;
    const size_t per_row = (size_t)p.slabs * (size_t)N * 8;
    p.z_off = 0;
    p.r_off = p.z_off + pad(per_row);
    p.abs_off = p.r_off + pad(per_row * c);
    p.zb_off = p.abs_off + pad(per_row * c);
    p.bytes = p.zb_off + pad((size_t)kZBlocks * 8);
    return p;
}

// ---------------------------------------------------------------------------------------------------------- affinities

__global__ __launch_bounds__(kThreads) void tsne_affinities_kernel(const int32_t* __restrict__ index,
                                                                   const float* __restrict__ sqdist, int64_t N, int k,
                                                                   double target, double* __restrict__ cond,
                                                                   double* __restrict__ beta_out, uint8_t* __restrict__ status)
{
    // the shifted distances of the block's four rows; a lane reads back only what it wrote itself, so nothing synchronises
    __shared__ double shifted[kThreads / 64][kMaxK];
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                               // wave-uniform
    double* g = shifted[threadIdx.x >> 6];
    const int64_t base = i * k;
    const double inf = INFINITY;

    double dmin = inf;
    bool bad_index = false, bad_self = false, bad_distance = false;
    for (int c = lane; c < k; c += 64) {
        const int64_t j = index[base + c];
        float d2 = sqdist[base + c];
        if (j < 0 || j >= N) bad_index = true;
        else if (j == i) bad_self = true;
        if (!(d2 >= 0.0f) || d2 == INFINITY) {
            bad_distance = true;
            d2 = 0.0f;
        }
        g[c] = (double)d2;
        dmin = fmin(dmin, (double)d2);
    }
    // every writer of a byte writes the same 1: no atomic
    if (bad_index) status[0] = 1;
    if (bad_self) status[1] = 1;
    if (bad_distance) status[2] = 1;
    dmin = wave_min(dmin);
    for (int c = lane; c < k; c += 64) g[c] -= dmin;

    double lo = 0.0, hi = inf, beta = 1.0, S;
    for (int it = 0;; ++it) {                         // (one copy of the evaluation: the last trip is that of the output)
        double s = 0.0, gp = 0.0;
        for (int c = lane; c < k; c += 64) {
            const double p = exp(-beta * g[c]);
            s += p;
            gp += g[c] * p;
        }
        S = wave_sum(s);
        if (it == kBisections) break;
        if (log(S) + beta * wave_sum(gp) / S > target) {
            lo = beta;
            beta = hi == inf ? 2 * beta : (lo + hi) / 2;
        } else {
            hi = beta;
            beta = (lo + hi) / 2;
        }
    }
    for (int c = lane; c < k; c += 64) cond[base + c] = exp(-beta * g[c]) / S;
    if (lane == 0) beta_out[i] = beta;
}

// ------------------------------------------------------------------------------------------------------------- fold

__global__ __launch_bounds__(kThreads) void tsne_fold_kernel(const int64_t* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                             const int64_t* __restrict__ pos, const double* __restrict__ vals,
                                                             int64_t M, int64_t N, int64_t nnz, int64_t* __restrict__ indptr,
                                                             int32_t* __restrict__ indices, double* __restrict__ data)
{
    const double twice_n = 2.0 * (double)N;
    fold_sorted_runs(
        sorted, perm, pos, vals, M, N, nnz, indptr, indices, data, [](double w, double b) { return w + b; },
        [twice_n](double w) { return w / twice_n; });
}

// -------------------------------------------------------------------------------------------------------- repulsion

// q of the definition and delta of the pair
template <int C>
__device__ __forceinline__ float pair_q(const float (&yi)[C], const float (&yj)[C], float (&delta)[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) delta[c] = yi[c] - yj[c];
    float d2 = delta[0] * delta[0];
#pragma unroll
    for (int c = 1; c < C; ++c) d2 = fmaf(delta[c], delta[c], d2);
    return __builtin_amdgcn_rcpf(1.0f + d2);
}

template <int C, bool ABS>
__global__ __launch_bounds__(kThreads) void tsne_pair_kernel(const float* __restrict__ y, int64_t N, int64_t tiles_per_slab,
                                                             double* __restrict__ zpart, double* __restrict__ rpart,
                                                             double* __restrict__ apart)
{
    __shared__ float cols[kTile * C];
    const int64_t slab = blockIdx.y;
    int64_t row[kRowsPerThread];
    float yi[kRowsPerThread][C];
    double zacc[kRowsPerThread], racc[kRowsPerThread][C], aacc[kRowsPerThread][C];
#pragma unroll
    for (int u = 0; u < kRowsPerThread; ++u) {
        row[u] = (int64_t)blockIdx.x * kBlockRows + u * kThreads + threadIdx.x;
        zacc[u] = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            yi[u][c] = row[u] < N ? y[row[u] * C + c] : 0.0f;
            racc[u][c] = 0.0;
            aacc[u][c] = 0.0;
        }
    }
    const int64_t tiles = (N + kTile - 1) / kTile;
    const int64_t tile_begin = slab * tiles_per_slab;
    const int64_t tile_end = tile_begin + tiles_per_slab < tiles ? tile_begin + tiles_per_slab : tiles;
    for (int64_t tile = tile_begin; tile < tile_end; ++tile) {
        const int64_t col0 = tile * kTile;
        const int cnt = (int)(N - col0 < kTile ? N - col0 : kTile);
        __syncthreads();                              // the previous tile has been read
        for (int t = threadIdx.x; t < cnt * C; t += kThreads) cols[t] = y[col0 * C + t];
        __syncthreads();
        float z[kRowsPerThread], r[kRowsPerThread][C], a[kRowsPerThread][C];
#pragma unroll
        for (int u = 0; u < kRowsPerThread; ++u) {
            z[u] = 0.0f;
#pragma unroll
            for (int c = 0; c < C; ++c) r[u][c] = a[u][c] = 0.0f;
        }
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            float yj[C];
#pragma unroll
            for (int c = 0; c < C; ++c) yj[c] = cols[j * C + c];
#pragma unroll
            for (int u = 0; u < kRowsPerThread; ++u) {
                float delta[C];
                const float q = pair_q<C>(yi[u], yj, delta);
                z[u] += q;
                const float q2 = q * q;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    r[u][c] = fmaf(q2, delta[c], r[u][c]);
                    if (ABS) a[u][c] += fabsf(q2 * delta[c]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRowsPerThread; ++u) {
            zacc[u] += (double)z[u];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                racc[u][c] += (double)r[u][c];
                if (ABS) aacc[u][c] += (double)a[u][c];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kRowsPerThread; ++u) {
        if (row[u] >= N) continue;
        const int64_t at = slab * N + row[u];
        zpart[at] = zacc[u];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            rpart[at * C + c] = racc[u][c];
            if (ABS) apart[at * C + c] = aacc[u][c];
        }
    }
}

__global__ __launch_bounds__(kThreads) void tsne_zsum_kernel(const double* __restrict__ zpart, int64_t N, int slabs,
                                                             int64_t rows_per_block, double* __restrict__ zblock)
{
    __shared__ double waves[kThreads / 64];
    const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
    const int64_t end = begin + rows_per_block < N ? begin + rows_per_block : N;
    double acc = 0.0;
    for (int64_t i = begin + threadIdx.x; i < end; i += kThreads) {
        double zi = 0.0;
        for (int s = 0; s < slabs; ++s) zi += zpart[(int64_t)s * N + i];
        acc += zi;
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) zblock[blockIdx.x] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

// ---------------------------------------------------------------------------------------------------------------- rows

struct StepParams {
    float x, mu, eta;
};

template <int C, bool STEP>
__global__ __launch_bounds__(kThreads) void tsne_row_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                            const double* __restrict__ P, const float* __restrict__ y, int64_t N,
                                                            StepParams sp, int slabs, const double* __restrict__ rpart,
                                                            const double* __restrict__ apart, const double* __restrict__ zblock,
                                                            int zblocks, float* __restrict__ grad, double* __restrict__ zout,
                                                            double* __restrict__ rep_abs, float* __restrict__ y1,
                                                            float* __restrict__ update, float* __restrict__ gains)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                               // wave-uniform
    double zsum = 0.0;
    for (int b = lane; b < zblocks; b += 64) zsum += zblock[b];
    const double Z = wave_sum(zsum) - (double)N;
    if (!STEP && i == 0 && lane == 0) *zout = Z;

    float yi[C], att[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        yi[c] = y[i * C + c];
        att[c] = 0.0f;
    }
    const int64_t end = indptr[i + 1];
    for (int64_t e = indptr[i] + lane; e < end; e += 64) {
        const int64_t j = indices[e];
        float yj[C], delta[C];
#pragma unroll
        for (int c = 0; c < C; ++c) yj[c] = y[j * C + c];
        const float pq = (float)P[e] * pair_q<C>(yi, yj, delta);
#pragma unroll
        for (int c = 0; c < C; ++c) att[c] += pq * delta[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) att[c] = wave_sum(att[c]);
    if (lane >= C) return;
    const float a = lane == 0 ? att[0] : (lane == 1 ? att[1] : att[C - 1]);
    const int64_t at = i * C + lane;
    double R = 0.0;
    for (int s = 0; s < slabs; ++s) R += rpart[((int64_t)s * N) * C + at];
    const float rep = (float)(R / Z);
    const float g = 4.0f * (sp.x * a - rep);
    if (!STEP) {
        grad[at] = g;
        if (rep_abs) {
            double A = 0.0;
            for (int s = 0; s < slabs; ++s) A += apart[((int64_t)s * N) * C + at];
            rep_abs[at] = A;
        }
    } else {
        float u = update[at], gain = gains[at];
        gain = u * g < 0.0f ? gain + 0.2f : gain * 0.8f;
        gain = fmaxf(gain, 0.01f);
        u = sp.mu * u - (sp.eta * gain) * g;
        update[at] = u;
        gains[at] = gain;
        y1[at] = y[at] + u;
    }
}

template <int C>
__global__ __launch_bounds__(kThreads) void tsne_objective_kernel(const int64_t* __restrict__ indptr,
                                                                  const int32_t* __restrict__ indices,
                                                                  const double* __restrict__ P, const float* __restrict__ y,
                                                                  int64_t N, double* __restrict__ rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= N) return;                               // wave-uniform
    float yi[C];
#pragma unroll
    for (int c = 0; c < C; ++c) yi[c] = y[i * C + c];
    double acc = 0.0;
    const int64_t end = indptr[i + 1];
    for (int64_t e = indptr[i] + lane; e < end; e += 64) {
        const int64_t j = indices[e];
        const double p = P[e];
        float d2 = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float delta = yi[c] - y[j * C + c];
            d2 = c == 0 ? delta * delta : fmaf(delta, delta, d2);
        }
        acc += p > 0.0 ? p * (log(p) + log1p((double)d2)) : 0.0;
    }
    acc = wave_sum(acc);
    if (lane == 0) rows[i] = acc;
}

// the refusals that _gradient and _iterations share; the plan on success
int check_descent(int64_t N, int64_t nnz, int32_t c, int32_t slabs, const void* ws, uint64_t ws_bytes, Plan& plan)
{
    if (int rc = check_csr(N, nnz, c)) return rc;
    if (slabs < 0 || slabs > kMaxSlabs) return fail(ABI_EINVAL, "need 0 <= slabs <= %d (got %d)", kMaxSlabs, (int)slabs);
    plan = make_plan(N, c, slabs);
    return check_workspace(ws, ws_bytes, plan.bytes);
}

bool positive_finite(double v) { return v > 0.0 && std::isfinite(v); }

// the repulsion's partial sums and the blocks of Z for the positions y
template <int C>
int enqueue_repulsion(hipStream_t st, const Plan& p, const float* y, int64_t N, char* ws, bool with_abs)
{
    const dim3 grid((unsigned)p.row_blocks, (unsigned)p.slabs), block(kThreads);
    double* zpart = (double*)(ws + p.z_off);
    double* rpart = (double*)(ws + p.r_off);
    double* apart = (double*)(ws + p.abs_off);
    if (with_abs) tsne_pair_kernel<C, true><<<grid, block, 0, st>>>(y, N, p.tiles_per_slab, zpart, rpart, apart);
    else tsne_pair_kernel<C, false><<<grid, block, 0, st>>>(y, N, p.tiles_per_slab, zpart, rpart, apart);
    HIP_TRY(hipGetLastError());
    tsne_zsum_kernel<<<dim3((unsigned)p.zblocks), block, 0, st>>>(zpart, N, p.slabs, p.zblock_rows, (double*)(ws + p.zb_off));
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int C>
int enqueue_gradient(hipStream_t st, const Plan& p, const int64_t* indptr, const int32_t* indices, const double* P,
                     const float* y, int64_t N, float x, char* ws, float* grad, double* z, double* rep_abs)
{
    if (int rc = enqueue_repulsion<C>(st, p, y, N, ws, rep_abs != nullptr)) return rc;
    const StepParams sp{x, 0.0f, 0.0f};
    tsne_row_kernel<C, false><<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, st>>>(
        indptr, indices, P, y, N, sp, p.slabs, (const double*)(ws + p.r_off), (const double*)(ws + p.abs_off),
        (const double*)(ws + p.zb_off), p.zblocks, grad, z, rep_abs, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int C>
int enqueue_iterations(hipStream_t st, const Plan& p, const int64_t* indptr, const int32_t* indices, const double* P,
                       int64_t N, float* y0, float* y1, float* update, float* gains, int it_begin, int it_end,
                       int exploration, float early, float eta, char* ws)
{
    float* src = y0;
    float* dst = y1;
    for (int n = it_begin; n < it_end; ++n) {
        if (int rc = enqueue_repulsion<C>(st, p, src, N, ws, false)) return rc;
        const StepParams sp{n < exploration ? early : 1.0f, n < exploration ? 0.5f : 0.8f, eta};
        tsne_row_kernel<C, true><<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, st>>>(
            indptr, indices, P, src, N, sp, p.slabs, (const double*)(ws + p.r_off), nullptr, (const double*)(ws + p.zb_off),
            p.zblocks, nullptr, nullptr, nullptr, dst, update, gains);
        HIP_TRY(hipGetLastError());
        float* was = src;
        src = dst;
        dst = was;
    }
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_tsne_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_tsne_workspace_bytes(int64_t N, int32_t c, int32_t slabs, uint64_t* bytes) try
{
    if (!bytes) return fail(ABI_EINVAL, "NULL argument");
    if (int rc = check_csr(N, 0, c)) return rc;
    if (slabs < 0 || slabs > kMaxSlabs) return fail(ABI_EINVAL, "need 0 <= slabs <= %d (got %d)", kMaxSlabs, (int)slabs);
    *bytes = make_plan(N, c, slabs).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_tsne_affinities(void* stream, const int32_t* index, const float* sqdist, int64_t N, int64_t k,
                                           double perplexity, double* cond, double* beta, uint32_t* status) try
{
    if (int rc = check_sizes(N, k, kMaxK)) return rc;
    if (!(perplexity > 1.0) || !(perplexity < (double)k))
        return fail(ABI_EINVAL, "need 1 < perplexity < k = %lld (got %g)", (long long)k, perplexity);
    if (!index || !sqdist || !cond || !beta || !status) return fail(ABI_EINVAL, "NULL argument");
    tsne_affinities_kernel<<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        index, sqdist, N, (int)k, std::log(perplexity), cond, beta, (uint8_t*)status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_tsne_symmetrize_fold(void* stream, const int64_t* sorted_keys, const int64_t* perm,
                                                const int64_t* pos, int64_t N, int64_t k, int64_t nnz, const void* ws,
                                                uint64_t ws_bytes, int64_t* indptr, int32_t* indices, double* data) try
{
    return symmetrize_fold(tsne_fold_kernel, kMaxK, stream, sorted_keys, perm, pos, N, k, nnz, ws, ws_bytes, indptr, indices,
                           data);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_tsne_gradient(void* stream, const int64_t* indptr, const int32_t* indices, const double* P,
                                         int64_t N, int64_t nnz, int32_t c, const float* y, double exaggeration, int32_t slabs,
                                         void* ws, uint64_t ws_bytes, float* grad, double* z, double* rep_abs) try
{
    Plan plan;
    if (int rc = check_descent(N, nnz, c, slabs, ws, ws_bytes, plan)) return rc;
    if (!positive_finite(exaggeration)) return fail(ABI_EINVAL, "need a finite exaggeration > 0 (got %g)", exaggeration);
    if (!indptr || !indices || !P || !y || !grad || !z) return fail(ABI_EINVAL, "NULL argument");
    if ((const void*)grad == (const void*)y) return fail(ABI_EINVAL, "grad must not alias y");
    hipStream_t st = (hipStream_t)stream;
    if (c == 2) return enqueue_gradient<2>(st, plan, indptr, indices, P, y, N, (float)exaggeration, (char*)ws, grad, z, rep_abs);
    return enqueue_gradient<3>(st, plan, indptr, indices, P, y, N, (float)exaggeration, (char*)ws, grad, z, rep_abs);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_tsne_iterations(void* stream, const int64_t* indptr, const int32_t* indices, const double* P,
                                           int64_t N, int64_t nnz, int32_t c, float* y0, float* y1, float* update, float* gains,
                                           int32_t it_begin, int32_t it_end, int32_t exploration, double early_exaggeration,
                                           double learning_rate, int32_t slabs, void* ws, uint64_t ws_bytes) try
{
    Plan plan;
    if (int rc = check_descent(N, nnz, c, slabs, ws, ws_bytes, plan)) return rc;
    if (it_begin < 0 || it_begin > it_end || it_end > kMaxIteration)
        return fail(ABI_EINVAL, "need 0 <= it_begin <= it_end <= 2^30 (got %d, %d)", (int)it_begin, (int)it_end);
    if (exploration < 0) return fail(ABI_EINVAL, "need exploration >= 0 (got %d)", (int)exploration);
    if (!positive_finite(early_exaggeration) || !positive_finite(learning_rate))
        return fail(ABI_EINVAL, "need finite early_exaggeration > 0 and learning_rate > 0 (got %g, %g)", early_exaggeration,
                    learning_rate);
    if (!indptr || !indices || !P || !y0 || !y1 || !update || !gains) return fail(ABI_EINVAL, "NULL argument");
    if (y0 == y1 || update == gains || update == y0 || update == y1 || gains == y0 || gains == y1)
        return fail(ABI_EINVAL, "y0, y1, update and gains must not alias each other");
    hipStream_t st = (hipStream_t)stream;
    if (c == 2)
        return enqueue_iterations<2>(st, plan, indptr, indices, P, N, y0, y1, update, gains, it_begin, it_end, exploration,
                                     (float)early_exaggeration, (float)learning_rate, (char*)ws);
    return enqueue_iterations<3>(st, plan, indptr, indices, P, N, y0, y1, update, gains, it_begin, it_end, exploration,
                                 (float)early_exaggeration, (float)learning_rate, (char*)ws);
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_tsne_objective(void* stream, const int64_t* indptr, const int32_t* indices, const double* P,
                                          int64_t N, int64_t nnz, int32_t c, const float* y, double* rows) try
{
    if (int rc = check_csr(N, nnz, c)) return rc;
    if (!indptr || !indices || !P || !y || !rows) return fail(ABI_EINVAL, "NULL argument");
    hipStream_t st = (hipStream_t)stream;
    if (c == 2) tsne_objective_kernel<2><<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, st>>>(indptr, indices, P, y, N, rows);
    else tsne_objective_kernel<3><<<dim3(wave_per_row_blocks(N)), dim3(kThreads), 0, st>>>(indptr, indices, P, y, N, rows);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
