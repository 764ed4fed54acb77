// libprosstt_amd_regress.so -- the quasi-score, the information (or the meat) and the quasi-log-likelihood of a per-gene
// regression of a device count matrix on a design (include/prosstt_amd_regress.h holds the definition; DESIGN section 31
// the reasons).
//
// The arithmetic of an entry, the order of the sums, their split over blockIdx.z (ACC; ACC = 0 adds Q and used), the two
// tables of factors and the slabs are quasi_device.h's, which factors shares.  What regress adds:
//
// Kernels (256 threads = 4 waves each)
//   regress_pass_kernel  a column kernel (column_device.h: a block owns a strip of 256 genes and a range of rows, a lane ONE
//                        gene; <VEC = true> stages tiles of 8 rows through LDS in 16-byte loads, <VEC = false> and the
//                        last, partial strip take 4-byte loads); the gene's coefficients, parameters and ACC sums stay in
//                        registers across the rows.
//                        What is uniform over the block is formed once per tile of 8 rows and read from LDS by every
//                        lane at one address: the row's size factor and its logarithm, whether the row is used, its
//                        design row, and for each of the block's sums its design factor (D_j for a sum of U, the rounded
//                        product D_j D_k for one of I).  With ACC = 32 that is one factor per thread and tile.
//                        `meat` puts u u in w's place in the sums of I.
//   regress_finish_kernel  quasi_finish over the row blocks
// No atomics but the OR of a status bit.
#include "../../../include/prosstt_amd_regress.h"

#define ABI_EINVAL PROSSTT_AMD_REGRESS_EINVAL
#define ABI_EHIP PROSSTT_AMD_REGRESS_EHIP
#include "../abi_util.h"
#include "../column_device.h"
#include "../quasi_device.h"

namespace {

constexpr int kMaxP = PROSSTT_AMD_REGRESS_MAX_P;
constexpr int kMaxSums = kMaxP + kMaxP * (kMaxP + 1) / 2;      // 152
static_assert(PROSSTT_AMD_REGRESS_SPLIT_16_MAX_SUMS == kQuasiSplit16MaxSums, "the header states the shared rule");

struct Geometry {
    int64_t strips = 0, row_blocks = 0, rows_per_block = 0, sums = 0;
    QuasiSlabs at;                          // the slabs [row_blocks][sums + 1][G] (U, I, then Q) and [row_blocks][G]
};

// The blocking of the rows depends on (N, strips) alone, never on p or the split.
Geometry geometry(int64_t N, int64_t G, int64_t p)
{
    Geometry g;
    g.strips = cdiv(G, kColumn);
    g.sums = quasi_sums(p);
    const RowBlocking b = row_blocking(N, g.strips);
    g.rows_per_block = b.rows_per_block;
    g.row_blocks = b.row_blocks;
    g.at = quasi_slabs(g.row_blocks, g.sums, G);
    return g;
}

template <bool VEC, int ACC>
__global__ __launch_bounds__(kThreads) void regress_pass_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G, int64_t ld,
                                                                const double* __restrict__ size,
                                                                const int32_t* __restrict__ labels, int32_t K,
                                                                const double* __restrict__ design, int64_t ldd, int32_t p,
                                                                const double* __restrict__ coef,
                                                                const double* __restrict__ alpha,
                                                                const double* __restrict__ beta, int32_t meat,
                                                                int64_t rows_per_block, double* __restrict__ slab,
                                                                uint32_t* __restrict__ usedslab, uint32_t* __restrict__ status)
{
    constexpr bool QPASS = ACC == 0;                      // this instantiation adds Q and used, and no sum of (U, I)
    constexpr int SLOTS = QPASS ? 1 : ACC;
    static_assert(kThreads % SLOTS == 0 && kColumnTile * SLOTS <= kThreads, "a thread forms at most one factor of a tile, of one sum");
    __shared__ int32_t tile[VEC ? kColumnTile : 1][kColumn];
    __shared__ double s_size[kColumnTile], s_logs[kColumnTile];
    __shared__ int32_t s_use[kColumnTile];
    __shared__ double s_design[kColumnTile][kMaxP];
    __shared__ double s_factor[kColumnTile][SLOTS], s_second[kColumnTile][SLOTS];
    const int sums = p + p * (p + 1) / 2;
    const auto [a0, na, nu, mixed] = quasi_block_sums<ACC>(p, sums);      // the block's first sum, how many, how many of U
    // (below the sums' bookkeeping: formed above it, the row loops of the aligned kernels name other scalar registers)
    const ColumnLane lane = column_lane<VEC>(N, G, rows_per_block);
    const int tid = lane.tid;
    const int64_t g = lane.g;
    const bool mine = lane.mine;

    // The gene's parameters and coefficients are judged HERE, before any arithmetic on them (the header's rule).
    uint32_t flags = 0;
    double a = 0.0, b = 2.0;
    double c[kMaxP], acc[SLOTS];
    if (mine) {
        const double av = alpha[g], bv = beta[g];
        if (column_admissible(av, bv)) {
            a = av;
            b = bv;
        } else {
            flags |= PROSSTT_AMD_REGRESS_PARAMETER;
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxP; ++j) {
        c[j] = 0.0;
        if (mine && j < p) {
            const double cv = coef[(int64_t)j * G + g];
            if (__builtin_fabs(cv) <= kBig)
                c[j] = cv;
            else
                flags |= PROSSTT_AMD_REGRESS_COEFFICIENT;
        }
    }
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) acc[i] = 0.0;
    double logb = 0.0;
    if constexpr (QPASS) logb = log(b);
    double q = 0.0;
    uint32_t used = 0;
    int32_t neg = 0;

    // the sum whose factors this thread forms for the tiles (thread tid: row tid / ACC of the tile, sum a0 + tid % ACC):
    // fj == fk for a sum of U (the factor is D[fj]), fj <= fk for one of I (D[fj] D[fk]), fj < 0 beyond the last sum
    // (quasi_device.h's order of the sums, written out: DESIGN section 36)
    const int frow = tid / SLOTS, fslot = tid % SLOTS;
    int fj = -1, fk = -1;
    bool fpair = false;
    if (frow < kColumnTile && fslot < na) {
        const int s = a0 + fslot;
        if (s < p) {
            fj = fk = s;
        } else {
            int t = s - p, j = 0;
            while (t >= p - j) {
                t -= p - j;
                ++j;
            }
            fj = j;
            fk = j + t;
            fpair = true;
        }
    }

    // where the lane's sums go, formed here so that the loop need not keep the kernel's arguments for it (in vector
    // registers from here on; kept as scalar arguments, some of them spill)
    const size_t gat = (size_t)(mine ? g : 0);
    double* sums_out = slab + ((size_t)blockIdx.y * (size_t)(sums + 1) + (size_t)a0) * (size_t)G + gat;
    double* q_out = slab + ((size_t)blockIdx.y * (size_t)(sums + 1) + (size_t)sums) * (size_t)G + gat;
    uint32_t* used_out = usedslab + (size_t)blockIdx.y * (size_t)G + gat;
    uint32_t* status_out = status;
    size_t out_stride = (size_t)G;
    asm volatile("" : "+v"(sums_out), "+v"(q_out), "+v"(used_out), "+v"(status_out), "+v"(out_stride));

    // everything below counts rows from r0, in 32 bits
    const int32_t* __restrict__ lab = labels + lane.r0;
    const double* __restrict__ siz = size + lane.r0;
    const ColumnReader rd = column_reader(lane, X, ld);
    const int n_rows = rd.n_rows;

#pragma unroll 1
    for (int rt = 0; rt < n_rows; rt += kColumnTile) {
        const int rows = (n_rows - rt < kColumnTile) ? n_rows - rt : kColumnTile;
        __syncthreads();                                  // the previous tile has been read
        if (rd.staged) {                                  // (column_stage, written out: column_device.h says why)
#pragma unroll
            for (int i = 0; i < kColumnTile / 4; ++i) {
                const int tr = rd.lrow + 4 * i;
                if (tr < rows)
                    *reinterpret_cast<int4*>(&tile[tr][rd.lcol]) = *reinterpret_cast<const int4*>(rd.xtile + (int64_t)(rt + tr) * ld);
            }
        }
        // a row's size factor, its logarithm and whether it is used
        if (tid < kColumnTile) {
            int32_t use = 0;
            double s = 1.0;
            if (tid < rows) {
                const int32_t k = lab[rt + tid];
                if (k >= K) {
                    flags |= PROSSTT_AMD_REGRESS_LABEL;
                } else if (k >= 0) {
                    const double sv = siz[rt + tid];
                    if (sv > 0.0 && sv <= kQuasiLargest) {
                        use = 1;
                        s = sv;
                    } else {
                        flags |= PROSSTT_AMD_REGRESS_SIZE;
                    }
                }
            }
            s_use[tid] = use;
            s_size[tid] = s;
            if constexpr (QPASS) s_logs[tid] = log(s);
        }
        // the design rows of the tile: 8 x 16 entries, one per thread of the first two waves
        if (tid < kColumnTile * kMaxP) {
            const int tr = tid / kMaxP, j = tid % kMaxP;
            double v = 0.0;
            if (tr < rows && j < p) {
                const int32_t k = lab[rt + tr];
                if (k >= 0 && k < K) v = design[(int64_t)k * ldd + j];
            }
            s_design[tr][j] = v;
        }
        // the factors of the block's sums
        if (!QPASS && frow < kColumnTile) {
            double v = 0.0;
            if (frow < rows && fj >= 0) {
                const int32_t k = lab[rt + frow];
                if (k >= 0 && k < K) {
                    const double* __restrict__ drow = design + (int64_t)k * ldd;
                    const double dj = drow[fj];
                    v = fpair ? dj * drow[fk] : dj;
                }
            }
            quasi_factor_tables(s_factor[frow][fslot], s_second[frow][fslot], mixed, fpair, v);
        }
        __syncthreads();
#pragma unroll 1
        for (int tr = 0; tr < rows; ++tr) {
            if (!__builtin_amdgcn_readfirstlane(s_use[tr])) continue;      // uniform over the block
            const int32_t x = column_entry(tile, rd, ld, rt, tr);
            neg |= x;
            // (quasi_device.h's eta, written out: in groups of four; beyond p both factors are +0)
            double eta = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) eta = eta + s_design[tr][j] * c[j];
            if (p > 4) {
#pragma unroll
                for (int j = 4; j < 8; ++j) eta = eta + s_design[tr][j] * c[j];
            }
            if (p > 8) {
#pragma unroll
                for (int j = 8; j < 12; ++j) eta = eta + s_design[tr][j] * c[j];
            }
            if (p > 12) {
#pragma unroll
                for (int j = 12; j < 16; ++j) eta = eta + s_design[tr][j] * c[j];
            }
            if (x < 0) continue;
            if (!(__builtin_fabs(eta) <= kQuasiEtaMax)) {      // (also a NaN)
                flags |= PROSSTT_AMD_REGRESS_ETA;
                continue;
            }
            const double mu = s_size[tr] * exp(eta);
            const double amu = a * mu;
            const double d = amu + b;
            if (!(d <= kBig)) {                           // (mu overflowed: infinite, or a NaN from 0 times infinity)
                flags |= PROSSTT_AMD_REGRESS_ETA;
                continue;
            }
            if constexpr (QPASS) {                        // (quasi_device.h's Q term, written out)
                const double l1 = log1p(amu / b);
                const double t = a > 0.0 ? l1 / a : mu / b;
                const double full = ((double)x / b) * ((eta + s_logs[tr]) - (logb + l1)) - t;
                q = q + (x == 0 ? -t : full);
                ++used;
                continue;
            }
            const double w = mu / d;
            const double u = ((double)x - mu) / d;
            const double second = meat ? u * u : w;
            if (!(second <= kBig)) {                      // (u u overflowed: only with a = 0 and a mean beyond 1e154)
                flags |= PROSSTT_AMD_REGRESS_ETA;
                continue;
            }
            // (quasi_device.h's two tables, written out)
            if (!mixed) {
                const double v = nu > 0 ? u : second;
#pragma unroll
                for (int i = 0; i < ACC; ++i) acc[i] = acc[i] + s_factor[tr][i] * v;
            } else {
#pragma unroll
                for (int i = 0; i < ACC; ++i) acc[i] = (acc[i] + s_factor[tr][i] * u) + s_second[tr][i] * second;
            }
        }
    }

    if (mine) {
#pragma unroll
        for (int i = 0; i < ACC; ++i)
            if (i < na) sums_out[(size_t)i * out_stride] = acc[i];
        if constexpr (QPASS) {
            *q_out = q;
            *used_out = used;
        }
    }
    if (neg < 0) flags |= PROSSTT_AMD_REGRESS_NEGATIVE;
    if (flags) atomicOr(status_out, flags);
}

__global__ __launch_bounds__(kThreads) void regress_finish_kernel(const double* __restrict__ slab,
                                                                  const uint32_t* __restrict__ usedslab, int64_t G, int64_t p,
                                                                  int64_t sums, int64_t row_blocks, double* __restrict__ U,
                                                                  double* __restrict__ I, double* __restrict__ Q,
                                                                  uint64_t* __restrict__ used)
{
    quasi_finish(slab, usedslab, G, p, sums, row_blocks, U, I, Q, used);
}

int check_sizes(int64_t N, int64_t G, int64_t p)
{
    if (int rc = column_matrix_refused(N, G)) return rc;
    if (p < 1 || p > kMaxP)
        return fail(PROSSTT_AMD_REGRESS_EINVAL, "need 1 <= p <= %d coefficients (got %lld)", kMaxP, (long long)p);
    return column_finish_refused(G, kMaxSums + 2);                   // (the finishing grid: (sums + 2) G / 256 blocks, for any p)
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_regress_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_regress_workspace_bytes(int64_t N, int64_t G, int64_t p, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_REGRESS_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, p)) return rc;
    *bytes = geometry(N, G, p).at.bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_regress_normal_equations(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                                    const double* size, const int32_t* labels, int64_t K,
                                                    const double* design, int64_t ldd, int64_t p, const double* coef,
                                                    const double* alpha, const double* beta, int32_t meat, int32_t split,
                                                    void* ws, uint64_t ws_bytes, double* U, double* I_or_M, double* Q,
                                                    uint64_t* used, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, p)) return rc;
    if (K < 1 || K >= (int64_t(1) << 31))
        return fail(PROSSTT_AMD_REGRESS_EINVAL, "need 1 <= K < 2^31 rows of the design (got %lld)", (long long)K);
    if (ld < G) return stride_below_row(ld, G);
    if (ldd < p) return stride_below_row(ldd, p);
    if (int rc = quasi_split(p, split)) return rc;
    if (!X || !size || !labels || !design || !coef || !alpha || !beta || !U || !I_or_M || !Q || !used || !status)
        return fail(PROSSTT_AMD_REGRESS_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, p);
    if (!ws || ws_bytes < geo.at.bytes) return workspace_too_small(ws_bytes, geo.at.bytes);
    hipStream_t st = (hipStream_t)stream;
    double* slab = (double*)((char*)ws + geo.at.slab);
    uint32_t* usedslab = (uint32_t*)((char*)ws + geo.at.used);
    const bool vec = aligned(X, ld, 4);
    const auto pass = [&](auto acc) {
        constexpr int ACC = decltype(acc)::value;         // (0: the Q pass, one layer of blocks)
        const dim3 grid((unsigned)geo.strips, (unsigned)geo.row_blocks, ACC ? (unsigned)cdiv(geo.sums, ACC) : 1u);
        const auto kernel = vec ? regress_pass_kernel<true, ACC> : regress_pass_kernel<false, ACC>;
        kernel<<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, size, labels, (int32_t)K, design, ldd, (int32_t)p, coef, alpha, beta,
                                                meat, geo.rows_per_block, slab, usedslab, status);
    };
    if (int rc = quasi_passes(split, pass)) return rc;
    regress_finish_kernel<<<dim3((unsigned)cdiv((geo.sums + 2) * G, kThreads)), dim3(kThreads), 0, st>>>(
        slab, usedslab, G, p, geo.sums, geo.row_blocks, U, I_or_M, Q, used);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
