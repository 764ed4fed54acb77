// libprosstt_amd_factors.so -- the quasi-score, the information and the quasi-log-likelihood of a per-cell regression of a
// device count matrix on gene loadings (include/prosstt_amd_factors.h holds the definition; DESIGN section 35 the reasons).
//
// The arithmetic of an entry, the order of the sums, their split over blockIdx.z (ACC; ACC = 0 adds Q and used), the two
// tables of factors and the slabs are quasi_device.h's, which regress shares.  What factors adds:
//
// Kernels (256 threads = 4 waves each)
//   factors_pass_kernel  regress's column kernel turned on its side: a block owns 256 cells and one range of
//                        genes_per_block genes (gene_blocking), a lane ONE cell, whose coefficients, size factor and ACC
//                        sums stay in registers across the genes.  The matrix is
//                        read along its rows and transposed through LDS: a tile of 256 cells x kTile = 32 genes, loaded in
//                        16-byte pieces (<VEC = true>, whole tiles) or 4-byte pieces (<VEC = false>, and the ragged last tile
//                        under either), eight or thirty-two consecutive lanes on one row; the tile's row stride is
//                        kTile + 1 = 33 words, so the 32 lanes of a half wave write, and later read their own cells'
//                        entries of one gene from, 32 different banks.
//                        What is uniform over the block is formed once per tile of genes and read from LDS by every lane
//                        at one address: whether the gene is used (`use`), its (a, b) and log b, its loadings, and for each
//                        of the block's sums its factor (L_j for a sum of U, the rounded product L_j L_k for one of I).
//   factors_finish_kernel  quasi_finish over the gene blocks
// No atomics but the OR of a status bit.
#include "../../../include/prosstt_amd_factors.h"

#define ABI_EINVAL PROSSTT_AMD_FACTORS_EINVAL
#define ABI_EHIP PROSSTT_AMD_FACTORS_EHIP
#include "../abi_util.h"
#include "../column_device.h"
#include "../quasi_device.h"

namespace {

constexpr int kMaxP = PROSSTT_AMD_FACTORS_MAX_P;
constexpr int kTile = PROSSTT_AMD_FACTORS_TILE_GENES;          // genes of a tile
constexpr int kTileStride = kTile + 1;                         // words of a cell's row of the tile: odd
constexpr int kCells = kThreads;                               // cells of a block: one per lane
constexpr int kOwnGenes = 1024;                               // the library's own blocking makes no block of genes longer than about this
constexpr int kMinTiles = 4;                                   // the library's own blocking gives a block at least this many tiles
constexpr int64_t kMaxGeneBlocks = PROSSTT_AMD_FACTORS_MAX_GENE_BLOCKS;
constexpr int64_t kMaxGenesPerBlock = int64_t(1) << 30;
static_assert(PROSSTT_AMD_FACTORS_SPLIT_16_MAX_SUMS == kQuasiSplit16MaxSums, "the header states the shared rule");
static_assert(kTile % 4 == 0 && kThreads % kTile == 0 && kThreads % (kTile / 4) == 0, "the tile's loads deal rows to whole groups of lanes");

// The library's choice of genes_per_block: about kTargetBlocks blocks over the blocks of cells and no block longer than about
// kOwnGenes genes (measured at 50 000 x 20 000: 256 and 1 024 genes per block are equally fast, 4 000 is 7 to 13 % slower, one
// block for all genes up to twice as slow), at least kMinTiles tiles each, at most kMaxGeneBlocks blocks.
int64_t gene_blocking(int64_t N, int64_t G)
{
    const int64_t cell_blocks = cdiv(N, kCells);
    int64_t gb = kTargetBlocks / cell_blocks;
    if (gb < cdiv(G, kOwnGenes)) gb = cdiv(G, kOwnGenes);
    gb = clamp64(gb, 1, cdiv(G, (int64_t)kMinTiles * kTile));
    if (gb > kMaxGeneBlocks) gb = kMaxGeneBlocks;
    const int64_t per = cdiv(cdiv(G, gb), kTile) * kTile;
    return per < kMaxGenesPerBlock ? per : kMaxGenesPerBlock;      // (a block counts its genes in 32 bits)
}

struct Geometry {
    int64_t cell_blocks = 0, gene_blocks = 0, genes_per_block = 0, sums = 0;
    QuasiSlabs at;                          // the slabs [gene_blocks][sums + 1][N] (U, I, then Q) and [gene_blocks][N]
};

Geometry geometry(int64_t N, int64_t G, int64_t p, int64_t genes_per_block)
{
    Geometry g;
    g.cell_blocks = cdiv(N, kCells);
    g.sums = quasi_sums(p);
    g.genes_per_block = genes_per_block == 0 ? gene_blocking(N, G) : genes_per_block;
    if (g.genes_per_block > cdiv(G, kTile) * kTile) g.genes_per_block = cdiv(G, kTile) * kTile;      // (one block: the same sums)
    if (g.genes_per_block > kMaxGenesPerBlock) g.genes_per_block = kMaxGenesPerBlock;      // (a block counts its genes in 32 bits)
    g.gene_blocks = cdiv(G, g.genes_per_block);
    g.at = quasi_slabs(g.gene_blocks, g.sums, N);
    return g;
}

template <bool VEC, int ACC>
__global__ __launch_bounds__(kThreads) void factors_pass_kernel(const int32_t* __restrict__ X, int64_t N, int64_t G, int64_t ld,
                                                                const double* __restrict__ size, const int32_t* __restrict__ use,
                                                                const double* __restrict__ loadings, int64_t ldl, int32_t p,
                                                                const double* __restrict__ coef, const double* __restrict__ alpha,
                                                                const double* __restrict__ beta, int64_t genes_per_block,
                                                                double* __restrict__ slab, uint32_t* __restrict__ usedslab,
                                                                uint32_t* __restrict__ status)
{
    constexpr bool QPASS = ACC == 0;                      // this instantiation adds Q and used, and no sum of (U, I)
    constexpr int SLOTS = QPASS ? 1 : ACC;
    static_assert(kThreads % SLOTS == 0, "a thread forms the factors of one sum, for kTile SLOTS / kThreads genes of a tile");
    __shared__ int32_t tile[kCells * kTileStride];
    __shared__ double s_load[kTile][kMaxP];
    __shared__ double s_a[kTile], s_b[kTile], s_logb[kTile];
    __shared__ int32_t s_use[kTile];
    __shared__ double s_factor[kTile][SLOTS], s_second[kTile][SLOTS];
    const int tid = threadIdx.x;
    const int sums = p + p * (p + 1) / 2;
    const auto [a0, na, nu, mixed] = quasi_block_sums<ACC>(p, sums);      // the block's first sum, how many, how many of U
    const int64_t cell0 = (int64_t)blockIdx.x * kCells;
    const int n_cells = (N - cell0 < kCells) ? (int)(N - cell0) : kCells;
    const int64_t cell = cell0 + tid;
    const bool mine = tid < n_cells;
    const int64_t g0 = (int64_t)blockIdx.y * genes_per_block;
    const int n_genes = (G - g0 < genes_per_block) ? (int)(G - g0) : (int)genes_per_block;

    // The cell's size factor and coefficients are judged HERE, before any arithmetic on them (the header's rule).
    uint32_t flags = 0;
    bool ok = false;
    double s = 1.0;
    double c[kMaxP], acc[SLOTS];
    if (mine) {
        const double sv = size[cell];
        if (sv > 0.0 && sv <= kQuasiLargest) {
            ok = true;
            s = sv;
        } else {
            flags |= PROSSTT_AMD_FACTORS_SIZE;
        }
    }
#pragma unroll
    for (int j = 0; j < kMaxP; ++j) {
        c[j] = 0.0;
        if (mine && j < p) {
            const double cv = coef[(int64_t)j * N + cell];
            if (__builtin_fabs(cv) <= kBig)
                c[j] = cv;
            else
                flags |= PROSSTT_AMD_FACTORS_COEFFICIENT;
        }
    }
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) acc[i] = 0.0;
    double logs = 0.0;
    if constexpr (QPASS) logs = log(s);
    double q = 0.0;
    uint32_t used = 0;
    int32_t neg = 0;

    // the sum whose factors this thread forms for the tiles (thread tid: genes tid / SLOTS + i kThreads / SLOTS of the tile,
    // sum a0 + tid % SLOTS): fj == fk for a sum of U (the factor is L[fj]), fj <= fk for one of I (L[fj] L[fk]), fj < 0
    // beyond the last sum (quasi_device.h's order of the sums, written out: DESIGN section 36)
    const int frow = tid / SLOTS, fslot = tid % SLOTS;
    int fj = -1, fk = -1;
    bool fpair = false;
    if (fslot < na) {
        const int t0 = a0 + fslot;
        if (t0 < p) {
            fj = fk = t0;
        } else {
            int t = t0 - p, j = 0;
            while (t >= p - j) {
                t -= p - j;
                ++j;
            }
            fj = j;
            fk = j + t;
            fpair = true;
        }
    }

    // where the Q instantiation's sums go, formed here so that its loop need not keep the kernel's arguments for them (in
    // vector registers from here on; kept as scalar arguments, four of them spill in the aligned kernel: regress_pass_kernel
    // has the same lines).  The sums kernels have scalar registers to spare and none of the vector kind: they form their
    // addresses after the loop.
    const size_t cat = (size_t)(mine ? cell : 0);
    double* q_out = slab + ((size_t)blockIdx.y * (size_t)(sums + 1) + (size_t)sums) * (size_t)N + cat;
    uint32_t* used_out = usedslab + (size_t)blockIdx.y * (size_t)N + cat;
    uint32_t* status_out = status;
    if constexpr (QPASS) asm volatile("" : "+v"(q_out), "+v"(used_out), "+v"(status_out));

    // the lane's part of a tile's loads: 16-byte pieces, eight lanes to a row; 4-byte pieces, thirty-two lanes to a row
    const int vrow = tid / (kTile / 4), vcol = 4 * (tid % (kTile / 4));
    const int srow = tid / kTile, scol = tid % kTile;
    const int32_t* __restrict__ xblock = X + cell0 * ld + g0;

#pragma unroll 1
    for (int gt = 0; gt < n_genes; gt += kTile) {
        const int genes = (n_genes - gt < kTile) ? n_genes - gt : kTile;
        __syncthreads();                                  // the previous tile and its tables have been read
        if (VEC && genes == kTile) {
            // (four loads in flight, two trips: all eight cost 24 to 26 more registers and a wave per SIMD of every sums kernel)
#pragma unroll 4
            for (int i = 0; i < kCells / (kThreads / (kTile / 4)); ++i) {
                const int r = vrow + i * (kThreads / (kTile / 4));
                if (r < n_cells) {
                    const int4 v = *reinterpret_cast<const int4*>(xblock + (int64_t)r * ld + gt + vcol);
                    int32_t* t = &tile[r * kTileStride + vcol];       // (the odd stride: four 4-byte stores)
                    t[0] = v.x;
                    t[1] = v.y;
                    t[2] = v.z;
                    t[3] = v.w;
                }
            }
        } else {
#pragma unroll 4
            for (int i = 0; i < kCells / (kThreads / kTile); ++i) {
                const int r = srow + i * (kThreads / kTile);
                if (r < n_cells && scol < genes) tile[r * kTileStride + scol] = xblock[(int64_t)r * ld + gt + scol];
            }
        }
        // whether a gene is used, its parameters and its loadings: judged here, once per block
        if (tid < kTile) {
            int32_t u = -1;
            double a = 0.0, b = 2.0;
            if (tid < genes) {
                const int64_t g = g0 + gt + tid;
                u = use ? use[g] : 0;
                if (u >= 0) {
                    const double av = alpha[g], bv = beta[g];
                    if (column_admissible(av, bv)) {
                        a = av;
                        b = bv;
                    } else {
                        flags |= PROSSTT_AMD_FACTORS_PARAMETER;
                    }
                }
            }
            s_use[tid] = u;
            s_a[tid] = a;
            s_b[tid] = b;
            if constexpr (QPASS) s_logb[tid] = log(b);
        }
#pragma unroll
        for (int i = 0; i < kTile * kMaxP / kThreads; ++i) {
            const int e = tid + i * kThreads;
            const int tg = e / kMaxP, j = e % kMaxP;
            double v = 0.0;
            if (tg < genes && j < p) {
                const int64_t g = g0 + gt + tg;
                if (!use || use[g] >= 0) {
                    const double lv = loadings[g * ldl + j];
                    if (__builtin_fabs(lv) <= kBig)
                        v = lv;
                    else
                        flags |= PROSSTT_AMD_FACTORS_COEFFICIENT;
                }
            }
            s_load[tg][j] = v;
        }
        // the factors of the block's sums
        if constexpr (!QPASS) {
#pragma unroll
            for (int i = 0; i < kTile * SLOTS / kThreads; ++i) {
                const int tg = frow + i * (kThreads / SLOTS);
                double v = 0.0;
                if (tg < genes && fj >= 0) {
                    const int64_t g = g0 + gt + tg;
                    if (!use || use[g] >= 0) {
                        const double* __restrict__ lrow = loadings + g * ldl;
                        double lj = lrow[fj], lk = lrow[fk];
                        if (!(__builtin_fabs(lj) <= kBig)) lj = 0.0;       // (its bit is set where the loadings' table is formed)
                        if (!(__builtin_fabs(lk) <= kBig)) lk = 0.0;
                        v = fpair ? lj * lk : lj;
                    }
                }
                quasi_factor_tables(s_factor[tg][fslot], s_second[tg][fslot], mixed, fpair, v);
            }
        }
        __syncthreads();
        if (ok) {
            const int32_t* __restrict__ mytile = &tile[tid * kTileStride];
#pragma unroll 1
            for (int tg = 0; tg < genes; ++tg) {
                if (__builtin_amdgcn_readfirstlane(s_use[tg]) < 0) continue;      // uniform over the block
                const int32_t x = mytile[tg];
                neg |= x;
                // (quasi_device.h's eta, written out: in groups of four; beyond p both factors are +0)
                double eta = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) eta = eta + s_load[tg][j] * c[j];
                if (p > 4) {
#pragma unroll
                    for (int j = 4; j < 8; ++j) eta = eta + s_load[tg][j] * c[j];
                }
                if (p > 8) {
#pragma unroll
                    for (int j = 8; j < 12; ++j) eta = eta + s_load[tg][j] * c[j];
                }
                if (p > 12) {
#pragma unroll
                    for (int j = 12; j < 16; ++j) eta = eta + s_load[tg][j] * c[j];
                }
                if (x < 0) continue;
                if (!(__builtin_fabs(eta) <= kQuasiEtaMax)) {      // (also a NaN)
                    flags |= PROSSTT_AMD_FACTORS_ETA;
                    continue;
                }
                const double a = s_a[tg], b = s_b[tg];
                const double mu = s * exp(eta);
                const double amu = a * mu;
                const double d = amu + b;
                if (!(d <= kBig)) {                           // (mu overflowed: infinite, or a NaN from 0 times infinity)
                    flags |= PROSSTT_AMD_FACTORS_ETA;
                    continue;
                }
                if constexpr (QPASS) {                        // (quasi_device.h's Q term, written out)
                    const double l1 = log1p(amu / b);
                    const double t = a > 0.0 ? l1 / a : mu / b;
                    const double full = ((double)x / b) * ((eta + logs) - (s_logb[tg] + l1)) - t;
                    q = q + (x == 0 ? -t : full);
                    ++used;
                    continue;
                }
                const double w = mu / d;
                const double u = ((double)x - mu) / d;
                // (quasi_device.h's two tables, written out)
                if (!mixed) {
                    const double v = nu > 0 ? u : w;
#pragma unroll
                    for (int i = 0; i < ACC; ++i) acc[i] = acc[i] + s_factor[tg][i] * v;
                } else {
#pragma unroll
                    for (int i = 0; i < ACC; ++i) acc[i] = (acc[i] + s_factor[tg][i] * u) + s_second[tg][i] * w;
                }
            }
        }
    }

    if (mine) {
        const size_t out_stride = (size_t)N;
        double* sums_out = slab + ((size_t)blockIdx.y * (size_t)(sums + 1) + (size_t)a0) * out_stride + cat;
#pragma unroll
        for (int i = 0; i < ACC; ++i)
            if (i < na) sums_out[(size_t)i * out_stride] = acc[i];
        if constexpr (QPASS) {
            *q_out = q;
            *used_out = used;
        }
    }
    if (neg < 0) flags |= PROSSTT_AMD_FACTORS_NEGATIVE;
    if (flags) atomicOr(status_out, flags);
}

__global__ __launch_bounds__(kThreads) void factors_finish_kernel(const double* __restrict__ slab,
                                                                  const uint32_t* __restrict__ usedslab, int64_t N, int64_t p,
                                                                  int64_t sums, int64_t gene_blocks, double* __restrict__ U,
                                                                  double* __restrict__ I, double* __restrict__ Q,
                                                                  uint64_t* __restrict__ used)
{
    quasi_finish(slab, usedslab, N, p, sums, gene_blocks, U, I, Q, used);
}

int check_sizes(int64_t N, int64_t G, int64_t p, int64_t genes_per_block)
{
    if (cells_out_of_range(N) || G < 1 || G >= (int64_t(1) << 31))
        return fail(PROSSTT_AMD_FACTORS_EINVAL, "need 1 <= N < 2^31 and 1 <= G < 2^31 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (p < 1 || p > kMaxP)
        return fail(PROSSTT_AMD_FACTORS_EINVAL, "need 1 <= p <= %d coefficients (got %lld)", kMaxP, (long long)p);
    if (genes_per_block < 0 || genes_per_block % kTile != 0)
        return fail(PROSSTT_AMD_FACTORS_EINVAL, "genes_per_block must be 0 or a multiple of %d (got %lld)", kTile,
                    (long long)genes_per_block);
    if (genes_per_block > 0 && cdiv(G, genes_per_block) > kMaxGeneBlocks)
        return fail(PROSSTT_AMD_FACTORS_EINVAL, "genes_per_block = %lld cuts %lld genes into more than %lld blocks",
                    (long long)genes_per_block, (long long)G, (long long)kMaxGeneBlocks);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_factors_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_factors_gene_blocking(int64_t N, int64_t G, int64_t* genes_per_block) try
{
    if (!genes_per_block) return fail(PROSSTT_AMD_FACTORS_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, 1, 0)) return rc;
    *genes_per_block = gene_blocking(N, G);
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_factors_workspace_bytes(int64_t N, int64_t G, int64_t p, int64_t genes_per_block, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_FACTORS_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, p, genes_per_block)) return rc;
    *bytes = geometry(N, G, p, genes_per_block).at.bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_factors_cell_equations(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                                  const double* size, const int32_t* use, const double* loadings, int64_t ldl,
                                                  int64_t p, const double* coef, const double* alpha, const double* beta,
                                                  int32_t split, int64_t genes_per_block, void* ws, uint64_t ws_bytes, double* U,
                                                  double* I, double* Q, uint64_t* used, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, p, genes_per_block)) return rc;
    if (ld < G) return stride_below_row(ld, G);
    if (ldl < p) return stride_below_row(ldl, p);
    if (int rc = quasi_split(p, split)) return rc;
    if (!X || !size || !loadings || !coef || !alpha || !beta || !U || !I || !Q || !used || !status)
        return fail(PROSSTT_AMD_FACTORS_EINVAL, "NULL argument");
    const Geometry geo = geometry(N, G, p, genes_per_block);
    if (!ws || ws_bytes < geo.at.bytes) return workspace_too_small(ws_bytes, geo.at.bytes);
    hipStream_t st = (hipStream_t)stream;
    double* slab = (double*)((char*)ws + geo.at.slab);
    uint32_t* usedslab = (uint32_t*)((char*)ws + geo.at.used);
    const bool vec = aligned(X, ld, 4);
    const auto pass = [&](auto acc) {
        constexpr int ACC = decltype(acc)::value;         // (0: the Q pass, one layer of blocks)
        const dim3 grid((unsigned)geo.cell_blocks, (unsigned)geo.gene_blocks, ACC ? (unsigned)cdiv(geo.sums, ACC) : 1u);
        const auto kernel = vec ? factors_pass_kernel<true, ACC> : factors_pass_kernel<false, ACC>;
        kernel<<<grid, dim3(kThreads), 0, st>>>(X, N, G, ld, size, use, loadings, ldl, (int32_t)p, coef, alpha, beta,
                                                geo.genes_per_block, slab, usedslab, status);
    };
    if (int rc = quasi_passes(split, pass)) return rc;
    factors_finish_kernel<<<dim3((unsigned)cdiv((geo.sums + 2) * N, kThreads)), dim3(kThreads), 0, st>>>(
        slab, usedslab, N, p, geo.sums, geo.gene_blocks, U, I, Q, used);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
