// libprosstt_amd_autocorr.so -- sums over the edges of a cell graph of the log-normalised count matrix, and the smoothed
// matrix W.A (include/prosstt_amd_autocorr.h).
//
// Kernels (the definition and the order of the sums are in the header)
//   autocorr_sums_kernel    a wave owns a block of matrix rows and a tile of genes: per row's cell it gathers the neighbours'
//                           segments of the int32 matrix, forms a = log1p(x * inv) (embed's entry()) and z = a - mean in registers,
//                           and keeps the lag m and the squared differences q of the cell, then the four sums of the block
//   autocorr_finish_kernel  one thread per gene: the blocks in ascending order
//   autocorr_smooth_kernel  the same gather with mean = 0 over 8 cells per wave; (float)(m * scale) is stored
// There are no floating-point atomics and nothing is fused (-ffp-contract=off): a numpy model reproduces the bits.
#include "../../../include/prosstt_amd_autocorr.h"

#define ABI_EINVAL PROSSTT_AMD_AUTOCORR_EINVAL
#define ABI_EHIP PROSSTT_AMD_AUTOCORR_EHIP
#include "../abi_util.h"
#include "../log1p_entry.h"                 // entry(): the float32 log1p(x * inv), shared with embed/embed.hip

namespace {

constexpr int kWaves = kThreads / 64;        // waves of a workgroup: adjacent gene tiles of the same cells
constexpr int kBatch = 4;                    // neighbours whose segments are in flight together
constexpr int kSmoothCells = 8;              // cells per wave of the smoothing kernel
constexpr int64_t kMaxGridY = 65535;
constexpr int64_t kMinRows = 16, kCellBlocks = 512, kMinWaves = 4096;

struct Geometry {
    int64_t rows_per_block = 0, blocks = 0;
    size_t bytes = 0;
};

// rows_per_block = 0: a function of N alone, so that the order of a gene's sum does not depend on G.
Geometry geometry(int64_t N, int64_t G, int64_t rows_per_block)
{
    Geometry g;
    const int64_t rule = cdiv(N, kCellBlocks) > kMinRows ? cdiv(N, kCellBlocks) : kMinRows;
    g.rows_per_block = rows_per_block > 0 ? rows_per_block : rule;
    g.blocks = cdiv(N, g.rows_per_block);
    g.bytes = 4 * pad((size_t)g.blocks * (size_t)G * 8);
    return g;
}

// gene_tile = 0: four genes per lane where every row can be read with 16-byte loads and that still fills the device.
int tile_rule(int32_t gene_tile, const void* X, int64_t ld, int64_t G, int64_t waves_per_tile)
{
    if (gene_tile) return gene_tile;
    return aligned(X, ld, 4) && cdiv(G, 256) * waves_per_tile >= kMinWaves ? 256 : 64;
}

struct Graph {
    const int64_t* __restrict__ indptr;
    const int32_t* __restrict__ indices;
    const double* __restrict__ data;
    int64_t nnz;
};

struct Matrix {
    const int32_t* __restrict__ X;
    const float* __restrict__ inv_size;
    const int32_t* __restrict__ cell_of_row;
    int64_t N, G, ld;
};

// The matrix row that an entry of the graph names, or -1 when it lies outside [0, N).  Wave-uniform.
__device__ __forceinline__ int64_t row_of(const Matrix& A, int64_t r) { return r < 0 || r >= A.N ? -1 : r; }

// The cell that matrix row r (in [0, N)) holds, or -1 when it lies outside [0, N).  Wave-uniform.
__device__ __forceinline__ int64_t cell_of(const Matrix& A, int64_t r)
{
    const int64_t i = A.cell_of_row ? (int64_t)A.cell_of_row[r] : r;
    return i < 0 || i >= A.N ? -1 : i;
}

// The lane's V counts of one row: genes g0 .. g0 + V - 1 (WIDE: one 16-byte load; else zeros past G).
template <int V, bool WIDE>
__device__ __forceinline__ void load_counts(int32_t (&x)[V], const int32_t* __restrict__ rp, int64_t g0, int64_t G)
{
    if constexpr (WIDE) {
        static_assert(V == 4, "a 16-byte load holds four counts");
        const int4 v = *reinterpret_cast<const int4*>(rp + g0);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) x[j] = g0 + j < G ? rp[g0 + j] : 0;
    }
}

// One neighbour: m = m + w z_j; SUMS: q = q + w (a_i - a_j)^2.  Every operation is rounded on its own.
template <int V, bool SUMS>
__device__ __forceinline__ void add_neighbour(double (&m)[V], double (&q)[V], const double (&ai)[V], const double (&mu)[V],
                                              const int32_t (&x)[V], float inv, double w)
{
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const double aj = (double)entry(x[j], inv);
        const double zj = SUMS ? aj - mu[j] : aj;
        m[j] = m[j] + w * zj;
        if (SUMS) {
            const double d = ai[j] - aj;
            q[j] = q[j] + w * (d * d);
        }
    }
}

// The lag m (and q) of one cell over the entries [e0, e1) of its row, in that order.
template <int V, bool WIDE, bool SUMS>
__device__ __forceinline__ void gather_row(double (&m)[V], double (&q)[V], const double (&ai)[V], const double (&mu)[V],
                                           const Matrix& A, const Graph& W, int64_t e0, int64_t e1, int64_t g0,
                                           uint32_t& flags)
{
    int64_t e = e0;
    // kBatch neighbours at a time while there are as many and all lie in the matrix: their loads are issued together
    for (; e + kBatch <= e1; e += kBatch) {
        int64_t r[kBatch];
        bool ok = true;
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            r[u] = row_of(A, W.indices[e + u]);
            ok = ok && r[u] >= 0;
        }
        if (!ok) break;
        int32_t x[kBatch][V];
        float inv[kBatch];
        double w[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            load_counts<V, WIDE>(x[u], A.X + r[u] * A.ld, g0, A.G);
            inv[u] = A.inv_size[r[u]];
            w[u] = W.data[e + u];
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) add_neighbour<V, SUMS>(m, q, ai, mu, x[u], inv[u], w[u]);
    }
    // the last entries of the row, and everything from a batch on that holds an index outside the matrix: one by one
    for (; e < e1; ++e) {
        const int64_t r = row_of(A, W.indices[e]);
        if (r < 0) {
            flags |= PROSSTT_AMD_AUTOCORR_INDEX_RANGE;   // the row is not read
        } else {
            int32_t x[V];
            load_counts<V, WIDE>(x, A.X + r * A.ld, g0, A.G);
            add_neighbour<V, SUMS>(m, q, ai, mu, x, A.inv_size[r], W.data[e]);
        }
    }
}

// The entries [e0, e1) of cell i's row, clamped into [0, nnz] (a guard: indptr is the caller's to check).
__device__ __forceinline__ void row_range(const Graph& W, int64_t i, int64_t& e0, int64_t& e1, uint32_t& flags)
{
    e0 = W.indptr[i];
    e1 = W.indptr[i + 1];
    if (e0 < 0 || e1 < e0 || e1 > W.nnz) {
        flags |= PROSSTT_AMD_AUTOCORR_INDEX_RANGE;
        e0 = e1 = 0;
    }
}

template <int V, bool WIDE>
__device__ __forceinline__ void sums_of_block(const Matrix& A, const Graph& W, const double* __restrict__ mean,
                                              int64_t first, int64_t last, int64_t g0, size_t at, size_t slab,
                                              double* __restrict__ partial, uint32_t* __restrict__ status)
{
    double mu[V], cross[V], sq[V], m2[V], m4[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        mu[j] = g0 + j < A.G ? mean[g0 + j] : 0.0;
        cross[j] = sq[j] = m2[j] = m4[j] = 0.0;
    }
    uint32_t flags = 0;
    int32_t neg = 0;
    for (int64_t r = first; r < last; ++r) {        // matrix rows: neighbours in the graph lie near each other there
        const int64_t i = cell_of(A, r);
        if (i < 0) {
            flags |= PROSSTT_AMD_AUTOCORR_INDEX_RANGE;
            continue;
        }
        int32_t x[V];
        load_counts<V, WIDE>(x, A.X + r * A.ld, g0, A.G);
        const float inv = A.inv_size[r];
        int64_t e0, e1;
        row_range(W, i, e0, e1, flags);
        double ai[V], z[V], m[V], q[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            neg |= x[j];
            ai[j] = (double)entry(x[j], inv);
            z[j] = ai[j] - mu[j];
            m[j] = q[j] = 0.0;
        }
        gather_row<V, WIDE, true>(m, q, ai, mu, A, W, e0, e1, g0, flags);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const double zz = z[j] * z[j];
            cross[j] = cross[j] + z[j] * m[j];
            sq[j] = sq[j] + q[j];
            m2[j] = m2[j] + zz;
            m4[j] = m4[j] + zz * zz;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        if (g0 + j < A.G) {
            partial[at + g0 + j] = cross[j];
            partial[slab + at + g0 + j] = sq[j];
            partial[2 * slab + at + g0 + j] = m2[j];
            partial[3 * slab + at + g0 + j] = m4[j];
        }
    }
    if (neg < 0) flags |= PROSSTT_AMD_AUTOCORR_NEGATIVE;
    if (flags) atomicOr(status, flags);
}

// blockIdx.x: the block of rows (fastest, so that resident workgroups share a column slab); blockIdx.y and the wave: the
// tile of genes.  slab: the elements of one of the four partial slabs [blocks][G].
template <int V>
__global__ __launch_bounds__(kThreads) void autocorr_sums_kernel(Matrix A, Graph W, const double* __restrict__ mean,
                                                                 int64_t rows_per_block, bool wide, size_t slab,
                                                                 double* __restrict__ partial, uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = (int64_t)blockIdx.y * kWaves + wave;
    const int64_t gbase = tile * (64 * V);
    if (gbase >= A.G) return;                       // (no barrier below: a wave past the last tile leaves)
    const int64_t g0 = gbase + V * lane;
    const int64_t first = (int64_t)blockIdx.x * rows_per_block;
    const int64_t last = first + rows_per_block < A.N ? first + rows_per_block : A.N;
    const size_t at = (size_t)blockIdx.x * (size_t)A.G;
    if constexpr (V == 4) {
        if (wide && gbase + 64 * V <= A.G) {
            sums_of_block<V, true>(A, W, mean, first, last, g0, at, slab, partial, status);
            return;
        }
    }
    sums_of_block<V, false>(A, W, mean, first, last, g0, at, slab, partial, status);
}

__global__ __launch_bounds__(kThreads) void autocorr_finish_kernel(const double* __restrict__ partial, int64_t blocks,
                                                                   int64_t G, size_t slab, double* __restrict__ cross,
                                                                   double* __restrict__ sqdiff, double* __restrict__ m2,
                                                                   double* __restrict__ m4)
{
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    double a = 0.0, b = 0.0, c = 0.0, d = 0.0;
    for (int64_t i = 0; i < blocks; ++i) {
        const size_t at = (size_t)i * (size_t)G + (size_t)g;
        a = a + partial[at];
        b = b + partial[slab + at];
        c = c + partial[2 * slab + at];
        d = d + partial[3 * slab + at];
    }
    cross[g] = a;
    sqdiff[g] = b;
    m2[g] = c;
    m4[g] = d;
}

template <int V, bool WIDE>
__device__ __forceinline__ void smooth_cells(const Matrix& A, const Graph& W, bool normalize, int64_t first, int64_t last,
                                             int64_t g0, float* __restrict__ out, int64_t ldo,
                                             uint32_t* __restrict__ status)
{
    uint32_t flags = 0;
    int32_t neg = 0;
    for (int64_t r = first; r < last; ++r) {
        const int64_t i = cell_of(A, r);
        if (i < 0) {
            flags |= PROSSTT_AMD_AUTOCORR_INDEX_RANGE;
            continue;
        }
        int64_t e0, e1;
        row_range(W, i, e0, e1, flags);
        {                                           // the cell's own row is read for the check of its counts alone
            int32_t x[V];
            load_counts<V, WIDE>(x, A.X + r * A.ld, g0, A.G);
#pragma unroll
            for (int j = 0; j < V; ++j) neg |= x[j];
        }
        double m[V], zero[V];
#pragma unroll
        for (int j = 0; j < V; ++j) m[j] = zero[j] = 0.0;
        gather_row<V, WIDE, false>(m, zero, zero, zero, A, W, e0, e1, g0, flags);
        double scale = 1.0;
        if (normalize) {
            double d = 0.0;
            for (int64_t e = e0; e < e1; ++e) d = d + W.data[e];
            scale = d == 0.0 ? 0.0 : 1.0 / d;
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (g0 + j < A.G) out[i * ldo + g0 + j] = scale == 0.0 ? 0.0f : (float)(m[j] * scale);
    }
    if (neg < 0) flags |= PROSSTT_AMD_AUTOCORR_NEGATIVE;
    if (flags) atomicOr(status, flags);
}

template <int V>
__global__ __launch_bounds__(kThreads) void autocorr_smooth_kernel(Matrix A, Graph W, bool normalize, bool wide,
                                                                   float* __restrict__ out, int64_t ldo,
                                                                   uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tile = (int64_t)blockIdx.y * kWaves + wave;
    const int64_t gbase = tile * (64 * V);
    if (gbase >= A.G) return;
    const int64_t g0 = gbase + V * lane;
    const int64_t first = (int64_t)blockIdx.x * kSmoothCells;
    const int64_t last = first + kSmoothCells < A.N ? first + kSmoothCells : A.N;
    if constexpr (V == 4) {
        if (wide && gbase + 64 * V <= A.G) {
            smooth_cells<V, true>(A, W, normalize, first, last, g0, out, ldo, status);
            return;
        }
    }
    smooth_cells<V, false>(A, W, normalize, first, last, g0, out, ldo, status);
}

int check_matrix(int64_t N, int64_t G, int64_t ld, int64_t nnz, int32_t gene_tile)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (ld < G) return stride_below_row(ld, G);
    if (nnz < 0) return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "need nnz >= 0 (got %lld)", (long long)nnz);
    if (gene_tile != 0 && gene_tile != 64 && gene_tile != 256)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "gene_tile must be 0, 64 or 256 (got %d)", (int)gene_tile);
    return 0;
}

int check_tiles(int64_t G, int tile)
{
    if (cdiv(cdiv(G, tile), kWaves) > kMaxGridY)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "%lld genes in tiles of %d are above the grid's %lld x %d tiles", (long long)G,
                    tile, (long long)kMaxGridY, kWaves);
    return 0;
}

bool on8(const void* p) { return (uintptr_t)p % 8 == 0; }

int check_graph(const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz)
{
    if (!indptr || ((!indices || !data) && nnz > 0)) return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "NULL argument");
    if (!on8(indptr) || !on8(data) || (uintptr_t)indices % 4 != 0)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "a misaligned CSR array");
    return 0;
}

int check_sizes(int64_t N, int64_t G, int64_t rows_per_block)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N,
                    (long long)G);
    if (rows_per_block < 0)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "need rows_per_block >= 0 (got %lld)", (long long)rows_per_block);
    return 0;
}

}  // namespace

ABI_EXPORT const char* prosstt_amd_autocorr_last_error(void) { return g_err; }

ABI_EXPORT int prosstt_amd_autocorr_workspace_bytes(int64_t N, int64_t G, int64_t rows_per_block, uint64_t* bytes) try
{
    if (!bytes) return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "NULL argument");
    if (int rc = check_sizes(N, G, rows_per_block)) return rc;
    *bytes = geometry(N, G, rows_per_block).bytes;
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_autocorr_gene_sums(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                              const float* inv_size, const int32_t* cell_of_row,
                                              const int64_t* indptr,
                                              const int32_t* indices, const double* data, int64_t nnz, const double* mean,
                                              int64_t rows_per_block, int32_t gene_tile, void* ws, uint64_t ws_bytes,
                                              double* cross, double* sqdiff, double* m2, double* m4, uint32_t* status) try
{
    if (int rc = check_sizes(N, G, rows_per_block)) return rc;
    if (int rc = check_matrix(N, G, ld, nnz, gene_tile)) return rc;
    if (!X || !inv_size || !mean || !ws || !cross || !sqdiff || !m2 || !m4 || !status)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "NULL argument");
    if (int rc = check_graph(indptr, indices, data, nnz)) return rc;
    if ((uintptr_t)X % 4 != 0 || (uintptr_t)inv_size % 4 != 0 || (uintptr_t)cell_of_row % 4 != 0 ||
        (uintptr_t)status % 4 != 0 ||
        !on8(mean) || !on8(cross) || !on8(sqdiff) || !on8(m2) || !on8(m4))
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "a misaligned array");
    if ((uintptr_t)ws % 16 != 0) return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "the workspace is not 16-byte aligned");
    const Geometry geo = geometry(N, G, rows_per_block);
    if (ws_bytes < geo.bytes) return workspace_too_small(ws_bytes, geo.bytes);
    const int tile = tile_rule(gene_tile, X, ld, G, geo.blocks);
    if (int rc = check_tiles(G, tile)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Matrix A{X, inv_size, cell_of_row, N, G, ld};
    const Graph W{indptr, indices, data, nnz};
    double* partial = (double*)ws;
    const size_t slab = geo.bytes / 4 / 8;
    const dim3 grid((unsigned)geo.blocks, (unsigned)cdiv(cdiv(G, tile), kWaves));
    if (tile == 256)
        autocorr_sums_kernel<4><<<grid, dim3(kThreads), 0, st>>>(A, W, mean, geo.rows_per_block, aligned(X, ld, 4), slab,
                                                                 partial, status);
    else
        autocorr_sums_kernel<1><<<grid, dim3(kThreads), 0, st>>>(A, W, mean, geo.rows_per_block, false, slab, partial, status);
    HIP_TRY(hipGetLastError());
    autocorr_finish_kernel<<<dim3((unsigned)cdiv(G, kThreads)), dim3(kThreads), 0, st>>>(partial, geo.blocks, G, slab, cross,
                                                                                         sqdiff, m2, m4);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH

ABI_EXPORT int prosstt_amd_autocorr_smooth(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld,
                                           const float* inv_size, const int32_t* cell_of_row,
                                              const int64_t* indptr,
                                           const int32_t* indices, const double* data, int64_t nnz, int32_t normalize,
                                           int32_t gene_tile, float* out, int64_t ldo, uint32_t* status) try
{
    if (int rc = check_matrix(N, G, ld, nnz, gene_tile)) return rc;
    if (ldo < G)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "output row stride %lld is below the row length %lld", (long long)ldo,
                    (long long)G);
    if (!X || !inv_size || !out || !status) return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "NULL argument");
    if (int rc = check_graph(indptr, indices, data, nnz)) return rc;
    if ((uintptr_t)X % 4 != 0 || (uintptr_t)inv_size % 4 != 0 || (uintptr_t)cell_of_row % 4 != 0 ||
        (uintptr_t)status % 4 != 0 ||
        (uintptr_t)out % 4 != 0)
        return fail(PROSSTT_AMD_AUTOCORR_EINVAL, "a misaligned array");
    const int64_t groups = cdiv(N, kSmoothCells);
    const int tile = tile_rule(gene_tile, X, ld, G, groups);
    if (int rc = check_tiles(G, tile)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Matrix A{X, inv_size, cell_of_row, N, G, ld};
    const Graph W{indptr, indices, data, nnz};
    const dim3 grid((unsigned)groups, (unsigned)cdiv(cdiv(G, tile), kWaves));
    if (tile == 256)
        autocorr_smooth_kernel<4><<<grid, dim3(kThreads), 0, st>>>(A, W, normalize != 0, aligned(X, ld, 4), out, ldo, status);
    else
        autocorr_smooth_kernel<1><<<grid, dim3(kThreads), 0, st>>>(A, W, normalize != 0, false, out, ldo, status);
    HIP_TRY(hipGetLastError());
    return 0;
}
ABI_CATCH
