// The host half of what the libraries on neighbour lists and CSR graphs share (knn, graph, layout, tsne, dpt, cluster): their
// refusals, each message said once, and their grid rules.  The device half is sorted_runs.h.  Internal: included after
// abi_util.h (fail, cdiv, clamp64, pad, kThreads, workspace_too_small, HIP_TRY) and not installed under include/.
#pragma once

namespace {

constexpr int kCUs = 256;                            // of the MI355X
constexpr int64_t kMaxBlocks = int64_t(1) << 20;     // of a grid-stride kernel

// The refusals: each is 0 or the refusal.
inline int check_cells(int64_t N)
{
    if (N < 3 || N >= (int64_t(1) << 31)) return fail(ABI_EINVAL, "need 3 <= N < 2^31 (got %lld)", (long long)N);
    return 0;
}

// a neighbour list of N rows of k entries; max_k is what the library's one-wave-per-row kernel holds
inline int check_sizes(int64_t N, int64_t k, int max_k)
{
    if (int rc = check_cells(N)) return rc;
    const int64_t kmax = N - 1 < max_k ? N - 1 : max_k;
    if (k < 2 || k > kmax) return fail(ABI_EINVAL, "need 2 <= k <= min(N - 1, %d) = %lld (got %lld)", max_k,
                                       (long long)kmax, (long long)k);
    return 0;
}

// a CSR matrix of N rows without a diagonal
inline int check_csr(int64_t N, int64_t nnz)
{
    if (int rc = check_cells(N)) return rc;
    if (nnz < 0 || nnz > N * (N - 1)) return fail(ABI_EINVAL, "need 0 <= nnz <= N (N - 1) (got %lld)", (long long)nnz);
    return 0;
}

// the same and a layout of its rows in c coordinates
inline int check_csr(int64_t N, int64_t nnz, int32_t c)
{
    if (int rc = check_csr(N, nnz)) return rc;
    if (c != 2 && c != 3) return fail(ABI_EINVAL, "need c = 2 or 3 (got %d)", (int)c);
    return 0;
}

inline int check_workspace(const void* ws, uint64_t have, size_t need)
{
    if (!ws) return fail(ABI_EINVAL, "NULL argument");
    if ((uintptr_t)ws % 16 != 0) return fail(ABI_EINVAL, "the workspace must be 16-byte aligned");
    if (have < need) return workspace_too_small(have, need);
    return 0;
}

// The grid rules: the blocks of a grid-stride kernel over `items`, and of a kernel that gives every row a wave.
inline unsigned stride_blocks(int64_t items) { return (unsigned)clamp64(cdiv(items, kThreads), 1, kMaxBlocks); }
inline unsigned wave_per_row_blocks(int64_t N) { return (unsigned)cdiv(N, kThreads / 64); }

// The slabs into which an all-pairs kernel cuts its column tiles when the caller leaves the count to the library: enough
// that `blocks_per_slab` blocks each fill the CUs four times, at least one and at most one per tile.
inline int default_slabs(int64_t blocks_per_slab, int64_t tiles, int max_slabs)
{
    return (int)clamp64(cdiv(4 * kCUs, blocks_per_slab), 1, tiles < max_slabs ? tiles : max_slabs);
}

// the half of the symmetrisation workspace of a neighbour list: 2 N k keys first, as many values behind them
inline size_t half_workspace(int64_t N, int64_t k) { return pad((size_t)(2 * N * k) * 8); }

// The body of a library's symmetrize_fold entry point; `kernel` is its one call of sorted_runs.h's fold_sorted_runs.
template <typename Kernel>
int symmetrize_fold(Kernel kernel, int max_k, void* stream, const int64_t* sorted_keys, const int64_t* perm, const int64_t* pos,
                    int64_t N, int64_t k, int64_t nnz, const void* ws, uint64_t ws_bytes, int64_t* indptr, int32_t* indices,
                    double* data)
{
    if (int rc = check_sizes(N, k, max_k)) return rc;
    if (nnz < N * k || nnz > 2 * N * k)
        return fail(ABI_EINVAL, "need N k <= nnz <= 2 N k (got %lld)", (long long)nnz);
    if (!sorted_keys || !perm || !pos || !indptr || !indices || !data) return fail(ABI_EINVAL, "NULL argument");
    const size_t half = half_workspace(N, k);
    if (int rc = check_workspace(ws, ws_bytes, 2 * half)) return rc;
    kernel<<<dim3(stride_blocks(2 * N * k)), dim3(kThreads), 0, (hipStream_t)stream>>>(
        sorted_keys, perm, pos, (const double*)((const char*)ws + half), 2 * N * k, N, nnz, indptr, indices, data);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
