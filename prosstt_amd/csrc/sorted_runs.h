// The fold of sorted keyed entries (row << 32 | column) into a CSR matrix: the device half of what the libraries on
// neighbour lists and CSR graphs share (the host half is graph_util.h).  Internal: included by graph/graph.hip and
// tsne/tsne.hip after abi_util.h, whose kThreads is the block of the fold; not installed under include/.
#pragma once

// The body of a fold kernel, one thread per sorted entry in a grid-stride loop.  The head of a run of equal keys (entry p
// with sorted[p - 1] != sorted[p]) folds the run's values vals[perm[.]] from the left with `combine(w, b)` and writes
// entry o = pos[p] - 1 of the output: the key's low half as the column and `finish(w)` as the value; pos is the prefix
// sum of the heads.  A pos outside [1, nnz] writes nothing, a perm outside [0, M) reads 0, and no row above N is written
// whatever the keys hold: no index the caller computed is trusted.
template <typename Combine, typename Finish>
__device__ __forceinline__ void fold_sorted_runs(const int64_t* __restrict__ sorted, const int64_t* __restrict__ perm,
                                                 const int64_t* __restrict__ pos, const double* __restrict__ vals, int64_t M,
                                                 int64_t N, int64_t nnz, int64_t* __restrict__ indptr,
                                                 int32_t* __restrict__ indices, double* __restrict__ data, Combine combine,
                                                 Finish finish)
{
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < M; p += stride) {
        const int64_t key = sorted[p];
        const int64_t before = p > 0 ? sorted[p - 1] : int64_t(-1);
        if (p > 0 && before == key) continue;         // not the head of its run
        const int64_t o = pos[p] - 1;
        if (o < 0 || o >= nnz) continue;              // (a pos that is not the prefix sum of the heads: write nothing)
        const uint64_t src = (uint64_t)perm[p];
        double w = src < (uint64_t)M ? vals[src] : 0.0;
        int64_t q = p + 1;
        for (; q < M && sorted[q] == key; ++q) {
            const uint64_t s = (uint64_t)perm[q];
            w = combine(w, s < (uint64_t)M ? vals[s] : 0.0);
        }
        indices[o] = (int32_t)(uint32_t)key;
        data[o] = finish(w);
        // the rows behind the previous head's row up to this one start at o: the empty rows between them too
        const int64_t row = key >> 32, prev = p > 0 ? before >> 32 : int64_t(-1);
        for (int64_t r = prev < -1 ? 0 : prev + 1; r <= row && r <= N; ++r) indptr[r] = o;
        if (q == M)                                   // the last run closes every row behind it, and indptr[N]
            for (int64_t r = row < -1 ? 0 : row + 1; r <= N; ++r) indptr[r] = nnz;
    }
}
