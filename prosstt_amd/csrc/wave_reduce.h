// Butterfly reductions over the lanes of a wave: every lane ends with the result of its group.
// Internal: included by graph/graph.hip, layout/layout.hip, cluster/cluster.hip, tsne/tsne.hip, mapping/mapping.hip, ptree/ptree.hip
// and evaluate/evaluate.hip (whose sums are integers: there the order does not matter), not installed under include/.
// (What those libraries share besides is in graph_util.h, the host half, and sorted_runs.h, the fold; neither needs this file.)
// The order is fixed, __shfl_xor with off = G / 2 down to 1: the binary64 and binary32 sums depend on it and the tests pin them
// bit for bit.  (count_summary's reduce_rows4 sums four rows in one butterfly of another shape and stays in stats.)
#pragma once

#include <hip/hip_runtime.h>

// The sum over each group of G adjacent lanes (G a power of two up to 64).
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v)
{
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return group_sum<64>(v); }

__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}
