// The float32 entry A[i][j] = log1p(X[i][j] * inv_size[i]) of the log-normalised count matrix, formed in registers: one
// definition for every library that reads the matrix this way, so that their entries are equal to the bit.
// Internal: included by embed/embed.hip, markers/markers.hip, ranks/ranks.hip, hvg/hvg.hip (which takes the product
// scaled() alone) and autocorr/autocorr.hip, and not installed under include/.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr float kLn2 = 0.693147180559945309f;

// y = x / s in f32: the count as a float32 times inv = fl32(1 / s), one rounding each.
__device__ __forceinline__ float scaled(int32_t x, float inv) { return (float)x * inv; }

// log1p(x * inv) in f32, relative error below 2^-20 against binary64 log1p(x / s): u = fl(1 + y) and u - 1 is exact, so
// log1p(y) = log(u) * y / (u - 1) loses only the roundings of v_log_f32, v_rcp_f32 (2^-23 each) and four products; when
// u == 1, log1p(y) = y to within y / 2 < 2^-25.
__device__ __forceinline__ float entry(int32_t x, float inv)
{
    const float y = scaled(x, inv);
    const float u = 1.0f + y;
    const float d = u - 1.0f;
    const float r = (__builtin_amdgcn_logf(u) * kLn2) * (y * __builtin_amdgcn_rcpf(d));
    return d == 0.0f ? y : r;
}

}  // namespace
