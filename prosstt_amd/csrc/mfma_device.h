// The device half of a matrix-core product of the int32 count matrix with a float32 panel, and the choice of its
// instantiation on the host.  Internal: included after abi_util.h by embed/embed.hip and mapping/mapping.hip, not installed
// under include/.
//
// A wave of 64 lanes owns a 32 x 32 NT tile of the result, as NT accumulators of v_mfma_f32_32x32x2_f32 (exact binary32 fma
// chains), and runs over the summed index in steps of kStep = 32.  With h = lane >> 5 and c = lane & 31:
//   the operands   lane (h, c) holds the 16 values of the step at the summed indices 16h .. 16h + 15 for row c of its tile
//                  (load_row16: 16 consecutive counts of its matrix row) and feeds value s in k-step s.  So the MFMA's k index
//                  is a permutation of the step: in k-step s, lane half h supplies index 16h + s, and the panel must be fed the
//                  same way: the block stages the step's slice as sh[index][column] and lane (h, c) reads column 32 t + c at
//                  index 16h + s for tile t.  A slice staged one way with values fed another gives products that are silently
//                  wrong.
//   the slice      a row of the staged slice is slice_stride(NT) = 32 NT + 2 floats: the two lane halves read rows 16 apart,
//                  which the 2 extra floats put 32 banks apart.  How a thread loads and stores its share of the slice
//                  (load_panel, stage_panel: row-major in embed, node-major and transposed in mapping) is the library's.
//   the result     C/D map of a 32 x 32 tile: column c, row tile_row(reg, h) = (reg & 3) + 8 (reg >> 2) + 4 h for register
//                  reg = 0 .. 15 of the accumulator.
// Masked rows, summed indices and columns are zeros, so every shape runs the same code.
//
// Every function here is inlined.  DESIGN.md, section 29, compares each kernel's machine code with the same kernel written
// out; where sharing changed a kernel the code stays written out, with a line that names this file.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kStep = 32;                   // summed indices per step of the k loop

constexpr int slice_stride(int nt) { return 32 * nt + 2; }

__device__ __forceinline__ f32x16 mfma(float a, float b, const f32x16& c)
{
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int tile_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// The lane's 16 counts of one step: genes g0 + 16h .. g0 + 16h + 15 of its row (zeros outside the row or from `end` on).
// VEC (aligned(X, ld, 4)) and a whole step: four 16-byte loads.
template <bool VEC>
__device__ __forceinline__ void load_row16(int32_t (&x)[16], const int32_t* __restrict__ rp, bool row_ok, int64_t g0,
                                           int64_t end, int h)
{
    const int64_t g = g0 + 16 * h;
    if (VEC && row_ok && g0 + kStep <= end) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int4 v = *reinterpret_cast<const int4*>(rp + g + 4 * q);
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) x[q] = (row_ok && g + q < end) ? rp[g + q] : 0;
    }
}

// The 16 k-steps of one step over the staged slice sh: acc[t] += a . slice columns 32 t .. 32 t + 31.
template <int NT>
__device__ __forceinline__ void mfma_steps(f32x16 (&acc)[NT], const float (&a)[16], const float* sh, int h, int c)
{
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float* b = sh + (16 * h + s) * slice_stride(NT) + c;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma(a[s], b[32 * t], acc[t]);
    }
}

// The same for a lane with two rows u = 0, 1 of the result (two accumulator sets); a slice value is read once for both.
template <int NT>
__device__ __forceinline__ void mfma_steps(f32x16 (&acc)[2][NT], const float (&a)[16][2], const float* sh, int h, int c)
{
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const float* b = sh + (16 * h + s) * slice_stride(NT) + c;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float bv = b[32 * t];
            acc[0][t] = mfma(a[s][0], bv, acc[0][t]);
            acc[1][t] = mfma(a[s][1], bv, acc[1][t]);
        }
    }
}

// The host's choice of a product kernel's instantiation: f(NT, VEC) with the two template arguments as
// std::integral_constant<int, 1 .. 4> and std::bool_constant; a tile count outside 1 .. 3 runs 4.
template <typename F>
void with_instantiation(int64_t nt, bool vec, F f)
{
    auto with_vec = [&](auto tiles) {
        if (vec) f(tiles, std::true_type{});
        else f(tiles, std::false_type{});
    };
    switch (nt) {
    case 1: with_vec(std::integral_constant<int, 1>{}); break;
    case 2: with_vec(std::integral_constant<int, 2>{}); break;
    case 3: with_vec(std::integral_constant<int, 3>{}); break;
    default: with_vec(std::integral_constant<int, 4>{}); break;
    }
}
