// The quasi-likelihood sums of the count model, which regress (per gene, over the cells) and factors (per cell, over the
// genes) both add: the quasi-score U, the information I and the quasi-log-likelihood Q of a unit's entries.
// Internal: included after abi_util.h and column_device.h by regress/regress.hip and factors/factors.hip, not installed under
// include/.  DESIGN.md, section 36, says what is shared here and what stays written out in the two kernels, and why.
//
// The definition, operation for operation, in binary64 with nothing contracted.  An entry x >= 0 of a unit (regress: a gene,
// factors: a cell) has a row F[0 .. p) of factors (the design row of the entry's cell; the loadings of the entry's gene), the
// unit's coefficients c[0 .. p), a size factor s in (0, kQuasiLargest] and admissible parameters (a, b) (column_admissible).
//   eta    from +0, eta = eta + F[j] c[j] for j = 0, 1, ... ascending, in groups of four: the groups below p are added whole
//          (beyond p both factors are +0, and adding their product changes no bit of eta)
//   refuse x >= 0 must hold, else the entry adds nothing (the NEGATIVE bit is set from the OR of the entries);
//          |eta| <= kQuasiEtaMax must hold (a NaN fails), else the entry sets the ETA bit and adds nothing
//   mu     mu = s exp(eta);  amu = a mu;  d = amu + b
//   refuse d <= kBig must hold (mu overflowed: infinite, or a NaN from 0 times infinity), else ETA as above
//   w, u   w = mu / d;  u = ((double)x - mu) / d;  regress's second = meat ? u u : w, refused with ETA unless <= kBig
//          (factors has no meat: its second is w)
//   Q      l1 = log1p(amu / b);  t = a > 0 ? l1 / a : mu / b;  full = ((double)x / b) ((eta + log s) - (log b + l1)) - t;
//          q = q + (x == 0 ? -t : full);  used counts the entries added
//   sums   p + p (p + 1) / 2 of them (quasi_sums), in the order U, I, then Q in slot `sums`:
//          sum j < p is U[j] += F[j] u;  sum p + (the place of (j, k), j <= k, in the upper triangle packed by rows) is
//          I[j, k] += (F[j] F[k]) second, the product of the two factors rounded first
// A unit's terms are added in ascending order of its entries within a block, from +0, and the blocks' sums in ascending block
// order by the finish kernel (quasi_finish): the order is part of the result.
//
// The split.  A block keeps ACC = 8, 16 or 32 of the sums in registers: block z of blockIdx.z owns the sums
// [ACC z, ACC z + ACC) (quasi_block_sums).  Every block forms eta, mu, w and u of its entries itself, by the operations above,
// so the sums do not depend on ACC.  The instantiation ACC = 0 is the Q pass: it adds Q and used and no sum of (U, I), which
// keeps log1p, log and their constants out of the other kernels' registers.  quasi_split resolves split = 0 (16 sums per block
// up to kQuasiSplit16MaxSums sums, 32 above) and refuses anything but 8, 16, 32; quasi_passes launches the sums pass and then
// the Q pass.
//
// The two tables.  A block's sums multiply a factor by u (a sum of U) or by second (a sum of I).  A block whose sums are all
// of one kind keeps one table, s_factor, and its loop is acc[i] = acc[i] + s_factor[i] v with v = u or second.  A block that
// has both (`mixed`: at most one layer of blocks per call, where the sums of U end) keeps two, with the factor of a sum of U in s_factor and 0
// in s_second and the other way round for a sum of I (quasi_factor_tables), and adds
// acc[i] = (acc[i] + s_factor[i] u) + s_second[i] second: one of the two products is a zero of either sign, and a sum that
// started from +0 is never -0, so adding a zero of either sign changes no bit of it.
// A slot beyond the block's last sum has the factor 0 in both tables and is not stored.
//
// The slabs.  [blocks][sums + 1][len] binary64 (U, I, then Q) and [blocks][len] uint32 (used), each padded to 256 bytes
// (quasi_slabs); `blocks` is the file's own blocking (regress: of the rows; factors: of the genes), `len` the units.
//
// What is NOT a function here, because as one it changed the machine code of a loop (section 36 has the counts): eta, the
// Q term, the accumulation loops, and the walk from a sum's index to its (j, k).  They stay written out in both kernels, each
// under a comment that names this definition.
#pragma once

#include <type_traits>

namespace {

constexpr double kQuasiLargest = 1e150;        // the largest size factor
constexpr double kQuasiEtaMax = 700.0;
constexpr int kQuasiSplit16MaxSums = 48;       // (both public headers state it: PROSSTT_AMD_*_SPLIT_16_MAX_SUMS)

inline int64_t quasi_sums(int64_t p) { return p + p * (p + 1) / 2; }

// The offsets of the two slabs in the workspace, and its size.
struct QuasiSlabs {
    size_t slab = 0, used = 0, bytes = 0;
};

inline QuasiSlabs quasi_slabs(int64_t blocks, int64_t sums, int64_t len)
{
    QuasiSlabs s;
    const size_t units = (size_t)blocks * (size_t)len;
    s.slab = 0;
    s.used = s.slab + pad(units * (size_t)(sums + 1) * 8);
    s.bytes = s.used + pad(units * 4);
    return s;
}

// split = 0 becomes the library's choice; anything but 8, 16 and 32 is refused.
inline int quasi_split(int64_t p, int32_t& split)
{
    // (measured at 50 000 x 20 000: 16 is the fastest split at 14 and at 44 sums, 32 at 152; nothing between was timed.
    // DESIGN section 35 holds what was measured for factors)
    if (split == 0) split = quasi_sums(p) <= kQuasiSplit16MaxSums ? 16 : 32;
    if (split != 8 && split != 16 && split != 32) return fail(ABI_EINVAL, "split must be 0, 8, 16 or 32 (got %d)", (int)split);
    return 0;
}

// The sums pass with ACC = split, then the Q pass: pass(std::integral_constant<int, ACC>) launches one instantiation.
template <class Pass>
int quasi_passes(int32_t split, Pass&& pass)
{
    if (split == 8)
        pass(std::integral_constant<int, 8>{});
    else if (split == 16)
        pass(std::integral_constant<int, 16>{});
    else
        pass(std::integral_constant<int, 32>{});
    HIP_TRY(hipGetLastError());
    pass(std::integral_constant<int, 0>{});
    HIP_TRY(hipGetLastError());
    return 0;
}

// Which of the sums the block owns (blockIdx.z; ACC = 0: none).
struct QuasiBlockSums {
    int a0;                         // the block's first sum
    int na;                         // how many it has
    int nu;                         // how many of them are sums of U (the first ones)
    bool mixed;                     // sums of U and of I: two factors per sum, one of them 0
};

template <int ACC>
__device__ __forceinline__ QuasiBlockSums quasi_block_sums(int p, int sums)
{
    QuasiBlockSums b;
    b.a0 = (int)blockIdx.z * ACC;
    b.na = ACC == 0 ? 0 : ((sums - b.a0 < ACC) ? sums - b.a0 : ACC);
    b.nu = (p - b.a0 < 0) ? 0 : ((p - b.a0 < b.na) ? p - b.a0 : b.na);
    b.mixed = b.nu > 0 && b.nu < b.na;
    return b;
}

// A slot's entries of the two tables from its factor v (0 beyond the block's last sum).
__device__ __forceinline__ void quasi_factor_tables(double& factor, double& second, bool mixed, bool fpair, double v)
{
    factor = (mixed && fpair) ? 0.0 : v;
    second = (mixed && fpair) ? v : 0.0;
}

// The finish kernel's body.  One thread per (sum, unit) and one per unit: i < (sums + 1) len adds a slab's partial sums -- sums
// of U, then of I, then Q; (sums + 1) len <= i < (sums + 2) len adds used's.
__device__ __forceinline__ void quasi_finish(const double* __restrict__ slab, const uint32_t* __restrict__ usedslab, int64_t len,
                                             int64_t p, int64_t sums, int64_t blocks, double* __restrict__ U,
                                             double* __restrict__ I, double* __restrict__ Q, uint64_t* __restrict__ used)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t SL = (sums + 1) * len;
    if (i < SL) {
        double sum = 0.0;
        for (int64_t b = 0; b < blocks; ++b) sum += slab[b * SL + i];
        if (i < p * len)
            U[i] = sum;
        else if (i < sums * len)
            I[i - p * len] = sum;
        else
            Q[i - sums * len] = sum;
    } else if (i < SL + len) {
        const int64_t unit = i - SL;
        uint64_t n = 0;
        for (int64_t b = 0; b < blocks; ++b) n += usedslab[b * len + unit];
        used[unit] = n;
    }
}

}  // namespace
