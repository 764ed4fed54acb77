/*
 * prosstt_amd_thin.h -- binomial thinning of a device count matrix (libprosstt_amd_thin.so; prosstt_amd/thin.py drives it).
 *
 * A count x is split at random into a part y ~ Binomial(x, p) and the rest x - y.  Fitting on one part and scoring on the
 * other (molecular cross-validation, count splitting) chooses a rank, a bandwidth or a node count without a truth: for a
 * Poisson count the parts are independent Poisson counts, and under the simulator's gamma-Poisson law they stay Poisson
 * given the entry's rate.  The same primitive with one p per cell lowers the depth of a matrix (scanpy's
 * pp.downsample_counts, as binomial thinning).  Integer arithmetic only.
 *
 * THIN-1, the definition
 *   grid      Probabilities live on a grid of 2^-16.  A part of a count is named by a half-open interval [lo, hi) with
 *             0 <= lo <= hi <= 65536.
 *   trials    The entry of cell c (int64 >= 0), gene g (int64 >= 0) with count x has the trials t = 0 .. x - 1.
 *   uniforms  Trial t has a 16-bit uniform U_t.  Bit 15 - b of U_t is bit (t mod 64) of the 64-bit word
 *             W(seed, c, g, floor(t / 64), b), for the planes b = 0 .. 15: plane 0 holds the most significant bits.
 *   the hash  With 64-bit wrapping arithmetic and mix the splitmix64 finaliser (layout.hip's mix)
 *               mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *               Kc = mix(seed ^ mix(c + 0xE7037ED1A0B428DB))            the cell half of the key
 *               Kg = mix(g + 0xA0761D6478BD642F)                        the gene half
 *               K  = mix(Kc ^ Kg)                                       the entry's key
 *               W(seed, c, g, w, b) = mix(K + 0x9E3779B97F4A7C15 * (16 w + b + 1))
 *             a function of exactly those five numbers: splitmix64's stream from the state K, word 16 w + b.
 *   value     y = #{t < x : lo <= U_t < hi}.
 * What follows from it is the contract: y ~ Binomial(x, (hi - lo) / 65536); the parts of disjoint intervals add up
 * exactly -- those of [lo, mid) and [mid, hi) to that of [lo, hi), and [0, 65536) gives x; the trials of a smaller count
 * are a prefix of those of a larger one; and nothing depends on where the entry lies in memory, on which other entries
 * are in the call, on the stream or on the launch.
 *
 * How the kernel evaluates it (the same value, 64 trials at a time): for a bound k < 65536 the comparison U < k runs over
 * the planes from 0 down with two words lt = 0 and eq = ~0: where bit 15 - b of k is set, lt |= eq & ~W and eq &= W;
 * otherwise eq &= ~W.  A bound of 65536 is lt = ~0.  The trials inside are lt_hi & ~lt_lo, masked to x mod 64 in the last
 * word and counted.  Planes below the lowest set bit of (lo | hi) mod 65536 cannot change lt and are not generated: a
 * split at 1/2 costs one word per 64 trials, a bound of 0 or 65536 no plane.
 *
 * Conventions (as in prosstt_amd_hvg.h)
 *  - extern "C", plain pointers and sizes; never throws.
 *  - return 0 on success, a negative PROSSTT_AMD_THIN_E* code otherwise; the message is in the thread-local
 *    last_error string.  Bad sizes are refused before anything is enqueued.
 *  - Array arguments are DEVICE pointers.  All work is enqueued on the caller's stream (NULL: the default stream of the
 *    current device); nothing synchronises, nothing allocates device memory, and no workspace is needed.
 *  - X: row r, column j at X[r*ld + j] (unit column stride, row stride ld >= G; any base alignment).  Y and R likewise
 *    with ldy and ldr.  When every row of X, Y and R (if given) starts on 16 bytes, rows are read and written in 16-byte
 *    pieces; otherwise in 4-byte pieces.
 *  - *status is only ever set (the caller zeroes it).  An entry that sets a bit is written as 0 in Y and in R and is
 *    never drawn; every other entry is still right.
 *  - Limits, refused with PROSSTT_AMD_THIN_EINVAL: 1 <= N < 2^31, 1 <= G, ld, ldy, ldr >= G, cell_offset and gene_offset
 *    >= 0, lo <= hi <= 65536 where they are given as one value, an output that overlaps X or the other output.
 */
#ifndef PROSSTT_AMD_THIN_H
#define PROSSTT_AMD_THIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    PROSSTT_AMD_THIN_OK = 0,
    PROSSTT_AMD_THIN_EINVAL = -1, /* bad argument */
    PROSSTT_AMD_THIN_EHIP = -3    /* HIP runtime error */
};

#define PROSSTT_AMD_THIN_GRID 65536u           /* the grid of probabilities: 2^16 */
#define PROSSTT_AMD_THIN_MAX_COUNT 16777216    /* 2^24: the largest count that is drawn (2^18 words of 64 trials) */

#define PROSSTT_AMD_THIN_NEGATIVE 1u /* status: a negative entry of X */
#define PROSSTT_AMD_THIN_OVER 2u     /* status: an entry of X above PROSSTT_AMD_THIN_MAX_COUNT */
#define PROSSTT_AMD_THIN_RANGE 4u    /* status: a row of the lo / hi tables with lo > hi or hi > 65536 (the whole row is 0) */

const char* prosstt_amd_thin_last_error(void);

/*
 * How a call with these arguments is laid out, without a device: *vec = 1 when rows go in 16-byte pieces (the aligned
 * instantiation), *strips blocks of 1024 genes (the last one ragged unless G is a multiple of 1024), *row_blocks blocks of
 * *rows_per_block rows.  The pointers are only looked at (R may be NULL).  None of it is part of the result.
 */
int prosstt_amd_thin_plan(int64_t N, int64_t G, const int32_t* X, int64_t ld, const int32_t* Y, int64_t ldy,
                          const int32_t* R, int64_t ldr, int32_t* vec, int64_t* strips, int64_t* row_blocks,
                          int64_t* rows_per_block);

/*
 * Y[r][j] = the part [lo, hi) of X[r][j] by THIN-1, with cell c = cell_ids[r] (N int64 on the device, each >= 0) or
 * cell_offset + r when cell_ids is NULL, and gene g = gene_offset + j.  lo and hi are lo_table[r] and hi_table[r] (N
 * uint32 on the device each) where the table is given, else the values lo_all and hi_all.  R, if not NULL, receives the
 * complement X - Y in the same pass.
 */
int prosstt_amd_thin_interval(void* stream, const int32_t* X, int64_t N, int64_t G, int64_t ld, uint64_t seed,
                              const int64_t* cell_ids, int64_t cell_offset, int64_t gene_offset, uint32_t lo_all,
                              uint32_t hi_all, const uint32_t* lo_table, const uint32_t* hi_table, int32_t* Y, int64_t ldy,
                              int32_t* R, int64_t ldr, uint32_t* status);

#ifdef __cplusplus
}
#endif
#endif
