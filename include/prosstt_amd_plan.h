/*
 * prosstt_amd_plan.h -- the strip plan of the sampler's stream kernel: two further entry points of libprosstt_amd.so, for
 * tests and diagnostics.  (They are declared here and not in prosstt_amd.h, whose symbols tests/test_native_libraries.py
 * counts; prosstt_amd/_native.py lists them in SAMPLER_LATER.)  Conventions as in prosstt_amd.h: 0 on success, a negative
 * PROSSTT_AMD_E* code otherwise, the message where the library keeps its last error.
 */
#ifndef PROSSTT_AMD_PLAN_H
#define PROSSTT_AMD_PLAN_H

#include "prosstt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells every wave of the stream kernel takes (host helper, no device work): the strip plan of a
 * prosstt_amd_sample_counts call of N cells x G genes on a device that holds `resident_blocks` blocks of that kernel at
 * once (5 per compute unit).  Up to 4 classes, class k = classes[3k .. 3k+2] = {first cell, strip length, first block}:
 * class k is the cells from its first cell to the next class's (the last: to N) in strips of its length, one per wave;
 * a block is four adjacent strips of one 256-gene tile, and blocks are numbered class by class, within a class tile by
 * tile.  The length of a uniform launch is 64 cells, halved (down to 8) while it would have fewer than 20 480 blocks;
 * strip_cells = 8, 16, 32 or 64 sets it instead (0: by the rule; 128 stands for 64 here).  A uniform launch of fewer than
 * 4 * resident_blocks blocks is the plan; a larger one -- or any, with taper > 0, which then stands for resident_blocks --
 * is graded: its bulk length is 128 where the uniform one is 64 by the rule (or strip_cells = 128), else the uniform one,
 * and classes of half, a quarter and an eighth of the bulk length follow (none under 8 cells), each of resident_blocks * 4 *
 * length / tiles cells rounded to the nearest multiple of 64, at least 64; the bulk class is the rest rounded down to whole
 * strips and a multiple of 64 (a short class that would leave it less than a strip is not made), the last class takes the
 * remainder.  The run
 * words of a cell (prosstt_amd_run_plan) are those of its class's strip length.  `classes` holds 12 entries;
 * *tiles_g and *blocks (either may be NULL) receive the gene tiles and the blocks of the launch.
 */
int prosstt_amd_strip_plan(int64_t N, int32_t G, int32_t resident_blocks, int32_t strip_cells, int32_t taper,
                           int32_t* classes, int32_t* n_classes, int32_t* tiles_g, int32_t* blocks);

/* The plan of the LAST prosstt_amd_sample_counts call on this ctx (*n_classes = 0: there was none). */
int prosstt_amd_last_strip_plan(prosstt_amd_ctx* ctx, int32_t* classes, int32_t* n_classes, int32_t* tiles_g, int32_t* blocks);

#ifdef __cplusplus
}
#endif

#endif
