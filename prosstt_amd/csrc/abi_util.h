// What a library behind a C ABI needs besides its kernels: the error plumbing, the refusals of a matrix argument, and the
// launch geometry of a "strip of genes over a range of rows" kernel (the host half of a strip kernel).  The device half is
// strip_device.h (a lane's genes, its four counts of a row, the slab stores and fold); wave_reduce.h holds the wave sums.
// Internal: included by every HIP library but the sampler (Makefile: the rows that list it), each a single translation
// unit, and not installed under include/.  The libraries that read no count matrix (knn, graph, layout, tsne, dpt, cluster)
// use the error plumbing, cdiv, clamp64, pad, aligned and the two refusals only, and include graph_util.h after this file
// for the refusals and grid rules they share.  The strip kernels are those of stats, embed, hvg, markers, ranks, trends and thin.
// embed's two products and mapping's pass multiply on the matrix cores: mfma_device.h holds their operand mapping, row load,
// k-steps and tile map, and the host's choice of a <NT, VEC> instantiation; mapping takes the plumbing and the refusals besides.
// ptree reads float32 panels, not a count matrix, and takes the plumbing, cdiv, pad and the two refusals.
// evaluate reads int32 vectors over the cells and takes the plumbing, cdiv, clamp64, pad and workspace_too_small.
// fit's and regress's passes are column kernels (a lane owns one gene): kColumn, kColumnTile, row_blocking and the two
// refusals of their sizes are here, the device half is column_device.h.
// factors' pass is regress's with a lane per cell: it takes the plumbing, cdiv, clamp64, pad, aligned, kTargetBlocks and the
// two refusals; what it shares with regress (the slabs, the split, the finish) is quasi_device.h.
// The including file defines ABI_EINVAL and ABI_EHIP (its header's error codes) first.
// (prosstt_amd.hip keeps macros of its own: its ABI has an ENOMEM code and reports e.what().)
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <new>

#if !defined(ABI_EINVAL) || !defined(ABI_EHIP)
#error "define ABI_EINVAL and ABI_EHIP before including abi_util.h"
#endif

#define ABI_EXPORT extern "C" __attribute__((visibility("default")))
// the tail of an entry point's function-try-block: no exception crosses the C ABI
#define ABI_CATCH                                                                                  \
    catch (const std::bad_alloc&) { return fail(ABI_EINVAL, "out of host memory"); }               \
    catch (...) { return fail(ABI_EINVAL, "unexpected exception"); }

static thread_local char g_err[512] = "";      // what the library's *_last_error returns

static int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return fail(ABI_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

namespace {

constexpr int kThreads = 256;               // 4 waves
constexpr int kStrip = 4 * kThreads;        // genes per block of a strip kernel: one 16-byte load per lane and row
constexpr int kStripMinRows = 64;           // a strip kernel's block takes at least this many rows (count_summary's batch)
constexpr int64_t kTargetBlocks = 1024;     // one round of blocks: about four per CU on 256 CUs
constexpr int kColumn = kThreads;           // genes per block of a column kernel: one per lane
constexpr int kColumnTile = 8;              // rows of a column kernel's LDS tile: two 16-byte loads per lane

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline size_t pad(size_t b) { return (b + 255) & ~size_t(255); }

// May every row be read with loads of `elems` counts (16 bytes: 4, 8 bytes: 2)?
inline bool aligned(const void* p, int64_t ld, int elems)
{
    return ((uintptr_t)p % (4 * elems) == 0) && (ld % elems == 0);
}

// The refusals of a matrix argument.  The bounds on G and their messages differ between the libraries and stay there.
inline bool cells_out_of_range(int64_t N) { return N < 1 || N >= (int64_t(1) << 31); }

inline int stride_below_row(int64_t ld, int64_t G)
{
    return fail(ABI_EINVAL, "row stride %lld is below the row length %lld", (long long)ld, (long long)G);
}

inline int workspace_too_small(uint64_t have, size_t need)
{
    return fail(ABI_EINVAL, "workspace of %llu bytes, %llu needed", (unsigned long long)have, (unsigned long long)need);
}

// How a kernel whose blocks own `strips` strips of genes cuts N rows: 1024 / strips blocks, at most ceil(N / 64), of equal size.  A
// function of (N, strips) alone; a gene's sums are added within a block and then over the blocks, so it is part of the result.
struct RowBlocking {
    int64_t rows_per_block = 0, row_blocks = 0;
};

inline RowBlocking row_blocking(int64_t N, int64_t strips)
{
    RowBlocking b;
    // (rounded down: a second round of a few blocks would cost as much as the first)
    const int64_t rb = clamp64(kTargetBlocks / strips, 1, cdiv(N, kStripMinRows));
    b.rows_per_block = cdiv(N, rb);
    b.row_blocks = cdiv(N, b.rows_per_block);
    return b;
}

// The grid of a strip kernel: blockIdx.x owns the genes [kStrip x, kStrip (x + 1)), blockIdx.y the rows
// [rows_per_block y, rows_per_block (y + 1)).  All zeros when G == 0.  (The mapping of a lane to its four genes is
// strip_device.h's.  count_summary_kernel takes it for g0, the whole-strip test and its stores, with the same loops and
// registers; inside its accumulate and rows4 the shared strip_gene changed the register allocation again, 122 / 124 VGPRs to
// 114 / 112, and there the mapping stays written out.)
struct StripGeometry {
    int64_t strips = 0, row_blocks = 0, rows_per_block = 0;
};

inline StripGeometry strip_geometry(int64_t N, int64_t G)
{
    StripGeometry g;
    g.strips = cdiv(G, kStrip);
    if (g.strips > 0) {
        const RowBlocking b = row_blocking(N, g.strips);
        g.rows_per_block = b.rows_per_block;
        g.row_blocks = b.row_blocks;
    }
    return g;
}

// The refusals of a column library's sizes: the matrix, and the finishing grid of threads_per_gene G / 256 blocks.
inline int column_matrix_refused(int64_t N, int64_t G)
{
    if (cells_out_of_range(N) || G < 1)
        return fail(ABI_EINVAL, "need 1 <= N < 2^31 and G >= 1 (got N = %lld, G = %lld)", (long long)N, (long long)G);
    return 0;
}

inline int column_finish_refused(int64_t G, int64_t threads_per_gene)
{
    if (G > ((int64_t(1) << 31) - 1) * kThreads / threads_per_gene)
        return fail(ABI_EINVAL, "too many genes for one launch (G = %lld)", (long long)G);
    return 0;
}

}  // namespace
