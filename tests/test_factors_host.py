"""The host side of prosstt_amd/factors.py without a GPU: every refusal of the wrapper (all before any device use), the
limits and status bits against include/prosstt_amd_factors.h, the gene blocking against the built library's own answer,
``CellEquations.concat``, and the refusals of the C ABI that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import factors_model as M
from conftest import ROOT

from prosstt_amd import _native, factors, regress

HEADER = open(os.path.join(ROOT, "include", "prosstt_amd_factors.h")).read()


def _define(name):
    return int(re.search(r"^#define PROSSTT_AMD_FACTORS_%s\s+(-?\d+)u?\b" % name, HEADER, re.M).group(1))


def test_the_constants_are_the_headers():
    assert factors.MAX_P == _define("MAX_P") == regress.MAX_P and factors.MAX_K == factors.MAX_P - 1
    assert factors.TILE_GENES == _define("TILE_GENES")
    for name in ("NEGATIVE", "PARAMETER", "SIZE", "COEFFICIENT", "ETA"):
        assert getattr(factors, name) == _define(name) == getattr(regress, name)       # named and numbered as in regress
    assert {bit for bit, _, _ in factors.STATUS_MESSAGES} == {factors.NEGATIVE, factors.PARAMETER, factors.SIZE, factors.COEFFICIENT,
                                                              factors.ETA}
    assert _define("SPLIT_16_MAX_SUMS") == 48 and regress.SPLITS == (8, 16, 32)
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "prosstt_amd", "csrc", "Makefile")).read()


def test_refusals_of_the_matrix_the_options_and_the_shapes():
    X = torch.zeros((6, 4), dtype=torch.int32)
    sc, L, coef = np.ones(6), np.ones((4, 2)), np.zeros((6, 2))
    with pytest.raises(TypeError, match="host arrays are refused"):
        factors.cell_equations(X.numpy(), sc, L, coef, 0.2, 2.0)
    with pytest.raises(TypeError, match="needs int32 counts"):
        factors.cell_equations(X.long(), sc, L, coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="needs a device tensor"):
        factors.cell_equations(X, sc, L, coef, 0.2, 2.0)
    with pytest.raises(ValueError, match="at least one cell and one gene"):
        factors.cell_equations(X[:0], sc[:0], L, coef[:0], 0.2, 2.0)
    with pytest.raises(ValueError, match="out must be"):
        factors.cell_equations(X, sc, L, coef, 0.2, 2.0, out="cupy")
    for split in (4, 64, True, 16.5):
        with pytest.raises(ValueError, match="split must be 0"):
            factors.cell_equations(X, sc, L, coef, 0.2, 2.0, split=split)
    for per in (-32, 31, 48, True, 32.0):
        with pytest.raises(ValueError, match="genes_per_block must be 0"):
            factors.cell_equations(X, sc, L, coef, 0.2, 2.0, genes_per_block=per)
    with pytest.raises(ValueError, match="need 1 <= p <= %d coefficients" % _define("MAX_P")):
        factors.cell_equations(X, sc, np.ones((4, 17)), np.zeros((6, 17)), 0.2, 2.0)
    with pytest.raises(ValueError, match=r"loadings must be a \(genes, p\) = \(4, p\) array"):
        factors.cell_equations(X, sc, np.ones((3, 2)), coef, 0.2, 2.0)
    with pytest.raises(ValueError, match=r"loadings must be a \(genes, p\)"):
        factors.cell_equations(X, sc, np.ones(4), coef, 0.2, 2.0)
    with pytest.raises(ValueError, match=r"coef must be \(cells, p\) = \(6, 2\)"):
        factors.cell_equations(X, sc, L, np.zeros((2, 6)), 0.2, 2.0)
    with pytest.raises(ValueError, match="alpha must be a number or one per gene"):
        factors.cell_equations(X, sc, L, coef, np.ones(3), 2.0)
    with pytest.raises(ValueError, match="beta must be a number or one per gene"):
        factors.cell_equations(X, sc, L, coef, 0.2, np.ones(6))
    with pytest.raises(ValueError, match="need one size factor per cell"):
        factors.cell_equations(X, sc[:5], L, coef, 0.2, 2.0)
    for use in (np.zeros(3, dtype=int), np.zeros(4), ["a", "b", "c", "d"]):
        with pytest.raises(ValueError, match="use must be one integer or boolean per gene"):
            factors.cell_equations(X, sc, L, coef, 0.2, 2.0, use=use)
    with pytest.raises(ValueError, match="status bit NEGATIVE .*; status bit ETA"):
        factors.check_status(factors.ETA | factors.NEGATIVE)
    with pytest.raises(RuntimeError, match="unknown status bit"):
        factors.check_status(2)                                  # regress's label bit means nothing here
    factors.check_status(0)
    assert factors._use([True, False, True], 3).tolist() == [0, -1, 0] and factors._use([5, -7, 0], 3).tolist() == [0, -1, 0]


def test_refusals_of_glmpca_before_any_device_use():
    X = torch.zeros((40, 30), dtype=torch.int32)
    sc = np.ones(40)
    for options, message in ((dict(k=0), "1 <= k <= 15"), (dict(k=16), "1 <= k <= 15"), (dict(k=2.0), "1 <= k <= 15"),
                             (dict(k=True), "1 <= k <= 15"), (dict(max_rounds=0), "max_rounds"), (dict(tol=0.0), "tol must be"),
                             (dict(penalty=-1.0), "penalty must be"), (dict(penalty=np.nan), "penalty must be"),
                             (dict(split=7), "split must be"), (dict(init="svd"), "init must be"),
                             (dict(init=np.zeros((40, 3))), "init must be"), (dict(init=np.full((40, 10), np.nan)), "init must be"),
                             (dict(alpha=np.ones(3)), "alpha must be")):
        args = dict(alpha=0.2, beta=2.0)
        args.update(options)
        with pytest.raises(ValueError, match=message):
            factors.glmpca(X, sc, **args)
    with pytest.raises(ValueError, match="need more than 12 cells and genes"):
        factors.glmpca(X[:, :12], sc, 12, alpha=0.2, beta=2.0)
    with pytest.raises(TypeError, match="host arrays are refused"):
        factors.glmpca(X.numpy(), sc, 3, alpha=0.2, beta=2.0)
    with pytest.raises(ValueError, match="need one size factor per cell"):
        factors.glmpca(X, sc[:5], 3, alpha=0.2, beta=2.0)
    with pytest.raises(ValueError, match="needs a device tensor"):
        factors.glmpca(X, sc, 3, alpha=0.2, beta=2.0, init="random")


def _library():
    """The built library (build() makes it on any machine: a missing file fails here, it does not skip)."""
    return _native.load("factors")


def test_gene_blocks_is_the_librarys_own_rule():
    assert factors.gene_blocks(1, 1) == (32, 1) and factors.gene_blocks(257, 513) == (128, 5) and factors.gene_blocks(700, 513, 32) == (32, 17)
    assert factors.gene_blocks(50000, 20000) == (1024, 20) and factors.gene_blocks(3000, 300) == (128, 3)
    assert factors.gene_blocks(50000, 2000) == (416, 5) and factors.gene_blocks(2 ** 31 - 1, 2 ** 31 - 1)[1] <= 65535
    assert factors.gene_blocks(5, 100, 4096) == (128, 1)         # one block: no more than the genes' tiles
    lib = _library()
    need = ctypes.c_uint64(0)
    for N, G in ((1, 1), (1, 513), (257, 513), (700, 513), (3000, 300), (50000, 20000), (300000, 33), (2 ** 31 - 1, 2 ** 31 - 1)):
        per, blocks = factors.gene_blocks(N, G)
        assert factors.gene_blocking(N, G) == per and per % factors.TILE_GENES == 0
        for p in (1, 7, 16):
            # the slabs [blocks][sums + 1][N] of binary64 and [blocks][N] of uint32, each padded to 256 bytes
            sums = p + p * (p + 1) // 2
            want = -(-blocks * N * (sums + 1) * 8 // 256) * 256 + -(-blocks * N * 4 // 256) * 256
            assert lib.prosstt_amd_factors_workspace_bytes(N, G, p, 0, ctypes.byref(need)) == 0 and need.value == want, (N, G, p)
            assert lib.prosstt_amd_factors_workspace_bytes(N, G, p, per, ctypes.byref(need)) == 0 and need.value == want
    blocks = factors.gene_blocks(700, 513, 32)[1]
    assert lib.prosstt_amd_factors_workspace_bytes(700, 513, 3, 32, ctypes.byref(need)) == 0
    assert need.value == -(-blocks * 700 * 10 * 8 // 256) * 256 + -(-blocks * 700 * 4 // 256) * 256


def test_the_abi_refuses_bad_sizes_before_anything_is_enqueued():
    """No device is needed: every refusal comes before the first use of a pointer or the runtime."""
    lib = _library()
    need, per = ctypes.c_uint64(0), ctypes.c_int64(0)
    E = _native.EINVAL
    top = 1 << 31
    for N, G, p, g in ((0, 5, 3, 0), (top, 5, 3, 0), (5, 0, 3, 0), (5, top, 3, 0), (5, 5, 0, 0), (5, 5, _define("MAX_P") + 1, 0),
                       (5, 5, 3, -32), (5, 5, 3, 33), (5, 5, 3, 16), (1, top - 1, 3, 32)):
        assert lib.prosstt_amd_factors_workspace_bytes(N, G, p, g, ctypes.byref(need)) == E, (N, G, p, g)
        assert lib.prosstt_amd_factors_last_error()
    assert b"more than 65535 blocks" in lib.prosstt_amd_factors_last_error()
    assert lib.prosstt_amd_factors_workspace_bytes(5, 5, 3, 0, None) == E
    assert lib.prosstt_amd_factors_gene_blocking(0, 5, ctypes.byref(per)) == E
    assert lib.prosstt_amd_factors_gene_blocking(5, 5, None) == E
    assert lib.prosstt_amd_factors_gene_blocking(top - 1, top - 1, ctypes.byref(per)) == 0 and per.value == 32800        # 65 535 blocks at the most
    one = ctypes.c_void_p(256)                                   # never read: a refusal comes first

    def call(N=5, G=5, ld=5, ldl=3, p=3, split=0, g=0, ws=one, bytes_=1 << 40, X=one, status=one):
        return lib.prosstt_amd_factors_cell_equations(None, X, N, G, ld, one, None, one, ldl, p, one, one, one, split, g, ws, bytes_,
                                                      one, one, one, one, status)
    for bad in (dict(N=0), dict(N=top), dict(G=0), dict(G=top), dict(p=0), dict(p=17, ldl=17), dict(ld=4), dict(ldl=2), dict(split=4),
                dict(split=24), dict(split=-8), dict(g=-32), dict(g=40), dict(ws=None), dict(bytes_=100), dict(X=None), dict(status=None)):
        assert call(**bad) == E, bad
        assert lib.prosstt_amd_factors_last_error()
    assert call(bytes_=100) == E and b"workspace of 100 bytes" in lib.prosstt_amd_factors_last_error()
    assert call(ld=4) == E and b"row stride 4 is below the row length 5" in lib.prosstt_amd_factors_last_error()


def test_concat_puts_the_cells_one_after_the_other_and_refuses_what_does_not_fit():
    rng = np.random.default_rng(2)
    X = rng.poisson(3.0, size=(90, 40))
    sc, L, coef = rng.lognormal(0, 0.3, size=90), rng.normal(0, 0.3, size=(40, 3)), rng.normal(0, 0.2, size=(90, 3))
    whole = M.cell_equations(X, sc, L, coef, 0.2, 2.0).eq
    parts = [M.cell_equations(X[lo:hi], sc[lo:hi], L, coef[lo:hi], 0.2, 2.0).eq for lo, hi in ((0, 30), (30, 50), (50, 90))]
    both = factors.CellEquations.concat(parts)
    assert both.n_cells == 90 and both.n_genes == 40 and both.p == 3 and "cells=90, p=3, genes=40" in repr(both)
    # rows are independent: the chunks hold the bits of the whole
    assert both.score.tobytes() == whole.score.tobytes() and both.information.tobytes() == whole.information.tobytes()
    assert both.q.tobytes() == whole.q.tobytes() and np.array_equal(both.used, whole.used) and both.used.dtype == np.int64
    full = both.symmetric()
    assert full.shape == (90, 3, 3) and np.array_equal(full, full.transpose(0, 2, 1)) and np.array_equal(factors.packed(full), both.information)
    with pytest.raises(ValueError, match="at least one"):
        factors.CellEquations.concat([])
    with pytest.raises(TypeError, match="concat takes CellEquations"):
        factors.CellEquations.concat([parts[0], parts[0].score])
    fewer = M.cell_equations(X[:30, :39], sc[:30], L[:39], coef[:30], 0.2, 2.0).eq
    with pytest.raises(ValueError, match="different genes or coefficients"):
        factors.CellEquations.concat([parts[0], fewer])
    with pytest.raises(ValueError, match="score must be"):
        factors.CellEquations(np.zeros((5, 3)), np.zeros((5, 5)), np.zeros(5), np.zeros(5), 40)


def test_set_design_of_the_regression_pass_keeps_the_shape():
    """The method ``factors.glmpca`` adds to ``regress._Pass``: checked on an object that never saw a device."""
    run = object.__new__(regress._Pass)
    run.K, run.p = 4, 2
    for bad in (np.ones((4, 3)), np.ones((5, 2)), np.ones(4)):
        with pytest.raises(ValueError):
            run.set_design(bad)
    with pytest.raises(ValueError, match="finite"):
        run.set_design(np.full((4, 2), np.nan))
