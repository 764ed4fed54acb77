"""
The rule the sampler's domain check is held to, pinned without a GPU.

``oracle.ref_numpy.domain_error`` evaluates the reference's argument check (``draw_counts``: scipy's
``nbinom(n=r, p=1-p).rvs()`` behind simulation.py:647-648) in binary64 on what the device is given; the kernels implement
its closed form -- a sample is refused iff m = M*s is not a positive finite number or theta = alpha*m + beta - 1 < 0.
Here, on the value table of tests/test_gpu_domain_check.py:

  * the helper equals the closed form on every entry outside the two rounding bands (the entries inside are named);
  * both equal whether scipy's ``rvs()`` raises (the frozen constructor alone does not check its arguments);
  * no sample of any GPU case lies in the rounding band: the device forms theta in binary32 from rounded alpha,
    beta - 1, s and M*s with one fma, at most five roundings of 2^-24 relative to |alpha|*m + |beta - 1|, so an input with
    |theta| <= 2^-20 * (|alpha|*m + |beta - 1|) could legitimately get either verdict and is not allowed as a test input
    (theta exactly 0 from alpha = 0, beta = 1 is exact in every format and is allowed).  The same holds for the reference's
    own cancellation in ``s2 - m`` (``ref_numpy.domain_cancellation_band``).

Range: positive finite means of the cases lie in [1e-100, 1e6].  The reference's own arithmetic breaks below about
1e-154, where ``m ** 2`` underflows and it refuses a positive mean (m = 1e-300 raises); that is outside what the device's
rule answers for and outside these tests.
"""
import itertools

import numpy as np
import pytest

from oracle import ref_numpy
import test_gpu_domain_check as gpu

TABLE = list(itertools.product(gpu.MEAN_VALUES, gpu.SCALING_VALUES, gpu.PARAM_VALUES))


def _one(mean, scaling, alpha, beta):
    return (np.array([[mean]], np.float32), np.zeros(1, np.int32), np.array([scaling]), np.array([alpha]), np.array([beta]))


def _table_arrays():
    """The whole table as one call: a row of the mean tensor per mean, a cell per (mean, scaling), a gene per (alpha, beta)."""
    means = np.repeat(np.array(gpu.MEAN_VALUES, np.float32)[:, None], len(gpu.PARAM_VALUES), axis=1)
    roc = np.repeat(np.arange(len(gpu.MEAN_VALUES)), len(gpu.SCALING_VALUES)).astype(np.int32)
    scaling = np.tile(np.array(gpu.SCALING_VALUES), len(gpu.MEAN_VALUES))
    alpha = np.array([p[0] for p in gpu.PARAM_VALUES])
    beta = np.array([p[1] for p in gpu.PARAM_VALUES])
    return means, roc, scaling, alpha, beta


def test_table_is_the_stated_one():
    assert len(gpu.MEAN_VALUES) == 10 and len(gpu.SCALING_VALUES) == 7 and len(gpu.PARAM_VALUES) == 9
    assert np.float32(1e-45) > 0 and np.float32(1e-45) < np.float32(1.17549435e-38)          # a binary32 denormal
    assert np.float32(1e-50) == 0 and 1e-50 > 0                                               # below binary32's range


def _in_a_band(*x):
    return ref_numpy.domain_rounding_band(*x) | ref_numpy.domain_cancellation_band(*x)


def test_helper_equals_closed_form_on_every_entry():
    """... outside the two bands in which a sign of theta is rounding noise: binary32's (the device's) and the
    reference's own cancellation in ``s2 - m``.  The entries of the table inside a band are exactly the ones named here;
    no GPU case uses them (test_no_gpu_case_in_the_rounding_band)."""
    x = _table_arrays()
    ok = ref_numpy.domain_ok(*x)
    closed = ref_numpy.domain_ok_closed_form(*x)
    assert ok.shape == (70, 9)
    mu = ref_numpy._device_sample_means(*x[:3])
    banded = {(float(mu[i, j]), float(x[3][j]), float(x[4][j])) for i, j in zip(*np.nonzero(_in_a_band(*x)))}
    positive = {float(np.float32(m)) * s for m in gpu.MEAN_VALUES for s in gpu.SCALING_VALUES if 0 < float(np.float32(m)) * s < np.inf}
    # theta = -0.1 m against beta = 1, m below 1e-14 (the reference sees s2 = m, theta = 0, and accepts), and
    # theta = 0.5 - 1e-4 * 5000 (a zero that depends on how 1e-4 is rounded)
    assert banded == {(m, -0.1, 1.0) for m in positive if m < 1e-14} | {(5000.0, -1e-4, 1.5)}
    assert len(banded) == 9
    np.testing.assert_array_equal(ok[~_in_a_band(*x)], closed[~_in_a_band(*x)])
    assert (ok != closed).sum() <= len(banded)
    # entry by entry through the verdict itself, and a few that need no arithmetic to decide
    for mean, scaling, (alpha, beta) in TABLE:
        one = _one(mean, scaling, alpha, beta)
        if not _in_a_band(*one)[0, 0]:
            assert ref_numpy.domain_error(*one) == (not ref_numpy.domain_ok_closed_form(*one)[0, 0]), (mean, scaling, alpha, beta)
    assert not ref_numpy.domain_error(*_one(1.0, 1.0, 0.2, 2.0))
    assert not ref_numpy.domain_error(*_one(1.0, 1.0, 0.0, 1.0))             # theta = 0: valid, all zeros
    assert not ref_numpy.domain_error(*_one(1e-45, 1.0, 0.2, 2.0))
    assert not ref_numpy.domain_error(*_one(1.0, 1e-50, 0.2, 2.0))           # positive in binary64
    assert not ref_numpy.domain_error(*_one(1e-30, 1e-10, 0.2, 2.0))
    for mean in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
        for alpha, beta in gpu.PARAM_VALUES:
            assert ref_numpy.domain_error(*_one(mean, 1.0, alpha, beta))     # +inf whatever alpha and beta are
    for scaling in (0.0, -1.0, np.nan, np.inf):
        assert ref_numpy.domain_error(*_one(1.0, scaling, 0.2, 2.0))
    assert ref_numpy.domain_error(*_one(1.0, 1.0, 0.2, 0.5)) and not ref_numpy.domain_error(*_one(5.0, 1.0, 0.2, 0.5))
    assert ref_numpy.domain_error(*_one(1e-300, 1.0, 0.2, 2.0))              # the reference's own underflow: out of scope
    # no cell, no verdict
    assert not ref_numpy.domain_error(np.zeros((2, 3), np.float32), np.zeros(0, np.int32), np.zeros(0), np.zeros(3), np.zeros(3))


def test_helper_is_draw_counts_rule():
    """``domain_error`` raises exactly where ``ref_numpy.draw_counts`` does on a tree that holds the same means."""
    means, roc, scaling, alpha, beta = _table_arrays()
    for r in range(means.shape[0]):
        tree = ref_numpy.RefTree([], {"A": 1}, num_branches=1, branch_points=0, modules=2, G=means.shape[1])
        tree.means = {"A": means[r:r + 1].astype(np.float64)}
        for s in gpu.SCALING_VALUES:
            want = ref_numpy.domain_error(means[r:r + 1], np.zeros(1, np.int32), np.array([s]), alpha, beta)
            np.random.seed(1)
            try:
                with np.errstate(invalid="ignore"):                 # (0 * inf on the way to the NaN that is refused)
                    ref_numpy.draw_counts(tree, np.array([0]), ["A"], np.array([s]), alpha, beta)
                raised = False
            except ValueError:
                raised = True
            assert raised == want, (gpu.MEAN_VALUES[r], s)


def test_both_equal_scipy_rvs():
    stats = pytest.importorskip("scipy.stats")
    x = _table_arrays()
    ok = ref_numpy.domain_ok(*x)
    closed = ref_numpy.domain_ok_closed_form(*x)
    band = _in_a_band(*x)
    mu = ref_numpy._device_sample_means(*x[:3])
    p, r = ref_numpy.get_pr_umi(x[3][None, :], x[4][None, :], mu)
    for i, j in itertools.product(range(ok.shape[0]), range(ok.shape[1])):
        try:
            with np.errstate(all="ignore"):
                stats.nbinom(n=r[i, j], p=1 - p[i, j]).rvs(random_state=1)
            raised = False
        except ValueError as exc:
            assert "Domain error" in str(exc)
            raised = True
        assert raised == (not ok[i, j]), (mu[i, j], x[3][j], x[4][j])
        if not band[i, j]:
            assert raised == (not closed[i, j]), (mu[i, j], x[3][j], x[4][j])


@pytest.mark.parametrize("planted", [False, True], ids=["valid", "planted"])
def test_no_gpu_case_in_the_rounding_band(planted):
    seen = set()
    for case in gpu.CASES:
        x = case.inputs(planted)
        if planted and any(p[0] == "roc" for p in case.plants):
            continue                                  # (refused for its row index before any sample is looked at)
        key = None if planted else (case.rows, case.G, case.N, case.roc, case.genes, case.columns, case.cells)
        if key is not None and key in seen:
            continue                                  # the valid input of an earlier case
        seen.add(key)
        args = (x["means"], x["roc"], x["scaling"], x["alpha"], x["beta"])
        assert not ref_numpy.domain_rounding_band(*args).any(), case.name
        assert not ref_numpy.domain_cancellation_band(*args).any(), case.name
        ok = ref_numpy.domain_ok(*args)
        np.testing.assert_array_equal(ok, ref_numpy.domain_ok_closed_form(*args), err_msg=case.name)
        mu = ref_numpy._device_sample_means(*args[:3])
        inside = mu[(mu > 0) & (mu < np.inf)]
        assert inside.size == 0 or (inside.min() >= 1e-100 and inside.max() <= 1e6), case.name
        if not planted:
            assert ok.all(), case.name                # the input every case starts from is valid
        elif ok.all():
            assert case.name.startswith("value-") or "-unused" in case.name, case.name      # only those plant valid values


def test_cases_cover_the_stated_places():
    names = [c.name for c in gpu.CASES]
    K = gpu.K
    for v in gpu.MEAN_VALUES:
        assert sum(c.plant == ("means", (1, 5), v) or (c.plant[0] == "means" and c.plant[2] != c.plant[2] and v != v)
                   for c in gpu.CASES if c.name.startswith("value-mean")) >= 2
    for v in gpu.SCALING_VALUES:
        assert sum(c.plant[0] == "scaling" and (c.plant[2] == v or (v != v and c.plant[2] != c.plant[2]))
                   for c in gpu.CASES if c.name.startswith("value-scaling")) >= 2
    for v in gpu.PARAM_VALUES:
        assert {c.params for c in gpu.CASES if c.plant == ("params", 6, v)} == {"host", "device"}
    # row_flags_kernel: 1, 2 and 5 steps of a thread over the genes; a second step of the grid over the rows
    T = K["flag_threads"]
    assert {-(-c.G // T) for c in gpu.CASES if c.name.startswith("rowflags-G")} == {1, 2, 5}
    assert any(c.plant[1][0] >= K["flag_rows"] for c in gpu.CASES if c.name.startswith("rowflags-rows"))
    # prep_kernel: N + 4 > G and G > N + 4, bad cells and genes beyond the first block
    prep = [c for c in gpu.CASES if c.name.startswith("prep-")]
    assert any(c.N + 4 > c.G for c in prep) and any(c.G > c.N + 4 for c in prep)
    assert any(c.plant[0] == "scaling" and c.plant[1] >= K["prep_threads"] and c.G > c.N + 4 for c in prep)
    assert any(c.plant[0] == "params" and c.plant[1] >= K["prep_threads"] and c.N + 4 > c.G for c in prep)
    # the per-sample pass: a block's second and third cell, a thread's second and third gene
    tail = [c for c in gpu.CASES if c.name.startswith("persample-")]
    grid, B = K["heavy_min_grid"], K["heavy_block"]
    assert all(c.G > 2 * B and c.N >= 3 * grid for c in tail) and any(c.G % B for c in tail)
    assert {min(c.plant[1][0] // grid, 2) for c in tail} == {0, 1, 2} and {min(c.plant[1][1] // B, 2) for c in tail} == {0, 1, 2}
    for c in tail:                                    # exactly one sample is refused
        x = c.inputs(True)
        ok = ref_numpy.domain_ok(x["means"], x["roc"], x["scaling"], x["alpha"], x["beta"])
        assert (~ok).sum() == 1 and not ok[c.plant[1]], c.name
    assert len(names) == len(set(names))
