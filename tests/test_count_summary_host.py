"""CountSummary (prosstt_amd/summary.py) from integer parts: exact means and variances, concatenation, the DataFrame
layouts of sim_utils.learn_data_summary, and learn_data_summary fed by it on the reference's fixture g9.  No GPU."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden


def _parts(X):
    """Integer parts of an integer matrix, on the host (Python ints for the sums of squares)."""
    X = np.asarray(X)
    Xi = X.astype(object)
    return dict(gene_sum=X.sum(axis=0).astype(np.int64), gene_sumsq=list((Xi * Xi).sum(axis=0)),
                gene_zeros=(X == 0).sum(axis=0), cell_total=X.sum(axis=1).astype(np.int64), cell_zeros=(X == 0).sum(axis=1))


def _ulps(got, exact):
    want = float(exact)
    return abs(Fraction(got) - exact) / Fraction(np.spacing(abs(want)) if want else np.finfo(float).tiny)


def test_means_and_variances_are_correctly_rounded_from_exact_integers():
    from prosstt_amd.summary import CountSummary
    rng = np.random.default_rng(3)
    X = rng.integers(0, 2 ** 31 - 1, size=(37, 9), dtype=np.int64)
    X[:, 0] = 2 ** 31 - 1              # sums of squares far above 2^64
    X[:, 1] = 0
    X[::3, 2] = 0
    X[:, 3] = rng.negative_binomial(2, 0.3, size=37)
    s = CountSummary.from_parts(**_parts(X))
    assert max(s.gene_sumsq) > 2 ** 64
    N = X.shape[0]
    for g in range(X.shape[1]):
        col = [int(v) for v in X[:, g]]
        mean = Fraction(sum(col), N)
        var = Fraction(sum(v * v for v in col), N) - mean * mean
        assert _ulps(s.gene_means[g], mean) <= 1
        assert _ulps(s.gene_var[g], var) <= 2
    assert s.gene_var[1] == 0.0 and s.gene_means[1] == 0.0
    np.testing.assert_allclose(s.gene_var, X.astype(np.float64).var(axis=0), rtol=1e-12)
    np.testing.assert_array_equal(s.gene_zeros, (X == 0).sum(axis=0))


@pytest.mark.parametrize("pieces", [1, 2, 3, 5])
def test_concat_of_row_chunks_equals_the_whole(pieces):
    from prosstt_amd.summary import CountSummary
    rng = np.random.default_rng(pieces)
    X = rng.negative_binomial(1, 0.2, size=(23, 7))
    X[0, :] = 2 ** 31 - 1
    cuts = np.sort(rng.choice(np.arange(1, 23), size=pieces - 1, replace=False)) if pieces > 1 else []
    parts = [CountSummary.from_parts(**_parts(chunk)) for chunk in np.split(X, cuts)]
    got, want = CountSummary.concat(parts), CountSummary.from_parts(**_parts(X))
    assert (got.n_cells, got.n_genes) == (23, 7)
    for f in ("gene_sum", "gene_zeros", "cell_total", "cell_zeros"):
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f))
    assert list(got.gene_sumsq) == list(want.gene_sumsq)
    np.testing.assert_array_equal(got.gene_var, want.gene_var)
    np.testing.assert_array_equal(got.gene_means, want.gene_means)


def test_dataframe_layouts():
    from prosstt_amd.summary import CountSummary
    X = np.array([[0, 1, 2], [3, 0, 0]])
    s = CountSummary.from_parts(**_parts(X))
    cs, gs = s.cell_stats(), s.gene_stats()
    assert list(cs.index) == ["total", "zeros"] and list(cs.columns) == [0, 1]
    assert list(gs.index) == ["means", "var", "zeros"] and list(gs.columns) == [0, 1, 2]
    np.testing.assert_array_equal(cs.loc["total"], [3, 3])
    np.testing.assert_array_equal(cs.loc["zeros"], [1, 2])
    np.testing.assert_array_equal(gs.loc["means"], [1.5, 0.5, 1.0])
    np.testing.assert_array_equal(gs.loc["var"], X.var(axis=0))
    np.testing.assert_array_equal(gs.loc["zeros"], [1, 1, 1])
    # the layouts of the reference's own construction (tests/golden/make_golden.py, learn_data_summary's inputs)
    ref_cs = pd.DataFrame({"total": X.sum(axis=1), "zeros": (X == 0).sum(axis=1)}).T
    ref_gs = pd.DataFrame({"means": X.mean(axis=0), "var": X.var(axis=0), "zeros": (X == 0).sum(axis=0)}).T
    assert list(ref_cs.index) == list(cs.index) and list(ref_cs.columns) == list(cs.columns)
    assert list(ref_gs.index) == list(gs.index) and list(ref_gs.columns) == list(gs.columns)


def test_learn_data_summary_on_the_reference_fixture():
    from prosstt_amd import sim_utils as sut
    from prosstt_amd.summary import CountSummary
    g = load_golden("g9_helpers")
    X = g["ld_X"]
    assert np.array_equal(X, np.round(X))
    s = CountSummary.from_parts(**_parts(X.astype(np.int64)))
    relm = pd.Series({b: g["ld_rel_%s" % b] for b in "ABC"})
    scale, la, lb, prop = sut.learn_data_summary(s.cell_stats(), s.gene_stats(), relm)
    np.testing.assert_allclose(scale, g["ld_scale"], rtol=1e-12)
    np.testing.assert_allclose(la, g["ld_alpha"], rtol=1e-12)
    np.testing.assert_allclose(lb, g["ld_beta"], rtol=1e-12)
    np.testing.assert_allclose(prop, g["ld_means"], rtol=1e-12)


def test_host_arrays_are_refused():
    pytest.importorskip("torch")
    from prosstt_amd.summary import count_summary
    with pytest.raises(TypeError):
        count_summary(np.zeros((3, 4), dtype=np.int32))
