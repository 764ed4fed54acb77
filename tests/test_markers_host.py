"""prosstt_amd.markers on the host: the statistics against the numpy model (tests/markers_model.py), the label encoding,
``GroupMoments.concat`` and its derived values, and every refusal that comes before a device is used (this file runs where
there is none)."""
import numpy as np
import pytest

pytest.importorskip("torch")

import markers_model as mm  # noqa: E402
from prosstt_amd import markers  # noqa: E402

N, G, K = 90, 40, 3


def _moments(seed=0, n_cells=N, k=K, names=None):
    """A GroupMoments built on the host from a random count matrix (binary64 entries: what the statistics take)."""
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.arange(n_cells) % k)
    s = rng.uniform(0.5, 2.0, size=n_cells)
    X = rng.poisson(rng.uniform(0.2, 8.0, size=G)[None, :] * s[:, None] * (1 + labels)[:, None])
    X[:, 5] = 0
    S1, S2, n = mm.sums64(mm.dense(X, s), labels)
    nz = np.stack([(X[labels == g] > 0).sum(0) for g in range(k)]).astype(np.int64)
    cs = np.stack([X[labels == g].sum(0) for g in range(k)]).astype(np.int64)
    groups = np.arange(k) if names is None else np.asarray(names)
    return markers.GroupMoments(groups, n, nz, cs, S1, S2, labels), X, s, labels


@pytest.mark.parametrize("method", markers.METHODS)
@pytest.mark.parametrize("reference", ["rest", 1])
def test_statistics_against_the_model(reference, method):
    gm, _, _, _ = _moments()
    got = markers.statistics(gm, reference, method)
    want = mm.statistics(gm.s1, gm.s2, gm.nonzero, gm.n, reference, method)
    for name, key in (("scores", "t"), ("df", "df"), ("pvals", "pvals"), ("pvals_adj", "pvals_adj"),
                      ("logfoldchanges", "logfoldchanges"), ("pts", "pts"), ("pts_rest", "pts_rest")):
        np.testing.assert_allclose(getattr(got, name), want[key], rtol=1e-12, atol=0, equal_nan=True, err_msg=name)
    assert got.scores[0, 5] == 0 and got.pvals[0, 5] == 1 and np.isnan(got.df[0, 5])


def test_a_named_reference_and_the_ranking():
    gm, _, _, _ = _moments(names=["A", "B", "C"])
    want = mm.statistics(gm.s1, gm.s2, gm.nonzero, gm.n, 2)
    res = markers.rank_genes_groups(gm, reference="C", n_genes=7)
    assert res.moments is gm and list(res.groups) == ["A", "B", "C"]
    names = mm.rank(want["t"], 7)
    assert res.names.dtype == np.int64 and np.array_equal(res.names, names)
    for field, key in (("scores", "t"), ("pvals", "pvals"), ("pvals_adj", "pvals_adj"), ("logfoldchanges", "logfoldchanges"),
                       ("pts", "pts"), ("pts_rest", "pts_rest")):
        np.testing.assert_allclose(getattr(res, field), np.take_along_axis(want[key], names, 1), rtol=1e-12, atol=0)
    full = markers.rank_genes_groups(gm)
    assert full.names.shape == (3, G)
    # ties go to the lower index: the reference against itself scores 0 everywhere
    assert np.array_equal(markers.rank_genes_groups(gm, reference="C").names[2], np.arange(G))


def test_benjamini_hochberg_against_the_model():
    rng = np.random.default_rng(3)
    p = np.stack([rng.uniform(size=G), rng.uniform(size=G) ** 5, np.r_[np.ones(G - 6), np.zeros(2), [0.25] * 4]])
    got = markers.benjamini_hochberg(p)
    for row, want in zip(got, p):
        np.testing.assert_allclose(row, mm.bh(want), rtol=1e-15, atol=0)


def test_label_encoding():
    groups, codes = markers.encode_labels(["B", "A", "C", "A"], 4)
    assert list(groups) == ["A", "B", "C"] and list(codes) == [1, 0, 2, 0] and codes.dtype == np.int64
    # integers are their own codes: negatives leave the cell out, a value nobody has is an empty category
    groups, codes = markers.encode_labels(np.array([3, -1, 0, 3, -7], dtype=np.int8), 5)
    assert list(groups) == [0, 1, 2, 3] and list(codes) == [3, -1, 0, 3, -1]
    import torch
    groups, codes = markers.encode_labels(torch.tensor([1, 0, 1]), 3)
    assert list(groups) == [0, 1] and list(codes) == [1, 0, 1]
    for bad, n in ((["A", "B"], 3), ([[0, 1]], 2), ([0.5, 1.0], 2), ([True, False], 2), ([-1, -1], 2),
                   (np.arange(1025), 1025)):
        with pytest.raises(ValueError):
            markers.encode_labels(bad, n)


def test_labels_follow_a_presented_matrix():
    """Row i of a presented matrix is cell cell_of_row[i]: the labels are permuted to row order, never the matrix."""
    class Presented:
        cell_of_row = np.array([2, 0, 3, 1])
    _, codes = markers.encode_labels(["a", "b", "c", "d"], 4)
    assert list(markers.codes_in_row_order(codes, Presented.cell_of_row)) == [2, 0, 3, 1]
    assert markers.codes_in_row_order(codes, None) is codes


def test_concat_and_the_derived_values():
    whole, X, s, labels = _moments(seed=4)
    cut = 37
    parts = []
    for lo, hi in ((0, cut), (cut, N)):
        S1, S2, n = mm.sums64(mm.dense(X[lo:hi], s[lo:hi]), labels[lo:hi], K)
        nz = np.stack([(X[lo:hi][labels[lo:hi] == g] > 0).sum(0) for g in range(K)])
        cs = np.stack([X[lo:hi][labels[lo:hi] == g].sum(0) for g in range(K)])
        parts.append(markers.GroupMoments(np.arange(K), n, nz, cs, S1, S2, labels[lo:hi]))
    both = markers.GroupMoments.concat(parts)
    assert np.array_equal(both.n, whole.n) and np.array_equal(both.codes, labels)
    assert np.array_equal(both.nonzero, whole.nonzero) and np.array_equal(both.count_sum, whole.count_sum)
    assert np.array_equal(both.s1, parts[0].s1 + parts[1].s1) and np.array_equal(both.s2, parts[0].s2 + parts[1].s2)
    np.testing.assert_allclose(both.s1, whole.s1, rtol=1e-13)
    A = mm.dense(X, s)
    for g in range(K):
        np.testing.assert_allclose(both.means()[g], A[labels == g].mean(0), rtol=1e-12)
        np.testing.assert_allclose(both.variances()[g], A[labels == g].var(0, ddof=1), rtol=1e-9, atol=1e-15)
        assert np.array_equal(both.fractions()[g], (X[labels == g] > 0).mean(0))
        np.testing.assert_allclose(both.pseudobulk(s)[g], X[labels == g].sum(0) / s[labels == g].sum(), rtol=1e-15)
    with pytest.raises(ValueError, match="at least one"):
        markers.GroupMoments.concat([])
    with pytest.raises(ValueError, match="different groups"):
        markers.GroupMoments.concat([whole, _moments(names=["A", "B", "C"])[0]])
    with pytest.raises(ValueError, match="size factor"):
        both.pseudobulk(s[:-1])
    with pytest.raises(ValueError):
        markers.GroupMoments(np.arange(K), whole.n[:-1], whole.nonzero, whole.count_sum, whole.s1, whole.s2, labels)
    with pytest.raises(ValueError):
        markers.GroupMoments(np.arange(K), whole.n, whole.nonzero[:, :-1], whole.count_sum, whole.s1, whole.s2, labels)


def test_statistics_refuses():
    gm, _, _, _ = _moments()
    with pytest.raises(ValueError, match="method"):
        markers.statistics(gm, method="wilcoxon")
    for reference in ("others", 3, -1, None, True):
        with pytest.raises(ValueError, match="reference"):
            markers.statistics(gm, reference)
    with pytest.raises(TypeError):
        markers.statistics((gm.s1, gm.s2))
    few = markers.GroupMoments(gm.groups, [1, 40, 49], gm.nonzero, gm.count_sum, gm.s1, gm.s2, gm.codes)
    with pytest.raises(ValueError, match="two cells"):
        markers.statistics(few)
    rest = markers.GroupMoments(gm.groups[:2], [89, 1], gm.nonzero[:2], gm.count_sum[:2], gm.s1[:2], gm.s2[:2], gm.codes)
    with pytest.raises(ValueError, match="two cells"):
        markers.statistics(rest)
    with pytest.raises(ValueError, match="two cells"):
        markers.rank_genes_groups(few)


def _cpu_counts():
    import torch
    return torch.zeros((N, G), dtype=torch.int32)


@pytest.mark.parametrize("kw,error,text", [
    (dict(counts=np.zeros((N, G), dtype=np.int32)), TypeError, "host arrays are refused"),
    (dict(counts="int64"), TypeError, "int32"),
    (dict(labels=np.zeros(N - 1, dtype=np.int64)), ValueError, "one label per cell"),
    (dict(labels=np.zeros((N, 1), dtype=np.int64)), ValueError, "one label per cell"),
    (dict(labels=np.full(N, -1)), ValueError, "no cell has a label"),
    (dict(size_factors=np.ones(N - 1)), ValueError, "one size factor per cell"),
    (dict(size_factors=np.zeros(N)), ValueError, "positive"),
    (dict(rows_per_block=-1), ValueError, "rows_per_block"),
    (dict(rows_per_block=1.5), ValueError, "rows_per_block"),
    (dict(out="scipy"), ValueError, "out must be"),
])
def test_group_moments_refuses(kw, error, text):
    import torch
    kw = dict(kw)
    counts = kw.pop("counts", _cpu_counts())
    if isinstance(counts, str):
        counts = torch.zeros((N, G), dtype=torch.int64)
    args = (counts, kw.pop("size_factors", np.ones(N)), kw.pop("labels", np.arange(N) % K))
    with pytest.raises(error, match=text):
        markers.group_moments(*args, **kw)
    if "rows_per_block" not in kw:                     # the ranking passes the same arguments on
        with pytest.raises(error, match=text):
            markers.rank_genes_groups(*args, **kw)


@pytest.mark.parametrize("kw,text", [
    (dict(n_genes=0), "n_genes"), (dict(n_genes=G + 1), "n_genes"), (dict(n_genes=2.5), "n_genes"), (dict(n_genes="all"), "n_genes"),
    (dict(method="logreg"), "method"), (dict(reference="others"), "reference"), (dict(reference=K), "reference"),
])
def test_rank_genes_groups_refuses(kw, text):
    with pytest.raises(ValueError, match=text):
        markers.rank_genes_groups(_cpu_counts(), np.ones(N), np.arange(N) % K, **kw)
    gm, _, _, _ = _moments()
    with pytest.raises(ValueError, match=text):
        markers.rank_genes_groups(gm, **kw)


def test_moments_come_without_further_arguments():
    gm, _, s, labels = _moments()
    with pytest.raises(ValueError, match="without"):
        markers.rank_genes_groups(gm, s, labels)


def test_accepted_calls_get_as_far_as_the_device():
    """With good arguments the next thing asked for is a device tensor: there is no CPU fallback."""
    with pytest.raises(ValueError, match="device tensor"):
        markers.group_moments(_cpu_counts(), np.ones(N), np.arange(N) % K)
    with pytest.raises(ValueError, match="device tensor"):
        markers.rank_genes_groups(_cpu_counts(), np.ones(N), np.array(["a", "b", "c"])[np.arange(N) % K], n_genes=G, reference="b")
