"""prosstt_amd.ranks on the host: the Wilcoxon statistics against the numpy model (tests/ranks_model.py) on hand-built
``RankSums``, and every refusal that comes before a device is used (this file runs where there is none)."""
import numpy as np
import pytest

pytest.importorskip("torch")

import markers_model as mm  # noqa: E402
import ranks_model as rm  # noqa: E402
from prosstt_amd import markers, ranks  # noqa: E402

N, G, K = 90, 40, 3


def _sums(reference="rest", names=None, seed=0):
    """(RankSums, GroupMoments) built on the host from a random count matrix: the model's integers on float32 entries."""
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.arange(N) % K)
    labels[:5] = -1
    s = rng.choice([0.5, 1.0, 2.0], size=N)
    X = rng.poisson(rng.uniform(0.2, 4.0, size=G)[None, :] * s[:, None] * (1 + np.maximum(labels, 0))[:, None])
    X[:, 5] = 0
    A = mm.dense(X, s).astype(np.float32)
    groups = np.arange(K) if names is None else np.asarray(names)
    ref = None if reference == "rest" else list(groups).index(reference)
    Q, T, n = rm.rank_sums(A, labels, K, reference=ref)
    S1, S2, n2 = mm.sums64(A[labels >= 0], labels[labels >= 0], K)
    assert np.array_equal(n, n2)
    nz = np.stack([(X[labels == g] > 0).sum(0) for g in range(K)]).astype(np.int64)
    cs = np.stack([X[labels == g].sum(0) for g in range(K)]).astype(np.int64)
    return ranks.RankSums(groups, n, Q, T, reference, labels), markers.GroupMoments(groups, n, nz, cs, S1, S2, labels)


@pytest.mark.parametrize("reference,tie_correct", [("rest", False), ("rest", True), (1, False)])
def test_wilcoxon_against_the_model(reference, tie_correct):
    rs, gm = _sums(reference)
    got = ranks.wilcoxon(rs, gm, tie_correct=tie_correct)
    want = rm.wilcoxon(rs.q, rs.ties, rs.n, reference, tie_correct)
    for name, key in (("scores", "z"), ("pvals", "pvals"), ("pvals_adj", "pvals_adj")):
        np.testing.assert_allclose(getattr(got, name), want[key], rtol=1e-12, atol=0, err_msg=name)
    assert np.isnan(got.df).all() and list(got.groups) == list(rs.groups)
    assert got.scores[0, 5] == 0 and got.pvals[0, 5] == 1                 # the all-zero gene: every rank sum at its mean
    t = markers.statistics(gm, reference)
    for name in ("logfoldchanges", "pts", "pts_rest"):
        assert np.array_equal(getattr(got, name), getattr(t, name), equal_nan=True), name
    bare = ranks.wilcoxon(rs, tie_correct=tie_correct)
    assert np.array_equal(bare.scores, got.scores) and np.array_equal(bare.pvals_adj, got.pvals_adj)
    for name in ("logfoldchanges", "pts", "pts_rest", "df"):
        assert np.isnan(getattr(bare, name)).all() and getattr(bare, name).shape == (K, G)


def test_a_flat_gene_under_the_tie_correction():
    """One value in every cell: T = n^3 - n, the corrected variance is 0; the score is 0 and p is 1."""
    n = np.array([4, 6])
    total = 10
    Q = (n * total)[:, None] * np.ones((2, 3), dtype=np.int64)
    T = np.full(3, total ** 3 - total, dtype=np.int64)
    st = ranks.wilcoxon(ranks.RankSums(np.arange(2), n, Q, T, "rest", np.zeros(10, dtype=np.int64)), tie_correct=True)
    assert not st.scores.any() and np.all(st.pvals == 1) and np.all(st.pvals_adj == 1)


def test_a_named_reference():
    rs, gm = _sums("B", names=["A", "B", "C"])
    got = ranks.wilcoxon(rs, gm)
    want = rm.wilcoxon(rs.q, rs.ties, rs.n, 1)
    np.testing.assert_allclose(got.scores, want["z"], rtol=1e-12, atol=0)
    assert not got.scores[1].any()                                          # the reference against itself


def test_wilcoxon_refuses():
    rs, gm = _sums()
    with pytest.raises(TypeError):
        ranks.wilcoxon((rs.q, rs.ties))
    with pytest.raises(TypeError):
        ranks.wilcoxon(rs, (gm.s1, gm.s2))
    against, _ = _sums(1)
    with pytest.raises(ValueError, match="tie_correct"):
        ranks.wilcoxon(against, tie_correct=True)
    with pytest.raises(ValueError, match="reference"):
        ranks.wilcoxon(rs._replace(reference="others"))
    with pytest.raises(ValueError, match="two cells"):
        ranks.wilcoxon(rs._replace(n=np.array([1, 40, 44])))
    with pytest.raises(ValueError, match="two cells"):
        ranks.wilcoxon(ranks.RankSums(rs.groups[:2], np.array([84, 1]), rs.q[:2], rs.ties, "rest", rs.codes))
    with pytest.raises(ValueError, match="other groups"):
        ranks.wilcoxon(rs, _sums(names=["A", "B", "C"])[1])
    with pytest.raises(ValueError):
        ranks.wilcoxon(rs._replace(ties=rs.ties[:-1]))


def _cpu_counts():
    import torch
    return torch.zeros((N, G), dtype=torch.int32)


@pytest.mark.parametrize("kw,error,text", [
    (dict(counts=np.zeros((N, G), dtype=np.int32)), TypeError, "host arrays are refused"),
    (dict(counts="int64"), TypeError, "int32"),
    (dict(labels=np.zeros(N - 1, dtype=np.int64)), ValueError, "one label per cell"),
    (dict(labels=np.zeros((N, 1), dtype=np.int64)), ValueError, "one label per cell"),
    (dict(labels=np.full(N, -1)), ValueError, "no cell has a label"),
    (dict(labels=np.arange(1025) % 1025, cells=1025), ValueError, "at most 1024 groups"),
    (dict(size_factors=np.ones(N - 1)), ValueError, "one size factor per cell"),
    (dict(size_factors=np.zeros(N)), ValueError, "positive"),
    (dict(reference="others"), ValueError, "reference"),
    (dict(reference=K), ValueError, "reference"),
    (dict(genes_per_pass=-1), ValueError, "genes_per_pass"),
    (dict(genes_per_pass=1.5), ValueError, "genes_per_pass"),
    (dict(genes_per_pass="all"), ValueError, "genes_per_pass"),
    (dict(out="scipy"), ValueError, "out must be"),
])
def test_rank_sums_refuses(kw, error, text):
    import torch
    kw = dict(kw)
    cells = kw.pop("cells", N)
    counts = kw.pop("counts", torch.zeros((cells, G), dtype=torch.int32))
    if isinstance(counts, str):
        counts = torch.zeros((N, G), dtype=torch.int64)
    args = (counts, kw.pop("size_factors", np.ones(cells)), kw.pop("labels", np.arange(cells) % K))
    with pytest.raises(error, match=text):
        ranks.rank_sums(*args, **kw)
    if "genes_per_pass" not in kw:                     # the ranking passes the same arguments on
        with pytest.raises(error, match=text):
            markers.rank_genes_groups(*args, method="wilcoxon", **kw)


def test_accepted_calls_get_as_far_as_the_device():
    """With good arguments the next thing asked for is a device tensor: there is no CPU fallback."""
    with pytest.raises(ValueError, match="device tensor"):
        ranks.rank_sums(_cpu_counts(), np.ones(N), np.arange(N) % K, reference=1, genes_per_pass=7)
    for tie_correct in (False, True):
        with pytest.raises(ValueError, match="device tensor"):
            markers.rank_genes_groups(_cpu_counts(), np.ones(N), np.arange(N) % K, method="wilcoxon", tie_correct=tie_correct)


def test_the_methods_and_what_a_group_moments_cannot_do():
    assert markers.METHODS == ("t-test", "t-test_overestim_var") and markers.RANK_METHODS == ("wilcoxon",)
    assert ranks.SORT_TILE == 1024
    _, gm = _sums()
    for call in (lambda: markers.statistics(gm, method="wilcoxon"), lambda: markers.rank_genes_groups(gm, method="wilcoxon")):
        with pytest.raises(ValueError, match="method") as err:
            call()
        assert "needs the matrix" in str(err.value)


@pytest.mark.parametrize("kw,text", [
    (dict(method="t-test", tie_correct=True), "tie_correct"),
    (dict(method="t-test_overestim_var", tie_correct=True), "tie_correct"),
    (dict(method="wilcoxon", tie_correct=True, reference=1), "tie_correct"),
    (dict(method="wilcoxon", tie_correct="yes"), "tie_correct"),
    (dict(method="wilcoxon", n_genes=0), "n_genes"),
    (dict(method="wilcoxon", reference="others"), "reference"),
    (dict(method="logreg"), "method"),
])
def test_rank_genes_groups_refuses_before_the_device(kw, text):
    with pytest.raises(ValueError, match=text):
        markers.rank_genes_groups(_cpu_counts(), np.ones(N), np.arange(N) % K, **kw)
