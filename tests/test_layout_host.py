"""prosstt_amd.layout without a device: the argument checks that refuse before any device use; the fit of a and b; the
binary64 model (tests/layout_model.py) against its own definition: the schedule, the hash, the trustworthiness score, the start's scaling and a whole run."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytest.importorskip("scipy")

import graph_model  # noqa: E402
import layout_model  # noqa: E402
from prosstt_amd import device, graph, layout, neighbors  # noqa: E402


@pytest.fixture
def no_device(monkeypatch):
    """Any step towards the device fails the test: the loader of every library and torch's own switch."""
    def reached(*args, **kwargs):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(device, "need_device", reached)
    monkeypatch.setattr(graph, "_on_device", reached)


def _nb(n=20, k=3):
    rng = np.random.default_rng(1)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)
    return neighbors.Neighbors(idx, rng.random((n, k)).astype(np.float32))


def _conn(n=20):
    return graph.Connectivities(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64), None, None)


def test_umap_refusals_before_any_device_use(no_device):
    nb = _nb()
    with pytest.raises(ValueError, match="pair"):
        layout.umap(nb.indices)
    with pytest.raises(ValueError, match="indices must be int32"):
        layout.umap(neighbors.Neighbors(nb.indices.astype(np.int64), nb.sq_distances))
    with pytest.raises(ValueError, match="neighbours"):
        layout.umap(neighbors.Neighbors(nb.indices[:, :1], nb.sq_distances[:, :1]))
    with pytest.raises(ValueError, match="must be a 1-D"):
        layout.umap(_conn()._replace(indptr=np.zeros(21, np.int32)))
    for c in (1, 4, 0, 2.5, "2", None):
        with pytest.raises(ValueError, match="n_components"):
            layout.umap(nb, c)
    for n_epochs in (0, -1, 4097, 2.5, "many"):
        with pytest.raises(ValueError, match="n_epochs"):
            layout.umap(nb, n_epochs=n_epochs)
    for name in ("alpha", "a", "b"):
        for bad in (0, -1.0, float("inf"), float("nan"), "big"):
            kw = dict(a=1.0, b=1.0)
            kw[name] = bad
            with pytest.raises(ValueError, match=name + " must be"):
                layout.umap(nb, **kw)
    for gamma in (-1e-9, float("inf"), float("nan"), None):
        with pytest.raises(ValueError, match="gamma"):
            layout.umap(nb, gamma=gamma)
    for rate in (-1, 32, 2.5, None):
        with pytest.raises(ValueError, match="negative_sample_rate"):
            layout.umap(nb, negative_sample_rate=rate)
    for seed in (-1, 1 << 64, 0.5, None):
        with pytest.raises(ValueError, match="seed"):
            layout.umap(nb, seed=seed)
    for lanes in (1, 8, 32, 128, -4):
        with pytest.raises(ValueError, match="lanes_per_row"):
            layout.umap(nb, lanes_per_row=lanes)
    with pytest.raises(ValueError, match="out must be"):
        layout.umap(nb, out="scipy")
    with pytest.raises(ValueError, match="both a and b"):
        layout.umap(nb, a=1.0)
    with pytest.raises(ValueError, match="both a and b"):
        layout.umap(nb, b=1.0)
    for spread in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="spread"):
            layout.umap(nb, spread=spread)
    for min_dist in (-0.1, 3.0, float("nan")):
        with pytest.raises(ValueError, match="min_dist"):
            layout.umap(nb, min_dist=min_dist)
    with pytest.raises(ValueError, match="init must be"):
        layout.umap(nb, init="pca")
    with pytest.raises(ValueError, match=r"init must be \(20, 2\)"):
        layout.umap(nb, init=np.zeros((20, 3), np.float32))
    with pytest.raises(ValueError, match=r"init must be \(20, 3\)"):
        layout.umap(nb, 3, init=torch.zeros(19, 3))
    for bad in (float("nan"), float("inf"), -float("inf")):
        start = np.zeros((20, 2))
        start[7, 1] = bad
        with pytest.raises(ValueError, match="init must be finite"):
            layout.umap(nb, init=start)
        with pytest.raises(ValueError, match="init must be finite"):
            layout.umap(nb, init=torch.from_numpy(start))
    with pytest.raises(ValueError, match="array of numbers"):
        layout.umap(nb, init=np.full((20, 2), "x"))


def test_optimize_and_spectral_refusals_before_any_device_use(no_device):
    g, Y = _conn(), np.zeros((20, 2), np.float32)
    good = dict(n_epochs=10, a=1.0, b=1.0)
    with pytest.raises(ValueError, match="Connectivities"):
        layout.optimize(_nb(), Y, 0, 1, **good)
    with pytest.raises(ValueError, match="differ in length"):
        layout.optimize(g._replace(data=np.zeros(4, np.float64)), Y, 0, 1, **good)
    for bad in (np.zeros((20, 4), np.float32), np.zeros(20, np.float32), np.zeros((19, 2), np.float32), None):
        with pytest.raises(ValueError, match="Y must be"):
            layout.optimize(g, bad, 0, 1, **good)
    for begin, end in ((-1, 1), (2, 1), (0, 11), (11, 11)):
        with pytest.raises(ValueError, match="epoch_begin <= epoch_end"):
            layout.optimize(g, Y, begin, end, **good)
    with pytest.raises(ValueError, match="integer"):
        layout.optimize(g, Y, 0.5, 1, **good)
    with pytest.raises(ValueError, match="n_epochs"):
        layout.optimize(g, Y, 0, 1, n_epochs=4097, a=1.0, b=1.0)
    with pytest.raises(ValueError, match="negative_sample_rate"):
        layout.optimize(g, Y, 0, 1, negative_sample_rate=32, **good)
    with pytest.raises(ValueError, match="lanes_per_row"):
        layout.optimize(g, Y, 0, 1, lanes_per_row=8, **good)
    with pytest.raises(ValueError, match="Y must be finite"):
        layout.optimize(g, np.full((20, 2), np.nan, np.float32), 0, 1, **good)
    for c in (1, 4):
        with pytest.raises(ValueError, match="n_components"):
            layout.spectral_vectors(_nb(), c)
    with pytest.raises(ValueError, match="pair"):
        layout.spectral_vectors(None)
    with pytest.raises(ValueError, match="seed"):
        layout.spectral_vectors(_nb(), seed=-1)
    with pytest.raises(ValueError, match="out must be"):
        layout.spectral_vectors(_nb(), out="scipy")
    with pytest.raises(ValueError, match=r"n_components \+ 1 < cells"):
        layout.spectral_vectors(graph.Connectivities(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64),
                                                     None, None), 2)


def test_find_ab_params_gives_the_published_values():
    a, b = layout.find_ab_params(1.0, 0.5)
    assert abs(a - 0.5830300) <= 1e-6 and abs(b - 1.3341670) <= 1e-6
    assert abs(a - layout_model.A) <= 1e-6 and abs(b - layout_model.B) <= 1e-6
    a2, b2 = layout.find_ab_params(1.0, 0.1)
    assert a2 > a and b2 < b                                     # a tighter layout: a steeper curve at the origin


def test_model_schedule_samples_an_edge_floor_E_p_times():
    rng = np.random.default_rng(5)
    p = np.r_[rng.random(2000), 0.0, 1.0, 0.5, 1 / 3, 1 / 50, 1 / 500, np.nextafter(1 / 50, 0), np.nextafter(1.0, 0), 0.999]
    for E in (1, 50, 200, 500, 4096):
        times = sum(layout_model.active(p, n).astype(np.int64) for n in range(E))
        np.testing.assert_array_equal(times, np.floor(E * p).astype(np.int64))
        assert np.all(times[p < 1.0 / E] == 0)


def test_model_hash_is_in_range_and_uniform():
    # splitmix64's finaliser on its published first output: seed 0 -> 0xE220A8397B1DCDAF
    assert int(layout_model.mix(layout_model.GOLDEN)[0]) == 0xE220A8397B1DCDAF
    for N in (3, 65, 1000, (1 << 31) - 1):
        k = layout_model.negatives(12345, 3, np.arange(200000)[:, None], np.arange(5)[None, :], N)
        assert k.dtype == np.int64 and k.min() >= 0 and k.max() < N
    # 10^6 draws into N = 1000 cells: Pearson's statistic has 999 degrees of freedom, mean 999 and variance 2 x 999; six
    # standard deviations either way (a chi-square tail below 1e-8; a hash that dealt the cells in turn would fall BELOW)
    N, draws = 1000, 1000000
    for seed, n in ((0, 0), (12345, 3), ((1 << 64) - 1, 4095)):
        k = layout_model.negatives(seed, n, np.arange(draws // 5)[:, None], np.arange(5)[None, :], N).ravel()
        counts = np.bincount(k, minlength=N)
        chi2 = float(np.sum((counts - draws / N) ** 2) / (draws / N))
        dof = N - 1
        assert abs(chi2 - dof) <= 6 * np.sqrt(2 * dof), chi2
    # consecutive samples of an entry and the same sample of consecutive entries are no copies of each other
    k = layout_model.negatives(7, 0, np.arange(100000)[:, None], np.arange(5)[None, :], N)
    assert np.mean(k[:, 0] == k[:, 1]) < 5.0 / N and np.mean(k[1:, 0] == k[:-1, 0]) < 5.0 / N
    assert not np.array_equal(k, layout_model.negatives(7, 1, np.arange(100000)[:, None], np.arange(5)[None, :], N))


def test_model_trustworthiness_is_scikit_learns():
    manifold = pytest.importorskip("sklearn.manifold")
    rng = np.random.default_rng(3)
    X = rng.standard_normal((400, 6))
    for Y in (X[:, :2], rng.standard_normal((400, 2)), X @ rng.standard_normal((6, 3))):
        for k in (5, 14):
            assert abs(layout_model.trustworthiness(X, Y, k) - manifold.trustworthiness(X, Y, n_neighbors=k)) <= 1e-12
    assert layout_model.trustworthiness(X, X, 14) == 1.0


def test_model_run_lays_the_test_cloud_out():
    case = graph_model.case(1000, 14)
    start, out = layout_model.reference_run(1000, 14, 200, "spectral")
    assert out.dtype == np.float32 and np.all(np.isfinite(out)) and np.abs(out).max() <= 40
    before, after = (layout_model.trustworthiness(case["P"], Y, 14) for Y in (start, out))
    print("trustworthiness: start %.4f, after 200 epochs %.4f" % (before, after))
    assert before < 0.95 and after >= 0.98


def test_spectral_start_scaling_is_the_stated_formula():
    W = graph_model.case(300, 5)["W"]
    for c in (2, 3):
        values, vectors = layout_model.spectral_vectors(W, c)
        assert values.shape == (c,) and np.all(np.diff(values) < 0) and values[0] < 1 - 1e-6
        np.testing.assert_allclose(np.linalg.norm(vectors, axis=0), 1.0, rtol=0, atol=1e-14)
        for seed in (0, 9):
            got = layout._scale_start(vectors, seed)
            assert got.dtype == np.float32 and got.shape == (300, c)
            np.testing.assert_array_equal(got, layout_model.scale_start(vectors, seed))
            np.testing.assert_array_equal(got.min(axis=0), 0.0)
            np.testing.assert_array_equal(got.max(axis=0), 10.0)
            # before the rescaling: the vectors blown up to a largest entry of 10, and noise of 1e-4
            x = vectors * (10.0 / np.abs(vectors).max())
            span = x.max(axis=0) - x.min(axis=0)
            back = got.astype(np.float64) * span / 10.0 + x.min(axis=0)
            assert np.abs(back - x).max() <= 1e-3 and np.abs(back - x).max() > 1e-5
        assert not np.array_equal(layout._scale_start(vectors, 0), layout._scale_start(vectors, 9))
