"""prosstt_amd.tsne's argument checks: everything that can be refused without a device is refused before one is used (this
file runs where there is none: a call that got past its checks would raise RuntimeError or NativeError, not ValueError)."""
import numpy as np
import pytest

pytest.importorskip("torch")

from prosstt_amd import tsne  # noqa: E402
from prosstt_amd.neighbors import Neighbors  # noqa: E402

N, K = 40, 12


def _neighbors(n=N, k=K):
    idx = (np.arange(n)[:, None] + 1 + np.arange(k)[None, :]) % n
    return Neighbors(idx.astype(np.int32), np.linspace(0.1, 2.0, n * k, dtype=np.float32).reshape(n, k))


def _affinities(n=N):
    indptr = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    indices = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 2) % n], axis=1).astype(np.int32).ravel()
    return tsne.Affinities(indptr, indices, np.full(2 * n, 0.5 / n), np.ones(n))


Y = np.zeros((N, 2), dtype=np.float32)


@pytest.mark.parametrize("kw,text", [
    (dict(out="numpy"), "out must be"),
    (dict(perplexity=1.0), "perplexity"), (dict(perplexity=float(K)), "perplexity"), (dict(perplexity=float("nan")), "perplexity"),
    (dict(perplexity="30"), "perplexity"),
])
def test_affinities_refuses(kw, text):
    with pytest.raises(ValueError, match=text):
        tsne.affinities(_neighbors(), **dict(dict(perplexity=4.0), **kw))


@pytest.mark.parametrize("nb,text", [
    (3, "Neighbors"),
    (Neighbors(_neighbors().indices.astype(np.int64), _neighbors().sq_distances), "indices must be int32"),
    (Neighbors(_neighbors().indices, _neighbors().sq_distances.astype(np.float64)), "sq_distances must be float32"),
    (Neighbors(_neighbors().indices[:, :5], _neighbors().sq_distances), "differ in shape"),
    (Neighbors(_neighbors().indices[0], _neighbors().sq_distances[0]), "dimensions"),
    (_neighbors(2, 1), "3 <= cells"), (_neighbors(40, 1), "neighbours"), (_neighbors(10, 10), "neighbours"),
])
def test_affinities_refuses_neighbours(nb, text):
    with pytest.raises(ValueError, match=text):
        tsne.affinities(nb, 1.5)
    with pytest.raises(ValueError, match=text):
        tsne.tsne(nb, perplexity=1.5, init="random") if isinstance(nb, tuple) else tsne.affinities(nb, 1.5)


def _bad_affinities():
    a = _affinities()
    return [(3, "Affinities"), (_neighbors(), "Affinities"),
            (a._replace(indptr=a.indptr.astype(np.int32)), "indptr"), (a._replace(indices=a.indices.astype(np.int64)), "indices"),
            (a._replace(data=a.data.astype(np.float32)), "data"), (a._replace(data=a.data[:-1]), "differ in length"),
            (a._replace(indptr=a.indptr[:3]), "3 <= cells"), (a._replace(indices=a.indices.reshape(-1, 2)), "indices")]


@pytest.mark.parametrize("aff,text", _bad_affinities())
def test_gradient_and_optimize_refuse_affinities(aff, text):
    with pytest.raises(ValueError, match=text):
        tsne.gradient(aff, Y)
    with pytest.raises(ValueError, match=text):
        tsne.optimize(aff, Y, 0, 1, learning_rate=50.0)


@pytest.mark.parametrize("kw,text", [
    (dict(Y=np.zeros((N, 4), np.float32)), "Y must be"), (dict(Y=np.zeros((N + 1, 2), np.float32)), "Y must be"),
    (dict(Y=np.zeros(N, np.float32)), "Y must be"), (dict(Y=np.full((N, 2), np.nan, np.float32)), "finite"),
    (dict(Y=np.zeros((N, 2), dtype="U1")), "numbers"),
    (dict(slabs=-1), "slabs"), (dict(slabs=1025), "slabs"), (dict(slabs=1.5), "slabs"),
    (dict(exaggeration=0.0), "exaggeration"), (dict(exaggeration=float("inf")), "exaggeration"), (dict(exaggeration=None), "exaggeration"),
])
def test_gradient_refuses(kw, text):
    kw = dict(kw)
    with pytest.raises(ValueError, match=text):
        tsne.gradient(_affinities(), kw.pop("Y", Y), **kw)


@pytest.mark.parametrize("kw,text", [
    (dict(Y=np.zeros((N, 1), np.float32)), "Y must be"), (dict(Y=np.full((N, 3), np.inf, np.float32)), "finite"),
    (dict(it_begin=-1), "it_begin"), (dict(it_begin=2, it_end=1), "it_end"), (dict(it_end=1.5), "it_end"),
    (dict(it_end=(1 << 30) + 1), "it_end"),
    (dict(update=np.zeros((N, 3), np.float32)), "update must be"), (dict(gains=np.zeros((N + 1, 2), np.float32)), "gains must be"),
    (dict(gains=np.full((N, 2), np.nan, np.float32)), "gains must be finite"),
    (dict(exploration=-1), "exploration"), (dict(exploration=2.5), "exploration"),
    (dict(early_exaggeration=0.0), "early_exaggeration"), (dict(early_exaggeration=float("nan")), "early_exaggeration"),
    (dict(learning_rate=0.0), "learning_rate"), (dict(learning_rate="auto"), "learning_rate"), (dict(learning_rate=float("inf")), "learning_rate"),
    (dict(slabs=-1), "slabs"), (dict(slabs=2000), "slabs"),
])
def test_optimize_refuses(kw, text):
    kw = dict(dict(it_begin=0, it_end=1, learning_rate=50.0), **kw)
    with pytest.raises(ValueError, match=text):
        tsne.optimize(_affinities(), kw.pop("Y", Y), kw.pop("it_begin"), kw.pop("it_end"), **kw)
    with pytest.raises(TypeError):
        tsne.optimize(_affinities(), Y, 0, 1)                     # the learning rate has no default here


PANEL = np.random.default_rng(0).standard_normal((N, 5)).astype(np.float32)


@pytest.mark.parametrize("kw,text", [
    (dict(out="scipy"), "out must be"), (dict(n_components=1), "n_components"), (dict(n_components=4), "n_components"),
    (dict(n_components=2.5), "n_components"),
    (dict(perplexity=1.0), "perplexity"), (dict(perplexity=None), "perplexity"), (dict(perplexity=40.0), "perplexity"),
    (dict(early_exaggeration=0.0), "early_exaggeration"), (dict(learning_rate=0.0), "learning_rate"),
    (dict(learning_rate="fast"), "learning_rate"), (dict(learning_rate=float("nan")), "learning_rate"),
    (dict(n_iter=-1), "n_iter"), (dict(n_iter=10.5), "n_iter"), (dict(exploration=-1), "exploration"),
    (dict(seed=-1), "seed"), (dict(seed=0.5), "seed"), (dict(slabs=-1), "slabs"), (dict(slabs=1025), "slabs"),
    (dict(init="spectral"), "init must be"), (dict(init=np.zeros((N, 3), np.float32)), "init must be"),
    (dict(init=np.full((N, 2), np.inf, np.float32)), "init must be finite"),
    (dict(X=PANEL[:, :1], n_components=2), "init='pca' needs"), (dict(X=PANEL[:2]), "3 <= cells"),
    (dict(X=PANEL[0]), "panel"), (dict(X=PANEL[:3], perplexity=2.5), "perplexity"),
    (dict(X=_neighbors()), "init='pca' needs"), (dict(X=_affinities()), "init='pca' needs"),
    (dict(X=_neighbors(), init="random", perplexity=12.0), "perplexity"),
    (dict(X=_affinities()._replace(data=np.zeros(3)), init="random"), "differ in length"),
    (dict(X=_affinities(), init=np.zeros((N + 1, 2), np.float32)), "init must be"),
])
def test_tsne_refuses(kw, text):
    kw = dict(dict(perplexity=4.0), **kw)
    with pytest.raises(ValueError, match=text):
        tsne.tsne(kw.pop("X", PANEL), **kw)


def test_accepted_calls_get_as_far_as_the_device():
    """With good arguments the next thing asked for is the device: there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the calls would run")
    for call in (lambda: tsne.affinities(_neighbors(), 4.0), lambda: tsne.gradient(_affinities(), Y),
                 lambda: tsne.optimize(_affinities(), Y, 0, 1, learning_rate=50.0), lambda: tsne.tsne(PANEL, perplexity=4.0),
                 lambda: tsne.tsne(_affinities(), init="random")):
        with pytest.raises(RuntimeError):
            call()
