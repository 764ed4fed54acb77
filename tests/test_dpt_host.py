"""prosstt_amd.dpt's argument checks and its distance weights: everything that can be refused without a device is refused
before one is used (this file runs where there is none: a call that got past its checks would raise RuntimeError or
NativeError, not ValueError)."""
import numpy as np
import pytest

pytest.importorskip("torch")

from prosstt_amd import dpt  # noqa: E402
from prosstt_amd.graph import DiffusionMap  # noqa: E402

N, C = 40, 6


def _map(n=N, c=C):
    rng = np.random.default_rng(1)
    return DiffusionMap(np.linspace(1.0, 0.5, c), rng.standard_normal((n, c)), c, np.zeros(c), None)


def _ranks(batch=2, n=N):
    return np.tile(np.arange(n, dtype=np.int32), (batch, 1))


def _bad_maps():
    m = _map()
    return [(3, "DiffusionMap"), ((m.eigenvalues, m.eigenvectors), "DiffusionMap"),
            (m._replace(eigenvalues=m.eigenvalues.astype(np.float32)), "eigenvalues"),
            (m._replace(eigenvectors=m.eigenvectors.astype(np.float32)), "eigenvectors"),
            (m._replace(eigenvectors=m.eigenvectors[:, 0]), "eigenvectors"), (m._replace(eigenvalues=m.eigenvalues[None]), "eigenvalues"),
            (m._replace(eigenvalues=list(m.eigenvalues)), "eigenvalues"),
            (m._replace(eigenvalues=m.eigenvalues[:-1]), "5 eigenvalues for 6"), (_map(2, 1), "3 <= cells"),
            (_map(4, 4), "n_comps"), (m._replace(eigenvalues=np.zeros(0), eigenvectors=np.zeros((N, 0))), "n_comps")]


@pytest.mark.parametrize("dm,text", _bad_maps())
def test_a_bad_map_is_refused(dm, text):
    with pytest.raises(ValueError, match=text):
        dpt.dpt(dm, 0)
    with pytest.raises(ValueError, match=text):
        dpt.distances(dm, [0])


@pytest.mark.parametrize("kw,text", [
    (dict(root=-1), "root"), (dict(root=N), "root"), (dict(root=1.5), "root"), (dict(root=None), "root"), (dict(root=True), "root"),
    (dict(n_dcs=0), "n_dcs"), (dict(n_dcs=C + 1), "n_dcs"), (dict(n_dcs=2.5), "n_dcs"), (dict(n_dcs="all"), "n_dcs"),
    (dict(n_branchings=2), "n_branchings"), (dict(n_branchings=-1), "n_branchings"), (dict(n_branchings=0.5), "n_branchings"),
    (dict(n_branchings=None), "n_branchings"),
    (dict(min_group_size=1), "min_group_size"), (dict(min_group_size=N // 2 + 1), "min_group_size"),
    (dict(min_group_size=2.5), "min_group_size"), (dict(min_group_size=None), "min_group_size"),
    (dict(n_branchings=1, min_group_size=21), "min_group_size"),
    (dict(slabs=-1), "slabs"), (dict(slabs=1025), "slabs"), (dict(slabs=1.5), "slabs"),
    (dict(out="scipy"), "out must be"), (dict(out=None), "out must be"),
])
def test_dpt_refuses(kw, text):
    kw = dict(kw)
    with pytest.raises(ValueError, match=text):
        dpt.dpt(_map(), kw.pop("root", 0), **kw)


@pytest.mark.parametrize("kw,text", [
    (dict(sources=[]), "sources"), (dict(sources=[0, N]), "outside"), (dict(sources=[-1]), "outside"), (dict(sources=3), "sources"),
    (dict(sources=[0.5]), "sources"), (dict(sources=[[0, 1]]), "sources"), (dict(sources=np.zeros(65536, dtype=np.int64)), "sources"),
    (dict(n_dcs=0), "n_dcs"), (dict(n_dcs=C + 1), "n_dcs"), (dict(out="scipy"), "out must be"),
])
def test_distances_refuses(kw, text):
    kw = dict(kw)
    with pytest.raises(ValueError, match=text):
        dpt.distances(_map(), kw.pop("sources", [0, 3]), **kw)


@pytest.mark.parametrize("ru,rv,kw,text", [
    (_ranks().astype(np.int64), _ranks(), {}, "ru must be int32"), (_ranks(), _ranks().astype(np.float32), {}, "rv must be int32"),
    (_ranks()[0], _ranks()[0], {}, "dimensions"), (_ranks(), _ranks()[:, :-1], {}, "differ in shape"),
    (_ranks(2, 2), _ranks(2, 2), {}, "3 <= cells"), (_ranks(0), _ranks(0), {}, "batch"), (_ranks(1025, 3), _ranks(1025, 3), {}, "batch"),
    (_ranks() - 1, _ranks(), {}, "rank of ru"), (_ranks(), _ranks() + 1, {}, "rank of rv"),
    (_ranks(), _ranks(), dict(slabs=-1), "slabs"), (_ranks(), _ranks(), dict(slabs=1025), "slabs"),
    (_ranks(), _ranks(), dict(slabs=0.5), "slabs"),
])
def test_concordance_refuses(ru, rv, kw, text):
    with pytest.raises(ValueError, match=text):
        dpt.concordance(ru, rv, **kw)


def test_concordance_refuses_mixed_places():
    import torch
    with pytest.raises(ValueError, match="rv must be int32"):
        dpt.concordance(torch.from_numpy(_ranks()), torch.from_numpy(_ranks()).long())


def test_the_weights():
    below = np.nextafter(0.9994, 0.0)
    lam = np.array([1.0, 0.9994, below, 0.5, 0.0, -0.25])
    with np.errstate(all="raise"):                    # the division is not evaluated at lambda = 1
        w = dpt.weights(lam, 6)
    assert w.dtype == np.float64
    assert w[0] == 1.0 and w[1] == 1.0
    assert w[2] == below / (1.0 - below) and w[2] > 1665
    assert w[3] == 1.0 and w[4] == 0.0 and w[5] == -0.25 / 1.25
    assert np.array_equal(dpt.weights(lam, 3), w[:3])
    import dpt_model
    assert np.array_equal(dpt_model.weights(lam, 6), w)


def test_accepted_calls_get_as_far_as_the_device():
    """With good arguments the next thing asked for is the device: there is no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is visible: the calls would run")
    for call in (lambda: dpt.dpt(_map(), 0), lambda: dpt.dpt(_map(), N - 1, C, n_branchings=1, min_group_size=20, slabs=1024, out="torch"),
                 lambda: dpt.distances(_map(), [0, N - 1], 1), lambda: dpt.concordance(_ranks(), _ranks(), 3)):
        with pytest.raises(RuntimeError):
            call()
