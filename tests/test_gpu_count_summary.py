"""-m gpu: count_summary / sample_density_summary (prosstt_amd/summary.py, libprosstt_amd_stats.so) against exact host
references: every integer field equal, on ragged shapes, strided and unaligned views, values that carry the 128-bit sum of
squares, the sampler's own matrices, and the reference's fixture g9 through learn_data_summary."""
import numpy as np
import pandas as pd
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _host_reference(X):
    """Exact sums of an int matrix (numpy, no Python-int loop over entries): sumsq through x = h * 2^16 + l."""
    X = np.asarray(X, dtype=np.int64)
    h, lo = X >> 16, X & 0xFFFF
    a, b, c = (h * h).sum(axis=0), (h * lo).sum(axis=0), (lo * lo).sum(axis=0)     # each < 2^45 for N < 2^13
    sumsq = [(int(x) << 32) + (int(y) << 17) + int(z) for x, y, z in zip(a, b, c)]
    return dict(gene_sum=X.sum(axis=0), gene_sumsq=sumsq, gene_zeros=(X == 0).sum(axis=0),
                cell_total=X.sum(axis=1), cell_zeros=(X == 0).sum(axis=1))


def _assert_exact(s, ref):
    for f in ("gene_sum", "gene_zeros", "cell_total", "cell_zeros"):
        np.testing.assert_array_equal(getattr(s, f), ref[f], err_msg=f)
    assert list(s.gene_sumsq) == [int(v) for v in ref["gene_sumsq"]]


NS = [1, 2, 63, 64, 65, 1000, 4097]
GS = [1, 3, 4, 5, 1023, 1024, 1025, 5003]
PADS = [0, 1, 3, 64]
KINDS = ["zeros", "nb", "big"]
CASES = [(NS[i % 7], GS[(3 * i + i // 7) % 8], PADS[(i // 2) % 4], KINDS[i % 3], (i // 5) % 2) for i in range(40)]


@pytest.mark.parametrize("N,G,pad,kind,shift", CASES)
def test_fuzz_shapes_strides_and_values(N, G, pad, kind, shift):
    import torch
    from prosstt_amd.summary import count_summary
    rng = np.random.default_rng(N * 100003 + G * 7 + pad)
    shift = shift if pad > 0 else 0                   # a base that is not 16-byte aligned needs room in the row
    width = G + pad
    if kind == "zeros":
        W = np.zeros((N, width), dtype=np.int32)
    elif kind == "nb":
        W = rng.negative_binomial(0.5, 0.4, size=(N, width)).astype(np.int32)
    else:
        W = (2 ** 31 - 1 - rng.integers(0, 3, size=(N, width))).astype(np.int32)
        W[rng.random((N, width)) < 0.1] = 0
    D = torch.as_tensor(W).cuda()
    view = D[:, shift:shift + G]
    assert view.stride() == ((width, 1) if N > 1 else view.stride())
    s = count_summary(view)
    assert (s.n_cells, s.n_genes) == (N, G)
    _assert_exact(s, _host_reference(W[:, shift:shift + G]))
    np.testing.assert_allclose(s.gene_var, W[:, shift:shift + G].astype(np.float64).var(axis=0), rtol=1e-12)


def test_reference_fixture_through_learn_data_summary():
    import torch
    from prosstt_amd import sim_utils as sut
    from prosstt_amd.summary import count_summary
    g = load_golden("g9_helpers")
    X = torch.as_tensor(g["ld_X"]).to(torch.int32).cuda()
    s = count_summary(X)
    relm = pd.Series({b: g["ld_rel_%s" % b] for b in "ABC"})
    scale, la, lb, prop = sut.learn_data_summary(s.cell_stats(), s.gene_stats(), relm)
    np.testing.assert_allclose(scale, g["ld_scale"], rtol=1e-12)
    np.testing.assert_allclose(la, g["ld_alpha"], rtol=1e-12)
    np.testing.assert_allclose(lb, g["ld_beta"], rtol=1e-12)
    np.testing.assert_allclose(prop, g["ld_means"], rtol=1e-12)


@pytest.fixture(scope="module")
def c2():
    from prosstt_amd import workloads
    return workloads.build("C2")


def test_presented_counts_in_plan_order(c2):
    from prosstt_amd import simulation as sim
    from prosstt_amd.summary import count_summary
    pt, br, sc, _ = c2.plan()
    presented = sim.draw_counts(c2.tree, pt, br, sc, c2.alpha, c2.beta, seed=31, out="torch")
    host = sim.draw_counts(c2.tree, pt, br, sc, c2.alpha, c2.beta, seed=31, out="numpy32")
    assert not np.array_equal(presented.cell_of_row, np.arange(len(pt)))
    s = count_summary(presented)
    _assert_exact(s, _host_reference(host))
    np.testing.assert_allclose(s.gene_var, host.var(axis=0), rtol=1e-12)
    np.testing.assert_allclose(s.gene_means, host.mean(axis=0), rtol=1e-15)


@pytest.mark.parametrize("chunk", [None, 1, 777, 5000])
def test_sample_density_summary_equals_the_summary_of_sample_density(c2, chunk):
    from prosstt_amd import simulation as sim
    from prosstt_amd.summary import sample_density_summary
    n = 5000 if chunk != 1 else 300           # (one launch per cell: a shorter plan)
    np.random.seed(77)
    X, pt, br, sc = sim.sample_density(c2.tree, n, alpha=c2.alpha, beta=c2.beta, out="numpy32")
    np.random.seed(77)
    s, spt, sbr, ssc = sample_density_summary(c2.tree, n, alpha=c2.alpha, beta=c2.beta, chunk_cells=chunk)
    np.testing.assert_array_equal(spt, pt)
    np.testing.assert_array_equal(sbr, br)
    np.testing.assert_array_equal(ssc, sc)
    _assert_exact(s, _host_reference(X))


def test_full_c3_matrix():
    import torch
    from prosstt_amd import workloads, simulation as sim
    from prosstt_amd.summary import count_summary
    work = workloads.build("C3")
    pt, br, sc, _ = work.plan()
    presented = sim.draw_counts(work.tree, pt, br, sc, work.alpha, work.beta, seed=2024, out="torch")
    s = count_summary(presented)
    host = presented.to_host("numpy32")
    del presented
    torch.cuda.empty_cache()
    N, G = host.shape
    assert (N, G) == (50000, 20000) and host.max() < 2 ** 26
    gene_sum = np.zeros(G, dtype=np.int64)
    gene_zeros = np.zeros(G, dtype=np.int64)
    sumsq = np.zeros(G, dtype=object)
    for lo in range(0, N, 2000):
        blk = host[lo:lo + 2000].astype(np.int64)
        gene_sum += blk.sum(axis=0)
        gene_zeros += (blk == 0).sum(axis=0)
        sumsq += (blk * blk).sum(axis=0).astype(object)          # < 2000 * 2^52: exact in int64
    ref = dict(gene_sum=gene_sum, gene_sumsq=list(sumsq), gene_zeros=gene_zeros,
               cell_total=host.sum(axis=1, dtype=np.int64), cell_zeros=(host == 0).sum(axis=1))
    _assert_exact(s, ref)


def test_non_default_stream(c2):
    import torch
    from prosstt_amd import simulation as sim
    from prosstt_amd.summary import count_summary, sample_density_summary
    pt, br, sc, _ = c2.plan(3000)
    want = count_summary(sim.draw_counts(c2.tree, pt, br, sc, c2.alpha, c2.beta, seed=5, out="torch"))
    np.random.seed(9)
    want_d = sample_density_summary(c2.tree, 2000, alpha=c2.alpha, beta=c2.beta, chunk_cells=600)[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = count_summary(sim.draw_counts(c2.tree, pt, br, sc, c2.alpha, c2.beta, seed=5, out="torch"))
        np.random.seed(9)
        got_d = sample_density_summary(c2.tree, 2000, alpha=c2.alpha, beta=c2.beta, chunk_cells=600)[0]
    for a, b in ((got, want), (got_d, want_d)):
        for f in ("gene_sum", "gene_zeros", "cell_total", "cell_zeros"):
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
        assert list(a.gene_sumsq) == list(b.gene_sumsq)


def test_errors():
    import torch
    from prosstt_amd.summary import count_summary
    X = torch.ones((6, 10), dtype=torch.int32, device="cuda")
    bad = X.clone()
    bad[3, 7] = -1
    with pytest.raises(ValueError):
        count_summary(bad)
    assert count_summary(X).gene_sum.tolist() == [6] * 10          # nothing left behind by the refused call
    with pytest.raises(TypeError):
        count_summary(X.to(torch.int64))
    with pytest.raises(TypeError):
        count_summary(X.cpu().numpy())
    with pytest.raises(ValueError):
        count_summary(X.cpu())
    with pytest.raises(ValueError):
        count_summary(X[:, ::2])
    with pytest.raises(ValueError):
        count_summary(X[:0])
