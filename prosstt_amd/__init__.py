"""
prosstt_amd -- the PROSSTT simulation hot path on AMD MI355X (gfx950).

Drop-in for the reference package's modules:

    from prosstt_amd import tree, simulation as sim, sim_utils as sut, count_model as cm

Count-matrix summaries on the device (means, variances, zeros, library sizes; no host copy of the matrix):

    from prosstt_amd import summary

Principal components of log1p(X / s) on the device (the example notebooks' route to neighbours and UMAP):

    from prosstt_amd import simulation as sim, embed
    X, pt, br, sc = sim.sample_density(t, n, alpha=a, beta=b, out="torch"); p = embed.pca(X, sc)

Exact k nearest neighbours of the cells on the device (what ``pp.neighbors`` computes, from the PCA scores):

    from prosstt_amd import neighbors
    nb = neighbors.knn(p.scores, 14)                  # nb.indices, nb.sq_distances, nb.distances, nb.to_csr()

The UMAP layout of that neighbour graph on the device (what ``tl.umap`` computes, in a reproducible form):

    from prosstt_amd import layout
    lay = layout.umap(nb)                             # lay.embedding (cells, 2) float32

Louvain clusters of that neighbour graph on the device (what ``tl.louvain`` computes, in a reproducible form):

    from prosstt_amd import cluster
    cl = cluster.louvain(nb)                          # cl.labels (cells,) int32, 0 the largest cluster; cl.modularity

Which genes follow the structure of that graph, without labels (``metrics.morans_i`` / ``gearys_c``), and the smoothed matrix:

    from prosstt_amd import autocorr
    ac = autocorr.autocorrelation(X, sc, nb)          # ac.morans_i, ac.gearys_c, ac.z_i, ac.pvals_adj, ac.order

The way back from counts to the simulator's inputs: the count model's alpha and beta per gene, and the tree's means and
densities from cells that have a branch and a pseudotime:

    from prosstt_amd import fit, trends
    tr = trends.expression_trends(X, sc, t, pt, br)   # tr.means (nodes, genes), tr.density, tr.to_tree()
    f = fit.count_model(X, sc, tr.labels, tr.means)   # f.alpha, f.beta

Where every cell sits on the tree, for a matrix that does not come with its positions (the tree's own likelihood on the
matrix cores):

    from prosstt_amd import mapping
    m = mapping.map_cells(X, sc, t)                   # m.node, m.branches, m.pseudotime, m.posterior, m.branch_posterior

The tree itself, for a matrix that comes without one (a regularised principal tree in PCA or diffusion-map space):

    from prosstt_amd import ptree
    lf = ptree.principal_tree(p.scores).to_tree(root=start_cell, G=X.shape[1])   # lf.tree, lf.branches, lf.pseudotime, lf.node

A question of the trends with an error bar: which genes change along the tree, which diverge after a fork (a per-gene
regression of the counts on hat functions along the tree, under the count model's variance):

    from prosstt_amd import regress
    d = regress.tree_design(t, inner=1)
    r = regress.regression(X, sc, m.node, d, alpha=f.alpha, beta=f.beta)   # r.coef, r.se, r.fitted()
    r.wald(d.constant()).pvals_adj, r.wald(d.between("B", "C")).pvals_adj

How close an inferred trajectory is to the simulated truth (exact sums over all pairs of cells, by pair of true branches):

    from prosstt_amd import evaluate
    ev = evaluate.trajectory(t, pt, br, lf)           # ev.labels.accuracy, ev.ordering.comparable.gamma, ev.distances.pearson()

An embedding that knows the count model, in PCA's place (GLM-PCA: the low-rank log-bilinear structure the simulator draws from):

    from prosstt_amd import factors
    fa = factors.glmpca(X, sc, 10, alpha=f.alpha, beta=f.beta)   # fa.scores, fa.loadings, fa.intercept, fa.fitted(), fa.project(X2, sc2)

A knob chosen without a truth: split every count at random into a train and a test part (binomial thinning; also the way to
lower the depth of a matrix), fit on one, score on the other:

    from prosstt_amd import thin
    sp = thin.split(X, 0.5, seed=1)                   # sp.train + sp.test == X; sp.sizes(sc); thin.fold, thin.downsample
    thin.rank_curve(X, sc, (1, 2, 3, 5, 8), alpha=f.alpha, beta=f.beta).best

or, for unmodified scripts that say ``from prosstt import ...``:

    import prosstt_amd; prosstt_amd.install_as_prosstt()

Host code is Python; every O(time x genes) / O(cells x genes) step runs in
hand-written HIP kernels behind the C ABI of include/prosstt_amd.h.  No CPU fallback.
"""
import sys

__version__ = "0.1.0"


def install_as_prosstt():
    """Alias this package as ``prosstt`` in ``sys.modules`` (tree, simulation, sim_utils,
    count_model, tree_utils), so ``from prosstt import simulation as sim`` resolves here."""
    import importlib
    pkg = sys.modules[__name__]
    sys.modules["prosstt"] = pkg
    for name in ("tree", "simulation", "sim_utils", "count_model", "tree_utils"):
        sys.modules["prosstt." + name] = importlib.import_module(__name__ + "." + name)
    return pkg
