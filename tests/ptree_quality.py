"""What the numpy model of ptree reaches on smoke()'s tree, measured on the CPU without the code under test, and the two scores
the GPU test shares with the measurement.  A helper: nothing here is collected.

The protocol (``python tests/ptree_quality.py``): the node means (60 x 300), size factors, pseudotimes and branches of
``test_gpu_trends._simulation()`` are read from tests/golden/ptree_smoke_tree.npz (written once from that function on the
device: ``python tests/ptree_quality.py --dump``); for each of 24 seeds a 3 000 x 300 matrix of numpy's negative binomial
(n = mu / (alpha mu + beta - 1), p = 1 / (alpha mu + beta), mu = s_i mean, alpha = 0.2, beta = 2), the first N_COMPONENTS
principal components of log1p(x / s) by ``numpy.linalg.svd``, tests/ptree_model.py's ``principal_tree`` and ``to_tree`` with the
package's defaults, rooted at a cell of lowest true pseudotime.  Recorded: the share of seeds whose pruned tree has one fork and
three tips; over those seeds the share of cells on the true branch under the best matching of the three labels and the Spearman
correlation of ``position`` with the true pseudotime, as (mean, standard deviation, ddof 1)."""
import itertools
import os
import sys

import numpy as np

N_COMPONENTS = 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ptree_smoke_tree.npz")

# measured by main() below with the defaults of prosstt_amd/ptree.py (DESIGN section 28 has the table)
TOPOLOGY_RECOVERED = 23 / 24             # one fork and three tips; the 24th seed keeps a fourth tip of three nodes
BRANCH_ACCURACY = (0.670609, 0.029892)
SPEARMAN = (0.796392, 0.021503)


def branch_accuracy(labels, truth):
    """The share of cells on their true branch under the best one-to-one matching of the found labels to the true ones."""
    found, true = sorted(set(labels.tolist())), sorted(set(truth.tolist()))
    best = 0.0
    for perm in itertools.permutations(true, min(len(found), len(true))):
        best = max(best, float(np.mean([dict(zip(found, perm)).get(a) == b for a, b in zip(labels.tolist(), truth.tolist())])))
    return best


def _ranks(x):
    x = np.asarray(x, dtype=np.float64)
    values, inverse, counts = np.unique(x, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts)
    return ((ends - counts + 1 + ends) / 2.0)[inverse]


def spearman(a, b):
    ra, rb = _ranks(a), _ranks(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra @ rb) / np.sqrt((ra @ ra) * (rb @ rb)))


def numpy_counts(means, rows, sc, seed, alpha=0.2, beta=2.0):
    rng = np.random.default_rng(seed)
    mu = sc[:, None] * means[rows]
    return rng.negative_binomial(mu / (alpha * mu + beta - 1.0), 1.0 / (alpha * mu + beta))


def numpy_scores(x, sc, k):
    z = np.log1p(x / sc[:, None])
    z = z - z.mean(axis=0)
    u, s, _ = np.linalg.svd(z, full_matrices=False)
    return (u[:, :k] * s[:k]).astype(np.float32)


def one_seed(data, seed, **options):
    """(one fork and three tips?, branch accuracy, Spearman, the branch times) of one numpy-drawn matrix."""
    import ptree_model as pm
    x = numpy_counts(data["means"], data["rows"], data["sc"], seed)
    Y = numpy_scores(x, data["sc"], N_COMPONENTS)
    fit = {k: v for k, v in options.items() if k not in ("min_branch_nodes",)}
    C, edges, _, _, _, _, best = pm.principal_tree(Y, **fit)
    lf = pm.to_tree(Y, C, edges, best, int(np.argmin(data["pt"])), G=300,
                    **{k: v for k, v in options.items() if k == "min_branch_nodes"})
    parents = [p for p, _ in lf.tree.topology]
    ok = len(lf.tree.branches) == 3 and len(parents) == 2 and parents[0] == parents[1] == lf.tree.root
    return ok, branch_accuracy(lf.branches, data["br"]), spearman(lf.position, data["pt"]), dict(lf.tree.time)


def main(argv):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.dirname(here)]
    if "--dump" in argv:
        from test_gpu_trends import _simulation
        from prosstt_amd import fit, simulation as sim
        t, _, pt, br, sc = _simulation()
        np.savez_compressed(GOLDEN, means=fit.simulation_means(t).astype(np.float32), rows=sim.cell_rows(t, pt, br),
                            pt=pt.astype(np.int32), br=br.astype("U1"), sc=sc)
        return
    data = dict(np.load(GOLDEN))
    data["means"] = data["means"].astype(np.float64)
    options = {}
    for arg in argv:
        if "=" in arg:
            key, value = arg.split("=")
            options[key] = float(value) if "." in value or "e" in value else int(value)
    results = [one_seed(data, seed, **options) for seed in range(24)]
    good = [r for r in results if r[0]]
    print("options %s: topology recovered in %d of 24 seeds" % (options, len(good)))
    for name, col in (("branch accuracy", 1), ("Spearman", 2)):
        v = np.array([r[col] for r in good])
        print("  %s: mean %.6f, sd %.6f, min %.4f" % (name, v.mean(), v.std(ddof=1) if len(v) > 1 else 0.0, v.min()))
    print("  times of the first seeds: %s" % [r[3] for r in results[:3]])


if __name__ == "__main__":
    main(sys.argv[1:])
