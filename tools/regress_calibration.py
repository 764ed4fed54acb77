"""The null distribution that tests/test_gpu_regress.py::test_calibration_of_the_wald_statistic compares the device with:
the numpy model of the regression (tests/regress_model.py) on numpy's negative binomial, from the means of smoke()'s tree
flattened per gene and from the sizes and labels of the test's own 3 000 cells, over 24 seeds.  Prints the constants of the
test: the mean over the genes of the Wald statistic of "all knots equal" and the share above the chi-square 95 % point of 6
degrees of freedom, each with its standard deviation over the seeds, and on the tree as it is the share of rejections less
the null share.  Needs the device once, for the tree and the plan of the cells (the sampler's host draws); the 24 fits are
numpy's, and run without a device from a file of those inputs.

    python tools/regress_calibration.py [--seeds 24] [--dump inputs.npz | --load inputs.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def draw(rng, mu, alpha, beta):
    var = alpha * mu * mu + beta * mu
    return rng.negative_binomial(mu * mu / (var - mu), mu / var)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--dump", help="write the inputs (means, rows, sizes and design of both trees) to this .npz and stop")
    ap.add_argument("--load", help="read the inputs from this .npz instead of the device")
    args = ap.parse_args()
    import scipy.stats
    import regress_model as M
    from prosstt_amd import regress
    point = scipy.stats.chi2.ppf(0.95, 6)
    if args.load:
        inputs = dict(np.load(args.load))
    else:
        import test_gpu_regress as T
        from prosstt_amd import fit
        inputs = {}
        for flat in (True, False):
            X, rows, sc, t = T._sampled(flat)
            inputs.update({"means%d" % flat: fit.simulation_means(t), "rows%d" % flat: rows, "sc%d" % flat: sc,
                           "design": regress.tree_design(t, 1).matrix})
    if args.dump:
        np.savez(args.dump, **inputs)
        return
    from prosstt_amd.tree import Tree
    design = regress.tree_design(Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 20, "B": 20, "C": 20}, num_branches=3,
                                      branch_points=1, modules=5, G=300), 1)
    assert np.array_equal(design.matrix, inputs["design"])
    out = {}
    for flat in (True, False):
        rows, sc = inputs["rows%d" % flat], inputs["sc%d" % flat]
        mu = sc[:, None] * inputs["means%d" % flat][rows]
        stats = []
        for seed in range(args.seeds):
            Xs = draw(np.random.default_rng(1000 + seed), mu, 0.2, 2.0)
            r = M.regression(Xs, sc, rows, design, 0.2, 2.0, ordered=False)
            w = r.wald(design.constant())
            have = np.isfinite(w.statistic)
            stats.append((w.statistic[have].mean(), (w.statistic[have] > point).mean(), r.rounds[have].max(), have.sum()))
            print("flat=%s seed %d: mean %.4f share %.4f rounds <= %d genes %d" % ((flat, seed) + stats[-1]), flush=True)
        out[flat] = np.array(stats)
    null, changing = out[True], out[False]
    print("NULL_MEAN, NULL_MEAN_SD = %.4f, %.4f" % (null[:, 0].mean(), null[:, 0].std(ddof=1)))
    print("NULL_SHARE, NULL_SHARE_SD = %.4f, %.4f" % (null[:, 1].mean(), null[:, 1].std(ddof=1)))
    print("CHANGING_SHARE, CHANGING_SHARE_SD = %.4f, %.4f" % (changing[:, 1].mean(), changing[:, 1].std(ddof=1)))
    print("(the lowest share of a seed on the tree as it is: %.4f)" % changing[:, 1].min())


if __name__ == "__main__":
    main()
