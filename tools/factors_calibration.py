"""The figures that tests/test_gpu_factors_quality.py compares the device with, and the table that chose the defaults of
``factors.glmpca``: the numpy model of the loop (tests/factors_model.py, numpy's own sums, the gene half through the
transposed cell half) on numpy's negative binomial from the node means, sizes and cells of tests/golden/ptree_smoke_tree.npz
(alpha = 0.2, beta = 2), from the "pca" start computed by numpy.  tests/factors_quality.py holds the protocol and the scores.
Needs no device.

    python tools/factors_calibration.py [--seeds 24] [--write]        the package's defaults: prints the constants of
                                                                      tests/factors_quality.py, --write puts them there
    python tools/factors_calibration.py --table --seeds 4             k = 3, 5, 10 x penalty = 1, 10, 50: DESIGN section 35's table
"""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def one_seed(data, seed, k, penalty, max_rounds, tol):
    """(rms of the log-mean, neighbour distance of the factors, of PCA, rounds, halvings after round 0, largest fall)."""
    import factors_model as M
    import factors_quality as Q
    import ptree_quality
    x = ptree_quality.numpy_counts(data["means"], data["rows"], data["sc"], seed)
    sc, pt, br = data["sc"], data["pt"], data["br"]
    scores, loadings = Q.pca_start(x, sc, k)
    history = []
    f = M.glmpca(x, sc, scores, 0.2, 2.0, loadings=loadings, ordered=False, transposed=True, history=history, penalty=penalty,
                 max_rounds=max_rounds, tol=tol)
    falls = f.objective[:-1] - f.objective[1:]
    later = sum(int((r.gene_halvings != 0).sum() + (r.cell_halvings != 0).sum()) for r in history[1:])
    return (Q.log_mean_rms(f.linear_predictor(), data["means"][data["rows"]], ~f.no_counts),
            Q.neighbour_distance(Q.nearest(f.scores), pt, br),
            Q.neighbour_distance(Q.nearest(ptree_quality.numpy_scores(x, sc, k)), pt, br), f.rounds, later,
            float(falls.max()) if falls.size else 0.0)


def main():
    from prosstt_amd import factors
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=24)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--tol", type=float, default=factors.TOL)
    args = ap.parse_args()
    import ptree_quality
    data = dict(np.load(ptree_quality.GOLDEN))
    data["means"] = data["means"].astype(np.float64)
    data["br"] = data["br"].astype("U1")
    grid = [(k, penalty) for k in (3, 5, 10) for penalty in (1.0, 10.0, 50.0)] if args.table else [(10, factors.PENALTY)]
    for k, penalty in grid:
        t0 = time.time()
        rows = np.array([one_seed(data, seed, k, penalty, factors.MAX_ROUNDS, args.tol) for seed in range(args.seeds)])
        mean, sd = rows.mean(axis=0), rows.std(axis=0, ddof=1) if len(rows) > 1 else np.zeros(rows.shape[1])
        print("k = %d, penalty = %g, %d seeds (%.0f s): log-mean rms %.4f (sd %.4f), neighbour distance %.4f (sd %.4f), of PCA %.4f "
              "(sd %.4f), rounds %.1f (at most %d), halvings after round 0: %d, largest fall of the objective %.3g"
              % (k, penalty, args.seeds, time.time() - t0, mean[0], sd[0], mean[1], sd[1], mean[2], sd[2], mean[3], rows[:, 3].max(),
                 rows[:, 4].sum(), rows[:, 5].max()), flush=True)
    if not args.table:
        lines = ["K, PENALTY, MAX_ROUNDS = %d, %r, %d" % (10, factors.PENALTY, factors.MAX_ROUNDS),
                 "LOG_MEAN_RMS = (%.4f, %.4f)" % (mean[0], sd[0]), "NEIGHBOUR_DISTANCE = (%.4f, %.4f)" % (mean[1], sd[1]),
                 "PCA_NEIGHBOUR_DISTANCE = (%.4f, %.4f)" % (mean[2], sd[2])]
        print("\n".join(lines))
        if args.write:
            path = os.path.join(ROOT, "tests", "factors_quality.py")
            text = open(path).read()
            text = re.sub(r"(---- begin\n).*?(# ---- end)", lambda m: m.group(1) + "\n".join(lines) + "\n" + m.group(2), text, flags=re.S)
            open(path, "w").write(text)


if __name__ == "__main__":
    main()
