"""-m gpu: what ``factors.glmpca`` reaches on smoke()'s tree with the package's defaults, on the device's own matrix of that tree
(``test_gpu_trends._simulation()``: 3 000 cells x 300 genes, alpha = 0.2, beta = 2), against what the numpy model of the loop
reaches on numpy's negative binomial from the same means, sizes and cells over 24 seeds (tests/factors_quality.py holds the
protocol, the scores and the constants; tools/factors_calibration.py writes them):

  (a) the rms of the fitted minus the true log-mean is within 5 sd of the model's;
  (b) the mean true tree distance from a cell to its 14 nearest neighbours in score space (``neighbors.knn``) is within 5 sd
      of the model's;
  (c) and it lies below the same distance in the space of ``embed.pca`` at equal k by the model's margin at its 5 sd low end,
      as regress's calibration has it: the embedding that knows the count model keeps a cell's neighbours nearer on the tree."""
import numpy as np
import pytest

import factors_quality as Q

pytestmark = pytest.mark.gpu


def test_the_defaults_are_the_calibrated_ones():
    from prosstt_amd import factors
    assert (Q.K, Q.PENALTY, Q.MAX_ROUNDS) == (10, factors.PENALTY, factors.MAX_ROUNDS)
    assert Q.LOG_MEAN_RMS[1] > 0 and Q.NEIGHBOUR_DISTANCE[1] > 0 and Q.MARGIN > 0


def test_quality_on_smokes_tree():
    import test_gpu_trends
    from prosstt_amd import embed, factors, fit, neighbors, simulation as sim
    t, X, pt, br, sc = test_gpu_trends._simulation()
    rows = sim.cell_rows(t, pt, br)
    f = factors.glmpca(X, sc, alpha=0.2, beta=2.0)
    assert f.scores.shape == (3000, Q.K) and f.rounds <= Q.MAX_ROUNDS
    falls = f.objective[:-1] - f.objective[1:]
    assert np.all(falls <= f.tol * (np.abs(f.objective[:-1]) + 1.0))
    rms = Q.log_mean_rms(f.linear_predictor(), fit.simulation_means(t)[rows], ~f.no_counts)
    mine = Q.neighbour_distance(neighbors.knn(f.scores, Q.N_NEIGHBORS).indices, pt, br)
    pca = Q.neighbour_distance(neighbors.knn(embed.pca(X, sc, Q.K).scores, Q.N_NEIGHBORS).indices, pt, br)
    print("glmpca on smoke()'s tree: %d rounds%s, log-mean rms %.4f (model %.4f, sd %.4f), neighbour distance %.4f (model %.4f, sd "
          "%.4f), of embed.pca %.4f (model's PCA %.4f): %.4f below it (margin %.4f)"
          % (f.rounds, ", converged" if f.converged else "", rms, *Q.LOG_MEAN_RMS, mine, *Q.NEIGHBOUR_DISTANCE, pca,
             Q.PCA_NEIGHBOUR_DISTANCE[0], pca - mine, Q.MARGIN))
    assert abs(rms - Q.LOG_MEAN_RMS[0]) <= 5.0 * Q.LOG_MEAN_RMS[1]
    assert abs(mine - Q.NEIGHBOUR_DISTANCE[0]) <= 5.0 * Q.NEIGHBOUR_DISTANCE[1]
    assert pca - mine >= Q.MARGIN
