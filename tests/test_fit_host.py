"""prosstt_amd/fit.py without a device: every refusal that needs none, ``LogLik.concat``, ``hyperparameters`` on a hand-made
fit, NaN for genes without counts, and ``maximize``'s determinism and scheme on plain functions."""
import numpy as np
import pytest

from prosstt_amd import fit


# ---------------------------------------------------------------------------------------------------------- refusals

def test_host_matrices_and_other_dtypes_are_refused():
    torch = pytest.importorskip("torch")
    X = np.ones((5, 4), dtype=np.int32)
    sc, means, ab = np.ones(5), np.ones((1, 4)), np.ones(4)
    with pytest.raises(TypeError, match="host arrays are refused"):
        fit.loglik(X, sc, None, means, ab, ab + 1)
    with pytest.raises(TypeError, match="host arrays are refused"):
        fit.count_model(X, sc)
    with pytest.raises(TypeError, match="int32"):
        fit.loglik(torch.ones((5, 4), dtype=torch.int64), sc, None, means, ab, ab + 1)
    with pytest.raises(ValueError, match="dimensions"):
        fit.loglik(torch.ones(5, dtype=torch.int32), sc, None, means, ab, ab + 1)
    with pytest.raises(ValueError, match="device tensor"):
        fit.loglik(torch.ones((5, 4), dtype=torch.int32), sc, None, means, ab, ab + 1)      # a CPU tensor


def test_shapes_and_candidate_counts_are_refused_before_any_device_use():
    torch = pytest.importorskip("torch")
    X = torch.ones((5, 4), dtype=torch.int32)          # (a CPU tensor: the checks below come before its device is asked for)
    sc, means, a, b = np.ones(5), np.ones((2, 4)), np.full(4, 0.1), np.full(4, 2.0)
    with pytest.raises(ValueError, match="candidates"):
        fit.loglik(X, sc, None, means, np.tile(a, (17, 1)), np.tile(b, (17, 1)))
    with pytest.raises(ValueError, match="4 genes"):
        fit.loglik(X, sc, None, means, a[:3], b[:3])
    with pytest.raises(ValueError, match="same shape"):
        fit.loglik(X, sc, None, means, np.tile(a, (2, 1)), b)
    with pytest.raises(ValueError, match="out must be"):
        fit.loglik(X, sc, None, means, a, b, out="cupy")
    with pytest.raises(ValueError, match="one size factor per cell"):
        fit.loglik(X, sc[:4], None, means, a, b)
    with pytest.raises(ValueError, match="means must be"):
        fit.loglik(X, sc, None, means[:, :3], a, b)
    with pytest.raises(ValueError, match="one label per cell"):
        fit.loglik(X, sc, np.zeros(4, dtype=np.int64), means, a, b)
    with pytest.raises(ValueError, match="integers or names"):
        fit.loglik(X, sc, np.zeros(5), means, a, b)


@pytest.mark.parametrize("options,match", [
    (dict(free=()), "free"), (dict(free=("gamma",)), "free"), (dict(free=("alpha", "alpha")), "free"),
    (dict(bounds=(4.0, -12.0)), "bounds"), (dict(bounds=(0.0,)), "bounds"), (dict(bounds=(-np.inf, 0.0)), "bounds"),
    (dict(tol=0.0), "tol"), (dict(max_rounds=0), "max_rounds"), (dict(max_rounds=2.5), "max_rounds"),
    (dict(alpha0=0.0), "alpha0"), (dict(beta0=1.0), "beta0"),
    (dict(free=("beta",), fixed_alpha=-1.0), "fixed_alpha"), (dict(free=("alpha",), fixed_beta=0.5), "fixed_beta"),
])
def test_bad_options_are_refused_by_maximize_and_by_count_model(options, match):
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match=match):
        fit.maximize(lambda a, b: -a - b, 3, **options)
    with pytest.raises(ValueError, match=match):       # before the matrix is looked at
        fit.count_model(torch.ones((5, 4), dtype=torch.int32), np.ones(5), **options)


def test_status_bits_are_named():
    fit.check_status(0)
    for bit, name in ((fit.NEGATIVE, "NEGATIVE"), (fit.LABEL, "LABEL"), (fit.PARAMETER, "PARAMETER"), (fit.SIZE, "SIZE"),
                      (fit.MEAN, "MEAN")):
        with pytest.raises(ValueError, match=r"status bit %s \(%d\)" % (name, bit)):
            fit.check_status(bit)
    with pytest.raises(ValueError, match="LABEL.*MEAN"):
        fit.check_status(fit.LABEL | fit.MEAN)
    with pytest.raises(RuntimeError):
        fit.check_status(32)


# ------------------------------------------------------------------------------------------------------------ concat

def test_loglik_concat_adds_in_list_order():
    rng = np.random.default_rng(1)
    parts = [fit.LogLik(rng.normal(size=(3, 5)), rng.random(5), rng.integers(0, 3, size=5), n) for n in (10, 20, 7)]
    whole = fit.LogLik.concat(parts)
    assert whole.n_cells == 37 and whole.n_genes == 5
    assert whole.values.tobytes() == ((parts[0].values + parts[1].values) + parts[2].values).tobytes()
    assert whole.base.tobytes() == ((parts[0].base + parts[1].base) + parts[2].base).tobytes()
    assert np.array_equal(whole.bad, parts[0].bad + parts[1].bad + parts[2].bad) and whole.bad.dtype == np.int64
    assert fit.LogLik.concat(parts[:1]).values is parts[0].values
    with pytest.raises(ValueError):
        fit.LogLik.concat([])
    with pytest.raises(TypeError):
        fit.LogLik.concat([parts[0], "x"])
    with pytest.raises(ValueError):
        fit.LogLik.concat([parts[0], fit.LogLik(np.zeros((2, 5)), np.zeros(5), np.zeros(5), 1)])
    with pytest.raises(ValueError):
        fit.LogLik(np.zeros((2, 5)), np.zeros(4), np.zeros(5), 1)


# ---------------------------------------------------------------------------------------------------------- maximize

def _paraboloid(centre_u, centre_v, cross=0.3):
    """A concave quadratic in (u, v) = (log alpha, log(beta - 1)) per gene, and a counter of its calls."""
    calls = []

    def evaluate(alpha, beta):
        calls.append(alpha.shape)
        du, dv = np.log(alpha) - centre_u[None, :], np.log(beta - 1.0) - centre_v[None, :]
        return -(2.0 * du * du + cross * du * dv + 0.7 * dv * dv)
    return evaluate, calls


def test_maximize_finds_the_top_of_a_quadratic_and_is_deterministic():
    rng = np.random.default_rng(3)
    cu, cv = rng.uniform(-8.0, 2.0, size=40), rng.uniform(-8.0, 2.0, size=40)
    evaluate, calls = _paraboloid(cu, cv)
    first = fit.maximize(evaluate, 40)
    assert set(calls) == {(10, 40)}                    # a 3 x 3 stencil and one quasi-Newton point per round, in one call
    assert first.converged.all() and not first.at_bound.any()
    np.testing.assert_allclose(first.u, cu, atol=1e-4)
    np.testing.assert_allclose(first.v, cv, atol=1e-4)
    assert np.all(first.value > -1e-7) and first.rounds.max() <= 30
    again = fit.maximize(_paraboloid(cu, cv)[0], 40)
    for a, b in zip(first, again):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()
    # a gene's path does not depend on the other genes of the call
    alone = fit.maximize(_paraboloid(cu[7:8], cv[7:8])[0], 1)
    assert alone.u.tobytes() == first.u[7:8].tobytes() and alone.rounds[0] == first.rounds[7]


def test_maximize_with_one_free_parameter_uses_three_points_and_keeps_the_other_fixed():
    cu = np.array([-3.0, 0.5, -11.0])
    evaluate, calls = _paraboloid(cu, np.zeros(3), cross=0.0)
    seen_beta = []

    def spy(alpha, beta):
        seen_beta.append(np.unique(beta))
        return evaluate(alpha, np.full(beta.shape, 2.0))
    got = fit.maximize(spy, 3, free=("alpha",))
    assert set(calls) == {(4, 3)}
    assert all(b.tolist() == [1.0] for b in seen_beta) and np.all(got.beta == 1.0) and np.all(np.isnan(got.v))
    np.testing.assert_allclose(got.u, cu, atol=1e-4)
    evaluate, calls = _paraboloid(np.zeros(3), cu, cross=0.0)
    got = fit.maximize(lambda a, b: evaluate(np.ones(a.shape), b), 3, free=("beta",), fixed_alpha=0.0)
    assert np.all(got.alpha == 0.0) and np.all(np.isnan(got.u))
    np.testing.assert_allclose(got.v, cu, atol=1e-4)


def test_maximize_stops_on_the_box_takes_ties_at_the_centre_and_survives_nan():
    evaluate, _ = _paraboloid(np.array([-20.0, 9.0]), np.array([0.0, 0.0]))
    got = fit.maximize(evaluate, 2)
    assert got.at_bound.all() and got.converged.all()
    assert got.u.tolist() == [-12.0, 4.0]
    flat = fit.maximize(lambda a, b: np.zeros(a.shape), 2, alpha0=0.5, beta0=3.0)
    assert np.all(flat.alpha == 0.5) and np.all(flat.beta == 3.0) and flat.converged.all()      # a tie: the centre stays
    assert flat.rounds.tolist() == [14, 14]            # h = 1 halves every round until it is below 1e-4
    holes = fit.maximize(lambda a, b: np.where(a > 1.0, np.nan, evaluate(a, b)), 2)
    assert np.all(np.isfinite(holes.value)) and np.all(holes.alpha <= 1.0)
    short = fit.maximize(evaluate, 2, max_rounds=3)
    assert not short.converged.any() and short.rounds.tolist() == [3, 3]


# ------------------------------------------------------------------------------------------- the fit and its summary

def test_genes_without_counts_or_with_bad_entries_are_nan():
    evaluate, _ = _paraboloid(np.full(4, -1.0), np.full(4, 0.5))
    got = fit.fit_with(evaluate, 4, base=np.array([1.0, 2.0, 3.0, 4.0]), bad=np.array([0, 2, 0, 0]),
                       has_counts=np.array([True, True, False, True]))
    assert got.converged.tolist() == [True, False, False, True]
    for field in (got.alpha, got.beta, got.loglik, got.se_log_alpha, got.se_log_beta_minus_1):
        assert np.isnan(field).tolist() == [False, True, True, False]
    assert np.isnan(got.hessian).all(axis=1).tolist() == [False, True, True, False]
    np.testing.assert_allclose(got.loglik[[0, 3]], [-1.0, -4.0], atol=1e-7)      # the value at the top is 0: base is taken off
    np.testing.assert_allclose(got.hessian[0], [-4.0, -0.3, -1.4], rtol=1e-6)
    cov = np.linalg.inv(np.array([[4.0, 0.3], [0.3, 1.4]]))
    np.testing.assert_allclose([got.se_log_alpha[0], got.se_log_beta_minus_1[0]], np.sqrt(np.diag(cov)), rtol=1e-6)
    assert got.bad.tolist() == [0, 2, 0, 0] and got.free == ("alpha", "beta")


def _hand_made(alpha, beta, converged, at_bound, free=("alpha", "beta")):
    G = len(alpha)
    nan = np.full(G, np.nan)
    return fit.CountModelFit(np.asarray(alpha, dtype=float), np.asarray(beta, dtype=float), nan, np.zeros(G, dtype=np.int64),
                             np.asarray(converged), np.asarray(at_bound), np.full((G, 3), np.nan), nan, nan, None,
                             np.zeros(G, dtype=np.int64), free)


def test_hyperparameters_of_a_hand_made_fit():
    f = _hand_made([np.e, np.e ** 3, 50.0, np.nan], [1 + np.e ** 2, 1 + np.e ** 4, 9.0, np.nan],
                   [True, True, True, False], [False, False, True, False])
    hp = fit.hyperparameters(f)
    assert hp.n_genes == 2                             # the gene on the box and the one that did not converge are left out
    assert hp.log_alpha_mean == pytest.approx(2.0) and hp.log_alpha_std == pytest.approx(np.sqrt(2.0))
    assert hp.log_beta_minus_1_mean == pytest.approx(3.0) and hp.log_beta_minus_1_std == pytest.approx(np.sqrt(2.0))
    one = fit.hyperparameters(_hand_made([np.e], [1.0], [True], [False], free=("alpha",)))
    assert one.n_genes == 1 and one.log_alpha_mean == pytest.approx(1.0) and np.isnan(one.log_alpha_std)
    assert np.isnan(one.log_beta_minus_1_mean) and np.isnan(one.log_beta_minus_1_std)
    none = fit.hyperparameters(_hand_made([1.0], [2.0], [False], [False]))
    assert none.n_genes == 0 and np.isnan(none.log_alpha_mean)
    with pytest.raises(TypeError):
        fit.hyperparameters("fit")
