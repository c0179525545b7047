"""CPU checks of the GMM block: the float64 restatement of tests/gmm_cases.py against sklearn and the fixtures, every size limit as a
ValueError with no device, the parameter counts of bic / aic, from_params / to_sklearn, and the rules the GPU tests lean on (the stop
margins of the whole-fit cases, the share of rows the hard-assignment tests may exclude, the derived float32 bounds against a float32
run of the same loop)."""
import os

import numpy as np
import pytest
import torch

import gmm_cases as G
from frl_hip import _lib, clustering, ops
from frl_hip.clustering import DiagGMM

try:
    import sklearn.mixture  # noqa: F401
    HAVE_SKLEARN = True
except Exception:  # pragma: no cover
    HAVE_SKLEARN = False
needs_sklearn = pytest.mark.skipif(not HAVE_SKLEARN, reason="sklearn is not installed")


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"gmm_{name}.npz"))


_FITS = {}


def _fit64(case):
    if case not in _FITS:
        inp = G.make_inputs(case)
        _FITS[case] = (inp, G.fit(inp["X"], inp["w"], inp["weights_init"], inp["means_init"], inp["variances_init"]))
    return _FITS[case]


@pytest.mark.parametrize("case", G.STEP_CASES)
def test_fixture_loads_and_inputs_regenerate(golden_dir, case):
    fx = _fx(golden_dir, case)
    assert int(fx["checksum"]) == G.checksum(G.make_inputs(case))
    k, d = fx["means"].shape
    assert fx["weights"].shape == (k,) and fx["covariances"].shape == (k, d)


@pytest.mark.parametrize("case", G.FIT_CASES)
def test_restatement_reproduces_the_fixture_fit(golden_dir, case):
    """sklearn's result (for j: on the rows repeated by their integer weights) against the weighted float64 restatement."""
    fx = _fx(golden_dir, case)
    inp, f = _fit64(case)
    assert f["n_iter"] == int(fx["n_iter"]) and f["converged"] == bool(fx["converged"])
    scale = max(1.0, np.abs(fx["means"]).max())
    assert np.abs(f["means"] - fx["means"]).max() <= 1e-9 * scale
    assert np.abs(f["covariances"] - fx["covariances"]).max() <= 1e-8 * scale
    assert np.abs(f["weights"] - fx["weights"]).max() <= 1e-9
    assert abs(f["lower_bounds"][-1] - float(fx["lower_bound"])) <= 1e-7
    lp, lse, _ = G.e_step(inp["X"], f["weights"], f["means"], f["covariances"])
    assert np.abs(lse - fx["score_samples"]).max() <= 1e-7 * max(1.0, np.abs(lse).max())
    assert (lp.argmax(1) != fx["predict"]).mean() <= 1e-3


@pytest.mark.parametrize("case", ["f", "g", "h"])
def test_restatement_reproduces_the_fixture_step(golden_dir, case):
    fx = _fx(golden_dir, case)
    inp = G.make_inputs(case)
    pi, mu, var, lb = G.em_step(inp["X"], None, inp["weights_init"], inp["means_init"], inp["variances_init"])
    assert np.abs(mu - fx["means"]).max() <= 1e-9 and np.abs(var - fx["covariances"]).max() <= 1e-8
    assert np.abs(pi - fx["weights"]).max() <= 1e-9 and abs(lb - float(fx["lower_bound"])) <= 1e-7


@needs_sklearn
@pytest.mark.parametrize("case", ["a", "d", "j"])
def test_restatement_agrees_with_sklearn_live(case):
    from sklearn.mixture import GaussianMixture
    inp, f = _fit64(case)
    X = inp["X"].astype(np.float64)
    if inp["w"] is not None:
        X = np.repeat(X, inp["w"].astype(int), axis=0)                           # integer weights are repeated rows
    pi = inp["weights_init"].astype(np.float64)
    g = GaussianMixture(len(pi), covariance_type="diag", tol=G.TOL, reg_covar=G.REG_COVAR, max_iter=G.MAX_ITER, weights_init=pi / pi.sum(),
                        means_init=inp["means_init"].astype(np.float64), precisions_init=1.0 / inp["variances_init"].astype(np.float64)).fit(X)
    assert g.n_iter_ == f["n_iter"]
    assert np.abs(g.means_ - f["means"]).max() <= 1e-9 and abs(g.lower_bound_ - f["lower_bounds"][-1]) <= 1e-7


@pytest.mark.parametrize("case", G.FIT_CASES)
def test_whole_fit_cases_stop_clear_of_tol(case):
    hi, lo = G.stop_margins(_fit64(case)[1]["lower_bounds"])
    assert hi >= 2 * G.TOL and lo <= G.TOL / 2, (hi, lo)


@pytest.mark.parametrize("case", G.HARD_CASES)
def test_hard_assignment_excludes_few_rows(case):
    inp = G.make_inputs(case)
    c = inp["X"][inp["init_rows"]].astype(np.float64)
    for _ in range(3):
        _, new, gap = G.lloyd_step(inp["X"], None, c)
        assert (gap <= G.hard_gap_bound(inp["X"], c)).mean() < 0.005
        c = new


@pytest.mark.parametrize("case", list("abcde"))
def test_float32_run_of_the_loop_is_within_the_derived_bounds(case):
    """The yardstick: numpy's float32 evaluation of the same step stays inside the bounds the GPU test derives."""
    inp = G.make_inputs(case)
    a = (inp["weights_init"], inp["means_init"], inp["variances_init"])
    b = G.step_bounds(inp["X"], inp["w"], *a)
    p64, m64, v64, l64 = G.em_step(inp["X"], inp["w"], *a)
    p32, m32, v32, l32 = G.em_step(inp["X"], inp["w"], *a, dtype=np.float32)
    assert np.abs(m32 - m64).max() <= b["mu"] and np.abs(v32 - v64).max() <= b["var_rel"] * v64.max()
    assert np.abs(p32 - p64).max() <= b["pi"] and abs(l32 - l64) <= b["lb"]
    print(case, b)
    assert b["mu"] <= 1e-4 and b["var_rel"] <= 5e-4                             # and the bounds stay within sight of 1e-5


def test_phase_summary_restatement_equals_the_reference(golden_dir):
    fx = _fx(golden_dir, "phase")
    for shape in G.PHASE_SHAPES:
        key = "x".join(map(str, shape))
        s, v = G.phase_summary(*G.make_phase_inputs(shape))
        assert np.abs(s - fx["summary_" + key]).max() <= 2e-6
        assert np.array_equal(np.isnan(v), np.isnan(fx["tvar_" + key])) and np.isnan(v).all() == (shape[1] == 1)
        assert np.nanmax(np.abs(v - fx["tvar_" + key]), initial=0.0) <= 2e-6


# ---- limits, with no device ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,k", [(10, 4, 0), (200, 4, 129), (200, 0, 2), (200, 129, 2), (200, 128, 65), (200, 65, 127), (3, 4, 4)])
def test_size_limits_raise_value_error(n, d, k):
    x = torch.zeros(n, d)
    with pytest.raises(ValueError):
        ops.chk_gmm(x, k)
    if 1 <= k <= 128:
        with pytest.raises(ValueError):
            DiagGMM(k).fit(x)
    else:
        with pytest.raises(ValueError):
            DiagGMM(k)


def test_other_limits_raise_value_error():
    x = torch.zeros(100, 8)
    with pytest.raises(ValueError):
        ops.chk_gmm(x.double(), 2)
    with pytest.raises(ValueError):
        ops.chk_gmm(x.t(), 2)
    with pytest.raises(ValueError):
        ops.chk_gmm(x, 2, sample_weight=torch.zeros(99))
    with pytest.raises(ValueError):
        ops.chk_gmm(x, 2, workgroups=4097)
    with pytest.raises(ValueError):
        ops.chk_gmm_dims(2 ** 31, 8, 2)
    with pytest.raises(ValueError):
        DiagGMM(2, covariance_type="full")
    with pytest.raises(ValueError):
        DiagGMM(2, init_rows=np.array([[0, 100]])).fit(x)
    with pytest.raises(ValueError):
        DiagGMM(2, means_init=np.zeros((3, 8))).fit(x)
    with pytest.raises(ValueError):
        ops.chk_phase_summary(torch.zeros(4, 65, 8), torch.zeros(4, 65))
    with pytest.raises(ValueError):
        ops.chk_phase_summary(torch.zeros(4, 5, 65), torch.zeros(4, 5))
    with pytest.raises(ValueError):
        ops.chk_phase_summary(torch.zeros(4, 5, 8), torch.zeros(4, 6))


def test_cpu_tensors_raise_frl_hip_error():
    x = torch.zeros(100, 8)
    with pytest.raises(_lib.FrlHipError):
        DiagGMM(2).fit(x)
    with pytest.raises(_lib.FrlHipError):
        clustering.phase_summary(torch.zeros(4, 5, 8), torch.zeros(4, 5))
    g = DiagGMM.from_params(np.full(2, 0.5), np.zeros((2, 8)), np.ones((2, 8)))
    with pytest.raises(_lib.FrlHipError):
        g.predict(x)


def test_bic_and_aic_parameter_counts():
    g = DiagGMM.from_params(np.full(7, 1 / 7), np.zeros((7, 65)), np.ones((7, 65)))
    assert g._n_parameters() == 2 * 7 * 65 + 7 - 1 == G.n_parameters(7, 65)
    if HAVE_SKLEARN:
        assert g.to_sklearn()._n_parameters() == g._n_parameters()


@needs_sklearn
@pytest.mark.parametrize("case", ["b", "e"])
def test_from_params_to_sklearn_predicts_and_scores_like_the_restatement(case):
    inp, f = _fit64(case)
    sk = DiagGMM.from_params(f["weights"], f["means"], f["covariances"]).to_sklearn()
    pi, mu, var = (a.astype(np.float32).astype(np.float64) for a in (f["weights"], f["means"], f["covariances"]))   # what from_params keeps
    X = inp["X"].astype(np.float64)
    lp, lse, resp = G.e_step(X, pi, mu, var)
    assert np.abs(sk.score_samples(X) - lse).max() <= 1e-9 * np.abs(lse).max()
    assert np.array_equal(sk.predict(X), lp.argmax(1))
    assert np.abs(sk.predict_proba(X) - resp).max() <= 1e-9
    assert abs(sk.bic(X) - G.bic(X, pi, mu, var)) <= 1e-6 and abs(sk.aic(X) - G.aic(X, pi, mu, var)) <= 1e-6
