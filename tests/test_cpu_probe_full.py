"""CPU tests of the phase probe's "full" design (frl_hip/probe.py: InteractionProbe): the host algebra from moments about a pivot against
the float64 restatement of the reference's two passes (tests/probe_full_cases.py) and what the reference's own transform gave
(tests/golden/probe_full_*.npz).  The tolerances are those of the 'two algebras' paragraph of probe_full_cases.py."""
import os

import numpy as np
import pytest
import torch

import probe_full_cases as FC
from frl_hip import _lib, probe as P
from frl_hip.probe import InteractionProbe

U = FC.U32
_FIT = {}


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"probe_full_{name}.npz"))


def _fit(case, k=None):
    """The restatement of a case and a probe solved from its exact float64 moments about a pivot that is not the mean: made once."""
    if (case, k) not in _FIT:
        inp = FC.make_inputs(case)
        r = FC.two_passes(inp, k)
        m = r["m"]
        dt, dp = r["zt"].shape[1], r["zp"].shape[1]
        rng = np.random.default_rng(7)
        centre = np.concatenate([r["zt"][m].mean(0), r["zp"][m].mean(0), r["Y"][m].mean(0)]).astype(np.float64)
        pivot = (centre + rng.normal(0.0, 0.2, size=centre.shape)).astype(np.float32)      # as far off as one sample's means are off the fit's
        S, Scq, Sqq = FC.exact_moments(r["zt"], r["zp"], r["Y"], m, pivot)
        g = InteractionProbe.from_moments(S, Scq, Sqq, r["n"], pivot, dt, dp, FC.RIDGE, inp["k"] if k is None else k)
        W, b = g.solve()
        _FIT[(case, k)] = dict(inp=inp, r=r, g=g, W=W.numpy(), b=b.numpy(), dm=dt + dp)
    return _FIT[(case, k)]


@pytest.mark.parametrize("case", FC.GOLDEN_CASES)
def test_inputs_are_well_posed(golden_dir, case):
    """The conditions on the inputs, from the restatement alone: a top-k subspace that is well defined, a system that is well conditioned."""
    fx, f = _fx(golden_dir, case), _fit(case)
    assert FC.checksum(f["inp"]) == int(fx["checksum"])
    pre = f["r"]["pre"]
    print(f"case {case}: n {f['r']['n']}, gap {pre['gap']:.3g}, cond {f['r']['cond']:.3g}, offset ratio {pre['offset_ratio']:.3g}")
    assert pre["gap"] >= 1e-3 and f["r"]["cond"] < 1e4
    assert np.array_equal(pre["mean"], fx["mean"]) and np.array_equal(pre["std"], fx["std"]) and int(fx["n_obs"]) == f["r"]["n"]


@pytest.mark.parametrize("case", FC.GOLDEN_CASES)
def test_solve_from_moments_against_golden(golden_dir, case):
    fx, f = _fx(golden_dir, case), _fit(case)
    g, r, dm = f["g"], f["r"], f["dm"]
    pre = r["pre"]
    tol = FC.algebra_tolerances(r["n"], r["cond"], pre["gap"], pre["offset_ratio"])
    print(f"case {case}: eps {tol['eps']:.2e}, turn {tol['turn']:.2e}, solve {tol['solve']:.2e}")
    assert g.n_obs_ == int(fx["n_obs"]) and g.output_dim == dm + pre["comp"].shape[1] == f["W"].shape[0]
    # mean and std to float32 rounding
    mean, std = g.mean_.numpy(), g.std_.numpy()
    assert mean.dtype == np.float32 and std.dtype == np.float32
    scale = np.abs(fx["mean"]).astype(np.float64) + fx["std"]
    assert np.all(np.abs(mean.astype(np.float64) - fx["mean"]) <= (U + tol["eps"]) * scale)
    assert np.all(np.abs(std.astype(np.float64) - fx["std"]) <= (U + tol["eps"] * (1 + pre["offset_ratio"])) * fx["std"])
    # the explained-variance ratios: eigenvalues move by eps of the largest
    evr = g.pca_explained_variance_ratio_.numpy()
    assert evr.dtype == np.float32 and np.all(np.abs(evr - fx["evr"]) <= U * fx["evr"] + 4 * tol["eps"] * fx["evr"][0])
    # comp comp^T on the stored rows
    comp = g.pca_components_.double().numpy()
    assert g.pca_components_.dtype == torch.float32 and comp.shape == pre["comp"].shape
    cr = fx["cct_rows"]
    d_cct = np.abs(comp[cr] @ comp.T - fx["cct"])
    b_cct = (tol["turn"] + 2 * U) * pre["weight"][cr] + 1e-300
    print(f"   comp comp^T at most {(d_cct / b_cct).max():.3f} of its bound")
    assert np.all(d_cct <= b_cct)
    # the model: main effects, bias, and the interaction part carried back to the standardised interaction columns
    wmax = max(np.abs(fx["W_main"]).max(), np.abs(r["W"][dm:]).max())
    d_w = tol["solve"] * wmax + U * np.abs(fx["W_main"])
    assert f["W"].dtype == np.float32 and np.all(np.abs(f["W"][:dm] - fx["W_main"]) <= d_w)
    assert np.all(np.abs(f["b"] - fx["b"]) <= tol["solve"] * np.abs(fx["b"]).max() + U * np.abs(fx["b"]))
    d_cw = np.abs(comp @ f["W"][dm:].astype(np.float64) - fx["comp_w"])
    b_cw = (tol["solve"] + tol["turn"] + 3 * U) * (np.abs(pre["comp"].astype(np.float64)) @ np.abs(r["W"][dm:]))
    assert np.all(d_cw <= b_cw + tol["solve"] * np.abs(fx["comp_w"]).max())
    # W and b against pass 2 of the restatement on the probe's own stored preprocessor: the R map
    own = dict(mean=mean, std=std, comp=g.pca_components_.numpy())
    m = r["m"]
    W2, b2, cond2 = FC.ridge(own, r["zt"][m], r["zp"][m], r["Y"][m])
    t2 = 8.0 * cond2 * tol["eps"]
    assert np.all(np.abs(g.coef64_.numpy() - W2) <= t2 * np.abs(W2).max()) and np.all(np.abs(g.intercept64_.numpy() - b2) <= t2 * np.abs(b2).max())
    # predictions through transform
    X = g.transform(torch.from_numpy(r["zt"][m]), torch.from_numpy(r["zp"][m]))
    assert X.dtype == torch.float32 and tuple(X.shape) == (r["n"], g.output_dim)
    pred = X.double().numpy() @ f["W"].astype(np.float64) + f["b"].astype(np.float64)
    mag = np.abs(X.double().numpy()) @ np.abs(f["W"].astype(np.float64)) + np.abs(f["b"])
    d_pred = (tol["solve"] + tol["turn"] + 3 * U) * mag                          # float32 rows, W and b on top of the algebra
    print(f"   pred at most {(np.abs(pred - fx['pred_64']) / d_pred).max():.3f} of its bound, largest |pred| {np.abs(fx['pred_64']).max():.3g}")
    assert np.all(np.abs(pred - fx["pred_64"]) <= d_pred)


@pytest.mark.parametrize("case", FC.GOLDEN_CASES)
def test_transform_equals_the_reference_rows_bit_for_bit(golden_dir, case):
    """The column order i Dp + a and the arithmetic of ProbePreprocessor.transform, with the reference's stored preprocessor loaded."""
    fx, f = _fx(golden_dir, case), _fit(case)
    r = f["r"]
    pre, m = r["pre"], r["m"]
    dt, dp = r["zt"].shape[1], r["zp"].shape[1]
    k = pre["comp"].shape[1]
    g = InteractionProbe().set_model(np.zeros((dt + dp + k, r["Y"].shape[1]), np.float32), np.zeros(r["Y"].shape[1], np.float32), fx["mean"], fx["std"],
                                     pre["comp"], d_type=dt, d_phase=dp)
    rows = fx["rows"]
    X = g.transform(torch.from_numpy(r["zt"][m][rows]), torch.from_numpy(r["zp"][m][rows]))
    assert X.dtype == torch.float32 and np.array_equal(X.numpy(), fx["X_rows"])


def test_without_pca_and_with_k_beyond_dq(golden_dir):
    fx, f = _fx(golden_dir, "a_k0"), _fit("a", 0)
    g, r, dm = f["g"], f["r"], f["dm"]
    assert g.pca_components_ is None and g.pca_explained_variance_ratio_ is None and g.output_dim == 5 + 3 + 15 == f["W"].shape[0]
    tol = FC.algebra_tolerances(r["n"], r["cond"], np.inf, r["pre"]["offset_ratio"])
    W64 = np.concatenate([fx["W_main"], fx["W_int"]])
    assert np.all(np.abs(f["W"] - W64) <= tol["solve"] * np.abs(W64).max() + U * np.abs(W64))
    assert np.all(np.abs(f["b"] - fx["b"]) <= tol["solve"] * np.abs(fx["b"]).max() + U * np.abs(fx["b"]))
    m = r["m"]
    X = g.transform(torch.from_numpy(r["zt"][m][fx["rows"]]), torch.from_numpy(r["zp"][m][fx["rows"]]))
    own = dict(mean=g.mean_.numpy(), std=g.std_.numpy(), comp=None)
    assert np.array_equal(X.numpy(), FC.transform(own, r["zt"][m][fx["rows"]], r["zp"][m][fx["rows"]]))
    # k beyond Dq keeps every component: a rotation of the standardised block, the same predictions
    big = _fit("a", 99)["g"]
    assert tuple(big.pca_components_.shape) == (15, 15) and big.output_dim == 23 and big.preprocessor_dict()["preprocessor_interaction_pca_k"] == 15
    assert abs(float(big.pca_explained_variance_ratio_.double().sum()) - 1.0) <= 16 * U


def test_preprocessor_dict_and_design_dim():
    g = _fit("b")["g"]
    d = g.preprocessor_dict()
    assert set(d) == {"preprocessor_mean", "preprocessor_std", "preprocessor_pca_components", "preprocessor_interaction_pca_k", "preprocessor_design",
                      "preprocessor_pca_explained_variance_ratio", "preprocessor_d_type", "preprocessor_d_phase"}
    assert d["preprocessor_mean"].dtype == torch.float32 and tuple(d["preprocessor_mean"].shape) == (16 + 4 + 64,)
    assert d["preprocessor_std"].dtype == torch.float32 and tuple(d["preprocessor_std"].shape) == (84,)
    assert d["preprocessor_pca_components"].dtype == torch.float32 and tuple(d["preprocessor_pca_components"].shape) == (64, 8)
    assert d["preprocessor_pca_explained_variance_ratio"].dtype == torch.float32 and tuple(d["preprocessor_pca_explained_variance_ratio"].shape) == (8,)
    assert (d["preprocessor_interaction_pca_k"], d["preprocessor_design"], d["preprocessor_d_type"], d["preprocessor_d_phase"]) == (8, "full", 16, 4)
    assert all(not t.is_cuda for t in d.values() if isinstance(t, torch.Tensor))
    k0 = _fit("a", 0)["g"].preprocessor_dict()
    assert k0["preprocessor_pca_components"] is None and k0["preprocessor_pca_explained_variance_ratio"] is None and k0["preprocessor_interaction_pca_k"] == 0
    assert (P.full_design_dim(64, 12), P.full_design_dim(64, 12, 20), P.full_design_dim(5, 3, 99), P.full_design_dim(5, 3, 4)) == (844, 96, 23, 12)
    with pytest.raises(NotImplementedError, match="InteractionProbe"):
        P.design_dim("full", 64, 12)


def test_the_model_about_the_pivot_is_the_model():
    """beta, u, v, omega folded about the pivot give the predictions of (W, b) through the preprocessor."""
    f = _fit("e")
    g, r = f["g"], f["r"]
    pivot, beta, u, v, omega = (t.numpy() for t in g.pivoted_model())
    assert all(t.dtype == np.float32 for t in (pivot, beta, u, v, omega)) and omega.shape == (7, 16, 4) and u.shape == (7, 16) and v.shape == (7, 4)
    m = r["m"]
    pred, bound = FC.pivoted_pred(r["zt"][m], r["zp"][m], pivot, beta, u, v, omega)
    own = dict(mean=g.mean_.numpy(), std=g.std_.numpy(), comp=g.pca_components_.numpy())
    want = FC.predict64(own, f["W"], f["b"], r["zt"][m], r["zp"][m])
    assert np.all(np.abs(pred - want) <= 2 * bound)                              # the rounding of the folded model and of x', p' to float32


def test_refusals():
    y, m = torch.zeros(1, 5, 2, 4, 4), torch.ones(1, 4, 4, dtype=torch.bool)
    zt, zp = torch.zeros(1, 8, 4, 4), torch.zeros(1, 4, 2, 4, 4)
    with pytest.raises(ValueError, match="768"):
        InteractionProbe().partial_fit((torch.zeros(1, 64, 4, 4), torch.zeros(1, 13, 2, 4, 4)), y, m)
    with pytest.raises(ValueError, match="16"):
        InteractionProbe().partial_fit((torch.zeros(1, 8, 4, 4), torch.zeros(1, 17, 2, 4, 4)), y, m)
    with pytest.raises(ValueError, match="64"):
        InteractionProbe().partial_fit((torch.zeros(1, 65, 4, 4), torch.zeros(1, 2, 2, 4, 4)), y, m)
    with pytest.raises(ValueError, match="both sources"):
        InteractionProbe().partial_fit(zt, y, m)
    with pytest.raises(ValueError, match="4-D or 5-D"):
        InteractionProbe().partial_fit((zt[0], zp), y, m)
    with pytest.raises(ValueError, match="interaction_pca_k"):
        InteractionProbe(interaction_pca_k=-1)
    with pytest.raises(ValueError, match="768"):
        InteractionProbe.from_moments(np.zeros((80, 80)), np.zeros((80, 832)), np.zeros((832, 832)), 1, np.zeros(79), 64, 13)
    with pytest.raises(ValueError, match="expected S"):
        InteractionProbe.from_moments(np.zeros((16, 16)), np.zeros((16, 15)), np.zeros((15, 16)), 1, np.zeros(15), 8, 4)
    with pytest.raises(_lib.FrlHipError, match="GPU"):                           # no CPU fallback
        InteractionProbe().partial_fit((zt, zp), y, m)
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        _fit("a")["g"].predict((torch.zeros(1, 5, 4, 4), torch.zeros(1, 3, 2, 4, 4)))
    with pytest.raises(RuntimeError, match="No valid observations"):
        InteractionProbe().solve()
