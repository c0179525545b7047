"""CPU tests of the linear-probe block: the float64 restatement of tests/probe_cases.py against what the reference's own functions gave
(tests/golden/probe_*.npz), and the pivoted, centred algebra of frl_hip.probe.RidgeProbe.from_moments(...).solve() against the
reference's normal equations.  No GPU.

Tolerances.  The restatement and the reference solve the same float64 system: they differ by the conditioning of A + reg,
cond 2^-52 16 relative to the largest coefficient, plus the rounding of the stored W and b to float32 (u).  The reference's metrics are
float32 throughout (the einsum, err * err and the sums): its prediction carries (D + 2) u (|b| + sum |x_d| |W_d|), a pairwise float32
sum over n terms (ceil(log2 n) + 3) u of sum |terms|; SSE, SST and what follows from them are bounded from those.  For case f
(features + 1000) that prediction error is about 1e-3 and reorders pairs, so the reference's own rho^2 is 2.5e-5 away from the float64
value: rho^2 is asserted at 1e-6 for cases a and g only and printed for f.  The evaluated split leaves out pixels whose predictions
nearly tie (eval_mask of the fixture), so that on a and g no float32 prediction error reorders a pair.
"""
import dataclasses
import os

import numpy as np
import pytest
import torch

import probe_cases as PC
from frl_hip import probe as P
from frl_hip.probe import RidgeProbe

U = PC.U32
EPS = 2.0 ** -52


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"probe_{name}.npz"))


_IN = {}


def _inputs(case):
    if case not in _IN:
        inp = PC.make_inputs(case)
        _IN[case] = (inp,) + PC.flatten(inp)
    return _IN[case]


@pytest.mark.parametrize("case", PC.GOLDEN_REFERENCE_CASES)
def test_restatement_reproduces_reference_fit_and_metrics(golden_dir, case):
    fx = _fx(golden_dir, case)
    inp, X, Y, m = _inputs(case)
    assert PC.checksum(inp) == int(fx["checksum"])
    W, b, cond = PC.ridge_fit(X, Y, m)
    scale = max(np.abs(W).max(), np.abs(b).max())
    tol = cond * EPS * 16 * scale
    print(f"case {case}: cond {cond:.3e}, W {np.abs(W - fx['W']).max():.2e}, b {np.abs(b - fx['b']).max():.2e} (solve tolerance {tol:.2e})")
    assert np.all(np.abs(W - fx["W"]) <= tol + U * np.abs(W))
    assert np.all(np.abs(b - fx["b"]) <= tol + U * np.abs(b))

    # the evaluated split: the fitted pixels without near-ties of the prediction (make_probe_golden.py)
    names = PC.TARGET_METRICS
    m = fx["eval_mask"].reshape(-1)
    pred = X.astype(np.float64) @ fx["W"].astype(np.float64) + fx["b"].astype(np.float64)
    if case != "f":
        assert np.array_equal(m, PC.separated_mask(pred, PC.flatten(inp)[2], float(fx["separation"])))
    s = PC.eval_sums(X, Y, m, fx["W"], fx["b"])
    got = PC.metrics(X, Y, m, fx["W"], fx["b"], names)
    n = s["n"]
    assert n == int(fx["n_pixels"]) == got["n_pixels"]
    rb = PC.reference_metric_bounds(X, Y, m, fx["W"], fx["b"])
    mse = np.asarray([got["mse_per_metric"][k] for k in names])
    r2 = np.asarray([got["r2_per_metric"][k] for k in names])
    print(f"   mse {np.abs(mse - fx['mse']).max():.2e} (bound {rb['mse'].max():.2e}), r2 {np.abs(r2 - fx['r2']).max():.2e} ({rb['r2'].max():.2e})")
    assert np.all(np.abs(mse - fx["mse"]) <= rb["mse"]) and np.all(np.abs(r2 - fx["r2"]) <= rb["r2"])
    assert abs(got["mse_total"] - float(fx["mse_total"])) <= rb["mse"].mean()
    assert abs(got["r2_total"] - float(fx["r2_total"])) <= rb["r2"].mean()
    rho = np.asarray([got["spearman_rho2_per_metric"][k] for k in names])
    print(f"   rho2 {np.abs(rho - fx['rho2']).max():.2e}")
    if case != "f":
        assert np.all(np.abs(rho - fx["rho2"]) <= 1e-6) and abs(got["spearman_rho2_total"] - float(fx["rho2_total"])) <= 1e-6


def _pivots(X, Y, m):
    c = np.concatenate([X[m].astype(np.float64).mean(0), Y[m].astype(np.float64).mean(0)])
    rng = np.random.default_rng(0)
    return {"mean": c.astype(np.float32), "zero": np.zeros_like(c, np.float32), "off": (c + rng.normal(0.0, 0.5, c.shape)).astype(np.float32)}


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
@pytest.mark.parametrize("pivot", ["mean", "zero", "off"])
def test_pivoted_algebra_gives_the_reference_solution(case, pivot):
    """Exact float64 moments in, the reference's (W, b) out, for any pivot."""
    _, X, Y, m = _inputs(case)
    W, b, cond = PC.ridge_fit(X, Y, m)
    p = _pivots(X, Y, m)[pivot]
    g = RidgeProbe.from_moments(PC.exact_moments(X, Y, m, p), int(m.sum()), p, Y.shape[1], ridge_lambda=PC.RIDGE)
    W32, b32 = g.solve()
    tol = cond * EPS * 16 * max(np.abs(W).max(), np.abs(b).max())
    ew, eb = np.abs(g.coef64_.numpy() - W).max(), np.abs(g.intercept64_.numpy() - b).max()
    print(f"case {case} pivot {pivot}: cond {cond:.3e}, W {ew:.2e}, b {eb:.2e} (tolerance {tol:.2e})")
    assert ew <= tol and eb <= tol
    assert W32.dtype == torch.float32 and b32.dtype == torch.float32 and tuple(W32.shape) == W.shape and tuple(b32.shape) == b.shape
    assert g.n_obs_ == int(m.sum())


@pytest.mark.parametrize("case", ["b", "c", "f"])
def test_standardised_algebra_gives_the_two_pass_solution(case):
    """standardize=True: the system of the reference's pass 2 on columns standardised in float64 by its float32 mean and std."""
    _, X, Y, m = _inputs(case)
    mean, std = PC.feature_statistics(X, m)
    p = _pivots(X, Y, m)["mean"]
    g = RidgeProbe.from_moments(PC.exact_moments(X, Y, m, p), int(m.sum()), p, Y.shape[1], ridge_lambda=PC.RIDGE, standardize=True)
    g.solve()
    # the statistics come out of centred moments: they may differ from the two-pass float32 values in the last bit
    assert np.all(np.abs(g.mean_.numpy() - mean) <= 2 * U * np.abs(mean)) and np.all(np.abs(g.std_.numpy() - std) <= 2 * U * std)
    Z = (X[m].astype(np.float64) - g.mean_.numpy().astype(np.float64)) / g.std_.numpy().astype(np.float64)
    W, b, cond = PC.ridge_from_normal(*PC.normal_equations(Z, Y[m]), PC.RIDGE)
    tol = cond * EPS * 16 * max(np.abs(W).max(), np.abs(b).max())
    ew, eb = np.abs(g.coef64_.numpy() - W).max(), np.abs(g.intercept64_.numpy() - b).max()
    print(f"case {case}: cond {cond:.3e}, W {ew:.2e}, b {eb:.2e} (tolerance {tol:.2e})")
    assert ew <= tol and eb <= tol


@pytest.mark.parametrize("case", PC.PHASE_CASES)
def test_standardised_solution_against_the_reference_transform(golden_dir, case):
    """Against the golden built with the reference's ProbePreprocessor.transform (float32 columns): inside the rounding bound."""
    fx = _fx(golden_dir, case)
    inp, X, Y, m = _inputs(case)
    assert PC.checksum(inp) == int(fx["checksum"]) and int(m.sum()) == int(fx["n_obs"])
    p = _pivots(X, Y, m)["mean"]
    S = PC.exact_moments(X, Y, m, p)
    g = RidgeProbe.from_moments(S, int(m.sum()), p, Y.shape[1], ridge_lambda=PC.RIDGE, standardize=True)
    W, b = g.solve()
    assert np.all(np.abs(g.mean_.numpy() - fx["mean"]) <= 2 * U * np.abs(fx["mean"])) and np.all(np.abs(g.std_.numpy() - fx["std"]) <= 2 * U * fx["std"])
    dW, db = PC.solve_bounds(S, np.zeros_like(S), int(m.sum()), p, X.shape[1], PC.RIDGE, std=fx["std"])
    ew, eb = np.abs(W.numpy() - fx["W"]), np.abs(b.numpy() - fx["b"])
    print(f"case {case}: W {ew.max():.2e} (bound {dW.max():.2e}), b {eb.max():.2e} ({db.max():.2e})")
    assert np.all(ew <= dW + 2 * U * np.abs(fx["W"])) and np.all(eb <= db + 2 * U * np.abs(fx["b"]))


def test_halo_mask_and_spearman_match_the_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "probe_misc.npz"))
    keys = [k for k in fx.files if k.startswith("halo_")]
    assert len(keys) >= 6
    for k in keys:
        h, w, halo = (int(v) for v in k.split("_")[1:])
        assert np.array_equal(P.halo_mask(h, w, halo).numpy(), fx[k]) and np.array_equal(PC.halo_mask(h, w, halo), fx[k])
    for seed, n in enumerate((1, 2, 501)):
        rng = np.random.default_rng(100 + seed)
        t = rng.normal(size=n).astype(np.float32)
        p = (t + rng.normal(0.0, 0.7, size=n)).astype(np.float32)
        want = float(fx[f"rho2_{seed}"])
        assert abs(P.spearman_rho2(torch.from_numpy(p), torch.from_numpy(t)) - want) <= 1e-12
        assert abs(PC.spearman_rho2(p, t) - want) <= 1e-12


def test_designs_and_limits():
    assert P.TARGET_METRICS == PC.TARGET_METRICS
    assert [f.name for f in dataclasses.fields(P.ProbeMetrics)] == ["mse_per_metric", "r2_per_metric", "spearman_rho2_per_metric", "mse_total",
                                                                    "r2_total", "spearman_rho2_total", "n_pixels"]
    assert (P.design_dim("additive", 64, 12), P.design_dim("type-only", 64, 12), P.design_dim("phase-only", 64, 12)) == (76, 64, 12)
    zt, zp = torch.zeros(1, 64, 4, 4), torch.zeros(1, 12, 3, 4, 4)
    assert P.design_features("additive", zt, zp) == (zt, zp) and P.design_features("type-only", zt, zp) is zt
    assert P.design_features("phase-only", zt, zp) is zp
    with pytest.raises(NotImplementedError):
        P.design_dim("full", 64, 12)
    with pytest.raises(NotImplementedError):
        P.fit_phase_probe([], None, "cpu", 1e-3, design="full")
    with pytest.raises(ValueError):
        P.design_dim("quadratic", 64, 12)
    # D > 128 and Cy > 16 are refused before anything reaches a device
    y, m = torch.zeros(1, 5, 4, 4), torch.ones(1, 4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="128"):
        RidgeProbe().partial_fit(torch.zeros(1, 129, 4, 4), y, m)
    with pytest.raises(ValueError, match="128"):
        RidgeProbe().partial_fit((torch.zeros(1, 120, 4, 4), torch.zeros(1, 9, 2, 4, 4)), y, m)
    with pytest.raises(ValueError, match="16"):
        RidgeProbe.from_moments(np.zeros((30, 30)), 1, np.zeros(29), 17)
    with pytest.raises(ValueError, match="128"):
        RidgeProbe.from_moments(np.zeros((131, 131)), 1, np.zeros(130), 1)
    # no CPU fallback
    with pytest.raises(Exception, match="GPU"):
        RidgeProbe().partial_fit(torch.zeros(1, 8, 4, 4), y, m)


def test_no_observation_raises_the_reference_message():
    g = RidgeProbe.from_moments(np.zeros((8, 8)), 0, np.zeros(7), 2)
    with pytest.raises(RuntimeError, match="No valid pixels found in training data; cannot fit probe."):
        g.solve()
    with pytest.raises(RuntimeError, match="No valid pixels found in training data; cannot fit probe."):
        RidgeProbe().solve()


def test_pivoted_model_predicts_what_the_model_predicts():
    """pred = bc + (x - p) Wc is the model, plain and standardised, whatever the pivot."""
    _, X, Y, m = _inputs("c")
    for std in (False, True):
        p = _pivots(X, Y, m)["off"]
        g = RidgeProbe.from_moments(PC.exact_moments(X, Y, m, p), int(m.sum()), p, Y.shape[1], ridge_lambda=PC.RIDGE, standardize=std)
        W, b = g.solve()
        pv, wc, bc = g.pivoted_model()
        assert np.array_equal(pv.numpy(), p)
        x = X[m].astype(np.float64)
        z = (x - g.mean_.numpy().astype(np.float64)) / g.std_.numpy().astype(np.float64) if std else x
        want = z @ W.numpy().astype(np.float64) + b.numpy().astype(np.float64)
        got = PC.pivoted_pred(X[m], pv.numpy(), wc.numpy(), bc.numpy())
        bound = 2 * U * (np.abs(bc.numpy().astype(np.float64)) + np.abs(x - p[:X.shape[1]].astype(np.float64)) @ np.abs(wc.numpy().astype(np.float64)))
        assert np.all(np.abs(got - want) <= bound)
