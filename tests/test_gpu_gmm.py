"""GPU tests of the GMM block (csrc/gmm.hip, frl_hip/clustering.py) against the float64 restatement of tests/gmm_cases.py, sklearn's
results and the reference's phase summary (tests/golden/gmm_*.npz).

Tolerances, from the operation count (u = 2^-24; gmm_cases.step_bounds computes them from the float64 quantities of each case, never
from the kernel's output):

lp.  lp[n][k] = a_k + sum_d (A y^2 + B y) is a chain of 2 D fused multiply-adds on the exact-float32 MFMA plus one add; a_k is formed in
double and rounded once.  Each rounding is at most u times the partial sum, which is at most M_nk = |a_k| + sum_d (|A| y^2 + |B y|).
Roundings are independent and uniform (standard deviation u |partial| / sqrt 3) and the partial sums grow linearly (rms M / sqrt 3), so
the error of one lp has standard deviation d_lp = u M sqrt(2 D + 3) / 3, with M the rms of M_nk over the pairs that carry
responsibility (r > 1e-7).  For one row alone (score_samples, labels) the bound is 6 u sqrt(2 D + 3) max M_nk (`lp_max`).

Responsibilities.  d r_k = r_k (1 - r_k) d lp_k - r_k sum_{j != k} r_j d lp_j: both parts are at most r_k (1 - r_k) in size, so
r_k changes by at most sqrt 2 r_k (1 - r_k) d_lp; exp, log and the division add 3 u relative.

Moments.  mu_k - p = sum w r y / nk: the errors of r are independent over rows, so the mean moves by
sqrt 2 d_lp sqrt(sum_n (w r (1 - r) |x - mu_k|)^2) / nk.  The sums over rows are float32 chains inside a workgroup (a row with r = 0 adds
exactly nothing) and double beyond it: with n_k rows that count, a relative error u sqrt(n_k) / 3 of sum w r |y| / nk.  Here mu_k is the
mean the step gives, not the one it started from.  The variance is S2 / nk - m^2 (m = mu_k - p): the same two terms with
(x - mu_k)^2 + var_k and sum w r y^2 / nk, plus 2 |m| times the error of m, all over the largest variance the step gives; the weights
with sum w r.  The outputs are rounded once (2 u |mu|, 4 u, 2 u).  Every term carries the factor 6: the largest of ~10^4 outputs stays within six standard deviations.
The bound covers the worst split, workgroups = 1; the same bound holds for every `workgroups`.

Lower bound.  The mean of lse over rows: u (max |a_k| + max |lse|) for the rounding of a_k (common to all rows of a component) and of
lse itself, plus 6 d_lp / sqrt N.

Whole fits.  n_iter must equal sklearn's (the cases stop clear of tol on both sides, test_cpu_gmm.py); the EM map does not expand
errors near its fixed point, so the error after n iterations is at most n times the one-step bound (the larger of the bounds at the
initial and the final parameters).  Case i adds what rounding x + 1000 to float32 does: half an ulp of 1000, 3.05e-5, on a mean,
2 sqrt(var) 3.05e-5 on a variance.

BIC = -2 N mean lse + const.  Two runs that apply the same stopping rule end at most one iteration apart, where the bound moves by less
than tol, so |BIC - sklearn's| <= 2 N (tol + 4 u max |lse|).

Hard assignments.  A difference of two squared distances carries at most 4 (2 D + 4) u M_n (gmm_cases.hard_gap_bound); rows whose
float64 gap is within it are excluded (at most 1 %; test_cpu_gmm.py shows the restatement excludes under 0.5 %).

Phase summary.  The reference sums T float32 terms: (T + 2) u max |z| on a mean, (2 T + 4) u max z^2 on the variance.
"""
import os

import numpy as np
import pytest
import torch

import gmm_cases as G
from frl_hip import clustering, ops
from frl_hip.clustering import DiagGMM, bic_sweep, fit_landscape_taxonomy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = G.U32


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"gmm_{name}.npz"))


def _t(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV, dtype).contiguous()


_REF = {}


def _ref(case):
    """Inputs, the float64 step from the fixture's init and its bounds: computed once per case."""
    if case not in _REF:
        inp = G.make_inputs(case)
        a = (inp["weights_init"], inp["means_init"], inp["variances_init"])
        _REF[case] = dict(inp=inp, step=G.em_step(inp["X"], inp["w"], *a), bounds=G.step_bounds(inp["X"], inp["w"], *a))
    return _REF[case]


_FIT64 = {}


def _fit64(case):
    if case not in _FIT64:
        inp = _ref(case)["inp"]
        _FIT64[case] = G.fit(inp["X"], inp["w"], inp["weights_init"], inp["means_init"], inp["variances_init"])
    return _FIT64[case]


def _gpu_step(inp, workgroups):
    X, w = _t(inp["X"]), _t(inp["w"])
    n, d = X.shape
    k = len(inp["weights_init"])
    ws = ops.gmm_workspace(n, d, k, DEV, workgroups)
    pivot = ops.gmm_pivot(X, ws)
    pi, mu, var = _t(inp["weights_init"]), _t(inp["means_init"]), _t(inp["variances_init"])
    mc = (mu.double() - pivot.double()).float()
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    hist = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, workgroups=workgroups)
    ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, hist, G.REG_COVAR, G.TOL, ops.GMM_M_EM, workgroups)
    assert state.tolist() == [1, 0]
    return pi.cpu().numpy(), mu.cpu().numpy(), var.cpu().numpy(), float(hist[0])


def _check_params(got, want, b, scale=1.0, what=""):
    pi, mu, var = got
    pi64, mu64, var64 = want
    e_mu, e_var, e_pi = np.abs(mu - mu64).max(), np.abs(var - var64).max() / var64.max(), np.abs(pi - pi64).max()
    print(f"{what}: means {e_mu:.2e} (bound {scale * b['mu']:.2e}), variances {e_var:.2e} ({scale * b['var_rel']:.2e}), "
          f"weights {e_pi:.2e} ({scale * b['pi']:.2e})")
    assert e_mu <= scale * b["mu"] and e_var <= scale * b["var_rel"] and e_pi <= scale * b["pi"]


# ---- 1. one EM step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.STEP_CASES)
def test_one_em_step(case):
    r = _ref(case)
    for wg in (1, 2, 3, 0):                                                      # 3 slabs: no multiple of the four parts of the slab sum
        got = _gpu_step(r["inp"], wg)
        again = _gpu_step(r["inp"], wg)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3], f"workgroups={wg}: two runs differ"
        _check_params(got[:3], r["step"][:3], r["bounds"], what=f"case {case} workgroups={wg}")
        print(f"   lower bound {abs(got[3] - r['step'][3]):.2e} (bound {r['bounds']['lb']:.2e})")
        assert abs(got[3] - r["step"][3]) <= r["bounds"]["lb"]


# ---- 2. whole fits -------------------------------------------------------------------------------------------------------------
_GPU_FITS = {}


def _gpu_fit(case, **kw):
    key = (case, tuple(sorted(kw.items())))
    if key not in _GPU_FITS:
        inp = _ref(case)["inp"]
        g = DiagGMM(len(inp["weights_init"]), tol=G.TOL, reg_covar=G.REG_COVAR, max_iter=kw.pop("max_iter", G.MAX_ITER),
                    weights_init=inp["weights_init"], means_init=inp["means_init"],
                    precisions_init=1.0 / inp["variances_init"].astype(np.float64), **kw)
        _GPU_FITS[key] = g.fit(_t(inp["X"]), _t(inp["w"]))
    return _GPU_FITS[key]


def _fit_bounds(case):
    inp, f = _ref(case)["inp"], _fit64(case)
    end = G.step_bounds(inp["X"], inp["w"], f["weights"], f["means"], f["covariances"])
    return {k: max(v, end[k]) for k, v in _ref(case)["bounds"].items()}


@pytest.mark.parametrize("case", G.FIT_CASES)
def test_whole_fit_equals_sklearn(golden_dir, case):
    fx, g, b = _fx(golden_dir, case), _gpu_fit(case), _fit_bounds(case)
    assert g.n_iter_ == int(fx["n_iter"]) and g.converged_ == bool(fx["converged"])
    n = g.n_iter_
    _check_params((g.weights_.cpu().numpy(), g.means_.cpu().numpy(), g.covariances_.cpu().numpy()),
                  (fx["weights"], fx["means"], fx["covariances"]), b, scale=n, what=f"fit {case} ({n} iterations)")
    assert abs(g.lower_bound_ - float(fx["lower_bound"])) <= n * b["lb"]
    assert g.lower_bounds_.shape == (G.MAX_ITER,) and np.isnan(g.lower_bounds_[n:]).all() and np.isfinite(g.lower_bounds_[:n]).all()
    assert np.allclose(g.precisions_cholesky_.cpu().numpy(), 1.0 / np.sqrt(g.covariances_.cpu().numpy()), rtol=1e-6)


def test_shifted_data_gives_shifted_means():
    """Case i is case b + 1000: the same variances, the means 1000 higher."""
    gb, gi = _gpu_fit("b"), _gpu_fit("i")
    bb, bi = _fit_bounds("b"), _fit_bounds("i")
    half_ulp = 0.5 * 2.0 ** -14                                                  # of a float32 near 1000
    n = gb.n_iter_
    assert gi.n_iter_ == n
    dm = np.abs(gi.means_.cpu().numpy().astype(np.float64) - 1000.0 - gb.means_.cpu().numpy()).max()
    vb, vi = gb.covariances_.cpu().numpy().astype(np.float64), gi.covariances_.cpu().numpy().astype(np.float64)
    dv = np.abs(vi - vb).max()
    print(f"means {dm:.2e}, variances {dv:.2e}")
    assert dm <= n * (bb["mu"] + bi["mu"]) + half_ulp
    assert dv <= n * (bb["var_rel"] + bi["var_rel"]) * vb.max() + 2 * np.sqrt(vb.max()) * half_ulp


# ---- 3. poll_every -------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_poll_every():
    fits = [_gpu_fit("c", max_iter=40, poll_every=p) for p in (1, 3, 40)]
    n = fits[0].n_iter_
    assert 1 < n < 40 and fits[0].converged_
    for g in fits[1:]:
        assert g.n_iter_ == n and g.converged_
        for a, b in ((g.weights_, fits[0].weights_), (g.means_, fits[0].means_), (g.covariances_, fits[0].covariances_)):
            assert torch.equal(a, b)
        assert np.array_equal(g.lower_bounds_, fits[0].lower_bounds_, equal_nan=True)
    assert np.isnan(fits[2].lower_bounds_[n:]).all()                              # iterations enqueued after the stop touched nothing


# ---- 4. hard mode and initialisation ------------------------------------------------------------------------------------------------
def _hard_pass(X, w, centres32, mode, reg_covar=G.REG_COVAR):
    """One hard E pass and an M pass of `mode` from centres -> (labels, pi, mu, var)."""
    n, d = X.shape
    k = len(centres32)
    ws = ops.gmm_workspace(n, d, k, DEV)
    pivot = ops.gmm_pivot(X, ws)
    pi = torch.full((k,), 1.0 / k, dtype=torch.float32, device=DEV)
    var = torch.ones(k, d, dtype=torch.float32, device=DEV)
    mu = _t(centres32)
    mc = (mu.double() - pivot.double()).float()
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    labels = ops.gmm_score(X, pivot, pi, mc, var)[1].cpu().numpy()
    ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, hard=True)
    ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, reg_covar=reg_covar, mode=mode)
    return labels, pi.cpu().numpy(), mu.cpu().numpy(), var.cpu().numpy()


def _hard_mean_bound(X, labels):
    """A mean of n_k rows about the pivot: a float32 chain of n_k terms of size <= max |y|, and one rounding of the result."""
    Y = X.astype(np.float64) - X.astype(np.float64).mean(0)
    nk = max(np.bincount(labels).max(), 1)
    return G.CONF * G.RMS * U * np.sqrt(nk) * np.abs(Y).max() + 2 * U * (np.abs(X).max() + np.abs(Y).max())


@pytest.mark.parametrize("case", G.HARD_CASES)
def test_lloyd_steps(case):
    inp = _ref(case)["inp"]
    X = _t(inp["X"])
    c = inp["X"][inp["init_rows"]].astype(np.float64)
    for step in range(3):
        c32 = c.astype(np.float32)
        want, new, gap = G.lloyd_step(inp["X"], None, c32)
        sure = gap > G.hard_gap_bound(inp["X"], c32)
        labels, _, mu, _ = _hard_pass(X, None, c32, ops.GMM_M_LLOYD)
        print(f"case {case} step {step}: {int((~sure).sum())} rows excluded, {int((labels != want).sum())} labels differ")
        assert (~sure).mean() <= 0.01
        assert np.array_equal(labels[sure], want[sure])
        if np.array_equal(labels, want):
            assert np.abs(mu - new).max() <= _hard_mean_bound(inp["X"], want)
        c = new


def test_centre_without_rows_keeps_its_value():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(300, 5)).astype(np.float32)
    c = np.stack([X[0], X[1], np.full(5, 100.0, np.float32)])
    labels, _, mu, _ = _hard_pass(_t(X), None, c, ops.GMM_M_LLOYD)
    assert labels.max() == 1
    assert np.array_equal(mu[2], c[2]) and not np.array_equal(mu[0], c[0])


@pytest.mark.parametrize("case", G.HARD_CASES)
def test_init_parameters(case):
    inp = _ref(case)["inp"]
    k = len(inp["init_rows"])
    g = DiagGMM(k, init_rows=inp["init_rows"][None], kmeans_iters=G.KMEANS_ITERS, reg_covar=G.REG_COVAR)
    pi, mu, var = (t.cpu().numpy() for t in g.init_params(_t(inp["X"])))
    pi64, mu64, var64 = G.kmeans_init(inp["X"], None, inp["init_rows"], G.KMEANS_ITERS)
    labels = G.sq_dist(inp["X"], mu64).argmin(1)
    Y = inp["X"].astype(np.float64) - inp["X"].astype(np.float64).mean(0)
    b = _hard_mean_bound(inp["X"], labels)
    b2 = G.CONF * G.RMS * U * np.sqrt(np.bincount(labels).max()) * (Y ** 2).max() + 2 * np.abs(Y).max() * b + 4 * U * var64.max()
    print(f"init {case}: means {np.abs(mu - mu64).max():.2e} ({b:.2e}), variances {np.abs(var - var64).max():.2e} ({b2:.2e})")
    assert np.abs(pi - pi64).max() <= 2 * U
    assert np.abs(mu - mu64).max() <= b and np.abs(var - var64).max() <= b2


# ---- 5. predict, score_samples, predict_proba ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SCORE_CASES)
def test_scoring(case):
    inp, f = _ref(case)["inp"], _fit64(case)
    pi, mu, var = (a.astype(np.float32) for a in (f["weights"], f["means"], f["covariances"]))
    g = DiagGMM.from_params(pi, mu, var)
    X = _t(inp["X"])
    lp, lse, resp = G.e_step(inp["X"], pi, mu, var)
    b = G.step_bounds(inp["X"], None, pi, mu, var)["lp_max"] + 4 * U * np.abs(lse).max()
    got_lse, got_lab, got_resp = g.score_samples(X).cpu().numpy(), g.predict(X).cpu().numpy(), g.predict_proba(X).cpu().numpy()
    print(f"score {case}: lse {np.abs(got_lse - lse).max():.2e} (bound {b:.2e}), resp {np.abs(got_resp - resp).max():.2e} ({2 * b + 4 * U:.2e})")
    assert np.abs(got_lse - lse).max() <= b
    assert np.abs(got_resp - resp).max() <= 2 * b + 4 * U
    assert np.abs(got_resp.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    s = np.sort(lp, 1)
    sure = (s[:, -1] - s[:, -2]) > 2 * b
    assert (~sure).mean() <= 0.01 and np.array_equal(got_lab[sure], lp.argmax(1)[sure])
    assert abs(g.score(X) - lse.mean()) <= b
    assert abs(g.bic(X) - G.bic(inp["X"], pi, mu, var)) <= 2 * len(lse) * b


# ---- 6. the BIC sweep -----------------------------------------------------------------------------------------------------------
def test_bic_sweep(golden_dir):
    fx = _fx(golden_dir, "bic")
    X, rows = G.make_bic_inputs()
    best_k, best, bics = bic_sweep(_t(X), G.BIC_K_VALUES, n_init_sweep=1, n_init_final=G.BIC_N_INIT_FINAL, init_rows=rows,
                                   kmeans_iters=G.KMEANS_ITERS)
    assert best_k == 3 == int(fx["best_k"]) and best.n_components == 3
    lse_max = max(abs(v) for v in fx["bic"]) / (2 * len(X))                      # |mean lse| <= this; rows of these blobs stay within a few times it
    tol = 2 * len(X) * (G.TOL + 4 * U * 4 * lse_max)
    for k, want in zip(fx["k_values"], fx["bic"]):
        print(f"K={k}: BIC {bics[int(k)]:.3f}, sklearn {want:.3f} (tolerance {tol:.3f})")
        assert abs(bics[int(k)] - want) <= tol
    assert abs(best.lower_bound_ - float(fx["best_lower_bound"])) <= G.TOL + 16 * U * lse_max


# ---- 7. the phase summary ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", G.PHASE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phase_summary(golden_dir, shape):
    fx = _fx(golden_dir, "phase")
    key = "x".join(map(str, shape))
    z, y = G.make_phase_inputs(shape)
    s, v = clustering.phase_summary(_t(z), _t(y))
    s, v = s.cpu().numpy(), v.cpu().numpy()
    t = shape[1]
    assert s.shape == (shape[0], 3 * shape[2]) and v.shape == (shape[0],)
    assert np.abs(s - fx["summary_" + key]).max() <= (t + 2) * U * np.abs(z).max()
    want = fx["tvar_" + key]
    assert np.array_equal(np.isnan(v), np.isnan(want)) and np.isnan(v).all() == (t == 1)
    assert np.nanmax(np.abs(v - want), initial=0.0) <= (2 * t + 4) * U * (z.astype(np.float64) ** 2).max()


# ---- 8. the taxonomy ---------------------------------------------------------------------------------------------------------------
def test_fit_landscape_taxonomy(golden_dir):
    fx = _fx(golden_dir, "taxonomy")
    z, s = G.make_taxonomy_inputs()
    out = fit_landscape_taxonomy(_t(z), _t(s), kmeans_iters=G.KMEANS_ITERS, **G.TAXONOMY)
    assert out["type_gmm"].n_components == 3 == int(fx["k_type"]) and set(out["bic_type"]) == set(G.TAXONOMY["k_type_values"])
    got = sorted((t["n_pixels"], t["k_phase"], t["is_dynamic"]) for t in out["taxonomy"].values())
    assert got == sorted((int(n), int(k), int(k) > 1) for n, k in zip(fx["n_pixels"], fx["k_phase"]))
    assert sorted(t["k_phase"] for t in out["taxonomy"].values()) == [1, 1, 2]
    assert all((out["phase_gmms"][k].n_components == t["k_phase"]) for k, t in out["taxonomy"].items())
