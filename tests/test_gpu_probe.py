"""GPU tests of the linear-probe block (csrc/probe.hip, frl_hip/probe.py) against the float64 restatement of tests/probe_cases.py and
what the reference's own functions gave (tests/golden/probe_*.npz).

Tolerances (u = 2^-24; probe_cases.py derives each from float64 quantities of the case, never from the kernel's output):

Moments.  Every entry of S against the float64 product of the same float32 rows v, which the test forms itself from the pivot the
kernel reports: 6 u sqrt(n) / 3 sum |v_i v_j| + 2 u |S_ij| (the chain model of test_gpu_gmm.py; n the unmasked count; it covers the
worst split, one workgroup, and is asserted for every `workgroups`).  The count is exact.

W and b.  2 |M^-1| (dB + dA |W|) elementwise with dA, dB the moment bounds carried through Sigma = S_vv - s s^T / n; for b,
sum |xbar| dW plus the bound on ybar.  For the standardised fits the reference's float32 rounding of the standardised columns is
added (probe_cases.standardise_bounds).

Evaluate.  pred within (D + 2) u (|bc| + sum |x_d - p_d| |Wc_dc|) of the float64 value of the same float32 model; SSE within
sum 2 |err| dpred + dpred^2; sum (y - q) and sum (y - q)^2 within 2 n 2^-53 of sum |terms| (double sums in two orders); n exact.
MSE and R2 against the golden add what the reference's own float32 arithmetic moves them by (probe_cases.reference_metric_bounds).
rho^2 within 1e-6 of the golden on the evaluated split, which leaves out near-ties of the prediction (eval_mask of the fixture); for
case f the reference's own rho^2 is 2.5e-5 off the float64 value (its float32 prediction of features near 1000 reorders pairs), so f is
held to the float64 value of the restatement instead.
"""
import os

import numpy as np
import pytest
import torch

import probe_cases as PC
from frl_hip import _lib, ops, probe as P
from frl_hip.probe import RidgeProbe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = PC.U32


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"probe_{name}.npz"))


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_IN = {}


def _inputs(case):
    """Inputs, their flattened float64-ready form and device tensors (channels-last): made once per case."""
    if case not in _IN:
        inp = PC.make_inputs(case)
        X, Y, m = PC.flatten(inp)

        def cl(a):                                                               # [B, T_s, H, W, C] -> [B, H, W, C] where T_s = 1 and static
            return None if a is None else _t(a[:, 0] if a.shape[1] == 1 else a)

        feats = cl(inp["A"]) if inp["Bs"] is None else (cl(inp["A"]), cl(inp["Bs"]))
        _IN[case] = dict(inp=inp, X=X, Y=Y, m=m, feats=feats, targets=cl(inp["Y"]), mask=_t(inp["M"]), halo=inp["halo"])
    return _IN[case]


def _fit(case, workgroups=0, standardize=False):
    r = _inputs(case)
    return RidgeProbe(PC.RIDGE, standardize, workgroups).partial_fit(r["feats"], r["targets"], r["mask"], halo=r["halo"], channels_last=True)


def _check_moments(g, X, Y, m, what):
    """-> (S64, bound, pivot) after asserting the count, the symmetry and every entry of S."""
    S, n, pivot = g.moments()
    S, pivot = S.numpy(), pivot.numpy().astype(np.float32)
    assert n == int(m.sum()), f"{what}: count {n}, expected {int(m.sum())}"
    assert np.array_equal(S, S.T)
    v = PC.pivoted_rows(X, Y, m, pivot)
    S64, bound = PC.moments(v)
    ratio = (np.abs(S - S64) / np.maximum(bound, 1e-300)).max()
    print(f"{what}: n {n}, moments at {ratio:.3f} of the bound")
    assert np.all(np.abs(S - S64) <= bound), f"{what}: {ratio:.3f} of the bound"
    return S64, bound, pivot


# ---- 1. moments and count ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list("abcdef"))
def test_moments_and_count(case):
    r = _inputs(case)
    for wg in (1, 3, 0):
        g = _fit(case, wg)
        _, _, pivot = _check_moments(g, r["X"], r["Y"], r["m"], f"case {case} workgroups={wg}")
        again = _fit(case, wg)
        assert torch.equal(g._S, again._S) and torch.equal(g._n, again._n) and torch.equal(g._pivot, again._pivot), f"workgroups={wg}: two runs differ"
        mean = np.concatenate([r["X"][r["m"]].astype(np.float64).mean(0), r["Y"][r["m"]].astype(np.float64).mean(0)])
        absm = np.concatenate([np.abs(r["X"][r["m"]]).astype(np.float64).mean(0), np.abs(r["Y"][r["m"]]).astype(np.float64).mean(0)])
        assert np.all(np.abs(pivot - mean) <= U * np.abs(mean) + 4 * len(r["X"]) * PC.U64 * absm)      # a double sum, rounded once


# ---- 2. W and b ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list("abcdefg"))
def test_solution(golden_dir, case):
    r = _inputs(case)
    g = _fit(case)
    S64, bound, pivot = _check_moments(g, r["X"], r["Y"], r["m"], f"case {case}")
    W, b = g.solve()
    if case in PC.GOLDEN_REFERENCE_CASES:
        fx = _fx(golden_dir, case)
        assert PC.checksum(r["inp"]) == int(fx["checksum"])
        W64, b64 = fx["W"], fx["b"]
    else:
        W64, b64, _ = PC.ridge_fit(r["X"], r["Y"], r["m"])
    dW, db = PC.solve_bounds(S64, bound, int(r["m"].sum()), pivot, r["X"].shape[1])
    ew, eb = np.abs(W.cpu().numpy() - W64), np.abs(b.cpu().numpy() - b64)
    print(f"case {case}: W {ew.max():.2e} (bound {dW.max():.2e}, at most {(ew / dW).max():.3f} of it), b {eb.max():.2e} ({db.max():.2e})")
    assert W.dtype == torch.float32 and b.dtype == torch.float32 and g.n_obs_ == int(r["m"].sum())
    assert np.all(ew <= dW) and np.all(eb <= db)


@pytest.mark.parametrize("case", PC.PHASE_CASES)
def test_standardised_solution(golden_dir, case):
    fx = _fx(golden_dir, case)
    r = _inputs(case)
    assert PC.checksum(r["inp"]) == int(fx["checksum"])
    g = _fit(case, standardize=True)
    S64, bound, pivot = _check_moments(g, r["X"], r["Y"], r["m"], f"case {case}")
    W, b = g.solve()
    assert g.n_obs_ == int(fx["n_obs"])
    mean, std = g.mean_.numpy(), g.std_.numpy()
    n = g.n_obs_
    d = r["X"].shape[1]
    dmean = bound[:d, -1] / n + 2 * U * np.abs(fx["mean"])                       # two roundings to float32 of nearly the same value
    dvar = bound[np.arange(d), np.arange(d)] / n + 2 * np.abs(S64[:d, -1]) * bound[:d, -1] / n ** 2
    dstd = dvar / (2 * fx["std"].astype(np.float64)) + 2 * U * fx["std"]
    assert np.all(np.abs(mean - fx["mean"]) <= dmean) and np.all(np.abs(std - fx["std"]) <= dstd)
    dW, db = PC.solve_bounds(S64, bound, n, pivot, d, std=fx["std"])
    dW = dW + np.abs(fx["W"]) * (dstd / fx["std"])[:, None]                      # W_std scales with std
    ew, eb = np.abs(W.numpy() - fx["W"]), np.abs(b.numpy() - fx["b"])
    print(f"case {case}: W {ew.max():.2e} (bound {dW.max():.2e}), b {eb.max():.2e} ({db.max():.2e})")
    assert np.all(ew <= dW) and np.all(eb <= db)


# ---- 3. evaluate ---------------------------------------------------------------------------------------------------------------
def _evaluate(case, W, b, pivot, eval_mask, names, golden=None):
    r = _inputs(case)
    X, Y = r["X"], r["Y"]
    b_, h, w = r["inp"]["M"].shape
    t = r["inp"]["T"]
    mm = np.ascontiguousarray(np.broadcast_to(eval_mask[:, None], (b_, t, h, w))).reshape(-1)
    g = RidgeProbe().set_model(W, b, pivot=pivot)
    g.partial_evaluate(r["feats"], r["targets"], _t(eval_mask), channels_last=True)
    pv, wc, bc = (a.numpy() for a in g.pivoted_model())
    # predictions of every pixel, masked or not
    pred = g.predict(r["feats"], channels_last=True).cpu().numpy().reshape(-1, Y.shape[1])
    assert pred.shape[0] == X.shape[0]
    want, dp = PC.pivoted_pred(X, pv, wc, bc), PC.pred_bound(X, pv, wc, bc)
    print(f"case {case}: pred at most {(np.abs(pred - want) / dp).max():.3f} of its bound")
    assert np.all(np.abs(pred - want) <= dp)
    # the sums
    E, n = g.evaluation_sums()
    assert n == int(mm.sum())
    err = np.abs(want[mm] - Y[mm].astype(np.float64))
    d_sse = (2 * err * dp[mm] + dp[mm] ** 2).sum(0)
    yq = Y[mm].astype(np.float64) - pv[X.shape[1]:].astype(np.float64)
    sse64 = ((want[mm] - Y[mm].astype(np.float64)) ** 2).sum(0)
    dsum = 2 * max(n, 1) * PC.U64
    print(f"   SSE {np.abs(E[:, 0] - sse64).max():.2e} (bound {d_sse.max():.2e})")
    assert np.all(np.abs(E[:, 0] - sse64) <= d_sse + dsum * sse64)
    assert np.all(np.abs(E[:, 1] - yq.sum(0)) <= dsum * np.abs(yq).sum(0)) and np.all(np.abs(E[:, 2] - (yq * yq).sum(0)) <= dsum * (yq * yq).sum(0))
    # without the ranks no prediction is written and empty tiles are skipped: the same sums, bit for bit
    g2 = RidgeProbe().set_model(W, b, pivot=pivot)
    g2.partial_evaluate(r["feats"], r["targets"], _t(eval_mask), channels_last=True, rank=False)
    E2, n2 = g2.evaluation_sums()
    assert n2 == n and np.array_equal(E, E2)
    # metrics
    mt = g.metrics(names)
    ref = PC.metrics(X, Y, mm, W, b, names)
    rb = PC.reference_metric_bounds(X, Y, mm, W, b)
    own_mse = (d_sse + dsum * sse64) / n
    d_sst = dsum * ((yq * yq).sum(0) + 2 * np.abs(yq.sum(0)) * np.abs(yq).sum(0) / n)
    own_r2 = own_mse * n / rb["sst"] + sse64 * d_sst / rb["sst"] ** 2
    mse = np.asarray([mt.mse_per_metric[k] for k in names])
    r2 = np.asarray([mt.r2_per_metric[k] for k in names])
    rho = np.asarray([mt.spearman_rho2_per_metric[k] for k in names])
    assert mt.n_pixels == n
    want_mse = np.asarray([ref["mse_per_metric"][k] for k in names])
    want_r2 = np.asarray([ref["r2_per_metric"][k] for k in names])
    want_rho = np.asarray([ref["spearman_rho2_per_metric"][k] for k in names])
    assert np.all(np.abs(mse - want_mse) <= own_mse) and np.all(np.abs(r2 - want_r2) <= own_r2)
    print(f"   rho2 against float64 {np.abs(rho - want_rho).max():.2e}")
    assert np.all(np.abs(rho - want_rho) <= 1e-6)
    if golden is not None:
        assert n == int(golden["n_pixels"])
        assert np.all(np.abs(mse - golden["mse"]) <= own_mse + rb["mse"]) and np.all(np.abs(r2 - golden["r2"]) <= own_r2 + rb["r2"])
        assert abs(mt.mse_total - float(golden["mse_total"])) <= (own_mse + rb["mse"]).mean()
        assert abs(mt.r2_total - float(golden["r2_total"])) <= (own_r2 + rb["r2"]).mean()
        print(f"   rho2 against the golden {np.abs(rho - golden['rho2']).max():.2e}")
        if case != "f":
            assert np.all(np.abs(rho - golden["rho2"]) <= 1e-6) and abs(mt.spearman_rho2_total - float(golden["rho2_total"])) <= 1e-6


@pytest.mark.parametrize("case", PC.GOLDEN_REFERENCE_CASES)
def test_evaluate_against_golden(golden_dir, case):
    fx = _fx(golden_dir, case)
    pivot = _fit(case).moments()[2]
    _evaluate(case, fx["W"], fx["b"], pivot, fx["eval_mask"], PC.TARGET_METRICS, fx)


@pytest.mark.parametrize("case", ["b", "c", "d", "e"])
def test_evaluate_other_shapes(case):
    """Time steps, two sources with a broadcast one, the limits, masked samples and tiles: against the restatement."""
    r = _inputs(case)
    W, b, _ = PC.ridge_fit(r["X"], r["Y"], r["m"])
    W, b = W.astype(np.float32), b.astype(np.float32)
    pivot = _fit(case).moments()[2]
    b_, h, w = r["inp"]["M"].shape
    mask = r["inp"]["M"] & PC.halo_mask(h, w, r["halo"])[None] if r["halo"] else r["inp"]["M"]
    pred = r["X"].astype(np.float64) @ W.astype(np.float64) + b.astype(np.float64)
    sep = 8.0 * PC.pred_bound(r["X"], pivot.numpy(), W, b).max()
    t = r["inp"]["T"]
    keep = PC.separated_mask(pred, r["m"], sep).reshape(b_, t, h, w).all(1) & mask          # a pixel stays when all its timesteps do
    _evaluate(case, W, b, pivot, keep, [f"y{i}" for i in range(r["Y"].shape[1])])


# ---- 4. empty calls, one observation ---------------------------------------------------------------------------------------------
def test_empty_calls_and_one_observation():
    r = _inputs("e")
    none = torch.zeros_like(r["mask"])
    g = RidgeProbe(PC.RIDGE).partial_fit(r["feats"], r["targets"], none, channels_last=True)
    with pytest.raises(RuntimeError, match="No valid pixels found in training data; cannot fit probe."):
        g.solve()
    assert int(g._n.item()) == 0 and not g._S.any()
    # the pivot comes from the first call that has a valid pixel
    g.partial_fit(r["feats"], r["targets"], r["mask"], channels_last=True)
    _check_moments(g, r["X"], r["Y"], r["m"], "case e after an empty call")
    S0, n0 = g._S.clone(), g._n.clone()
    g.partial_fit(r["feats"], r["targets"], none, channels_last=True)
    assert torch.equal(g._S, S0) and torch.equal(g._n, n0), "an empty call changed the state"
    # one more observation: the last pixel of the last sample at every timestep shares it, so T of them
    one = torch.zeros_like(r["mask"])
    one[2, -1, -1] = True
    g.partial_fit(r["feats"], r["targets"], one, channels_last=True)
    m1 = np.zeros_like(r["inp"]["M"])
    m1[2, -1, -1] = True
    m1 = np.ascontiguousarray(np.broadcast_to(m1[:, None], (3, r["inp"]["T"], 23, 23))).reshape(-1)
    rows = np.concatenate([np.flatnonzero(r["m"]), np.flatnonzero(m1)])
    S, n, pivot = g.moments()
    v = PC.pivoted_rows(r["X"][rows], r["Y"][rows], np.ones(len(rows), bool), pivot.numpy().astype(np.float32))
    S64, bound = PC.moments(v)
    assert n == len(rows) and np.all(np.abs(S.numpy() - S64) <= bound)
    # exactly one valid observation in all: a static probe
    a = _inputs("a")
    one = torch.zeros_like(a["mask"])
    one[1, 22, 22] = True
    g1 = RidgeProbe(PC.RIDGE).partial_fit(a["feats"], a["targets"], one, channels_last=True)
    S, n, pivot = g1.moments()
    c = S.shape[0] - 1
    want = np.zeros((c + 1, c + 1))
    want[c, c] = 1.0
    assert n == 1 and np.array_equal(S.numpy(), want)                            # the pivot is the row itself
    assert np.array_equal(pivot.numpy()[:64].astype(np.float32), a["inp"]["A"][1, 0, 22, 22])
    W, b = g1.solve()
    assert not W.any() and np.array_equal(b.numpy(), a["inp"]["Y"][1, 0, 22, 22])


# ---- 5. streaming ----------------------------------------------------------------------------------------------------------------
def test_streaming_and_workgroups():
    r = _inputs("g")
    X, Y, m = r["X"], r["Y"], r["m"]
    whole = _fit("g")
    parts = RidgeProbe(PC.RIDGE)
    for i in range(3):
        parts.partial_fit(r["feats"][i:i + 1], r["targets"][i:i + 1], r["mask"][i:i + 1], channels_last=True)
    Sw, bw, pw = _check_moments(whole, X, Y, m, "one call")
    Sp, bp, pp = _check_moments(parts, X, Y, m, "three calls")
    n = int(m.sum())
    Ww, bw_ = whole.solve()
    Wp, bp_ = parts.solve()
    dWw, dbw = PC.solve_bounds(Sw, bw, n, pw, 64)
    dWp, dbp = PC.solve_bounds(Sp, bp, n, pp, 64)
    assert np.all(np.abs(Ww.numpy() - Wp.numpy()) <= dWw + dWp) and np.all(np.abs(bw_.numpy() - bp_.numpy()) <= dbw + dbp)
    # the pivot of the streamed state is the one of its first call
    first = RidgeProbe(PC.RIDGE).partial_fit(r["feats"][:1], r["targets"][:1], r["mask"][:1], channels_last=True)
    assert torch.equal(first._pivot, parts._pivot) and not torch.equal(whole._pivot, parts._pivot)
    for wg in (1, 3, 0):
        a, b = _fit("g", wg), _fit("g", wg)
        _check_moments(a, X, Y, m, f"workgroups={wg}")
        assert torch.equal(a._S, b._S) and torch.equal(a._n, b._n)


# ---- 6. layouts ------------------------------------------------------------------------------------------------------------------
def test_channels_first_view_is_used_in_place_and_gives_the_same_bits():
    r = _inputs("c")
    zt, zp = r["feats"]                                                          # [B, H, W, 64], [B, T, H, W, 12]
    y, m = r["targets"], r["mask"]
    zt_cf, zp_cf, y_cf = zt.permute(0, 3, 1, 2), zp.permute(0, 4, 1, 2, 3), y.permute(0, 4, 1, 2, 3)   # the reference's shapes, as views
    assert P._rows(zt_cf, False, "features")[0].data_ptr() == zt.data_ptr() and P._rows(zp_cf, False, "features")[0].data_ptr() == zp.data_ptr()
    last = RidgeProbe(PC.RIDGE).partial_fit((zt, zp), y, m, halo=4, channels_last=True)
    view = RidgeProbe(PC.RIDGE).partial_fit((zt_cf, zp_cf), y_cf, m, halo=4)
    copy = RidgeProbe(PC.RIDGE).partial_fit((zt_cf.contiguous(), zp_cf.contiguous()), y_cf.contiguous(), m, halo=4)
    for other in (view, copy):
        assert torch.equal(last._S, other._S) and torch.equal(last._n, other._n) and torch.equal(last._pivot, other._pivot)
    assert P._rows(zt_cf.contiguous(), False, "features")[0].data_ptr() != zt.data_ptr()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_abi_refuses_what_it_cannot_run():
    lib = _lib.load()
    x = torch.zeros(4096, dtype=torch.float32, device=DEV)
    m = torch.ones(64, dtype=torch.uint8, device=DEV)
    S = torch.zeros(146 * 146, dtype=torch.float64, device=DEV)
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = ops.probe_workspace(128, 16, DEV)
    p = lambda t: t.data_ptr()                                                   # noqa: E731

    def acc(da, db, cy, ta, tb, ty, b, t, pp):
        return lib.frl_probe_accumulate(p(x), ta, da, p(x) if db else None, tb, db, p(x), ty, cy, p(m), b, t, pp, p(x), 0, p(S), p(n), p(ws),
                                        ws.numel(), None)

    assert acc(8, 0, 2, 1, 1, 1, 1, 1, 4) == 0
    torch.cuda.synchronize()
    for bad in ((129, 0, 1, 1, 1, 1, 1, 1, 4), (120, 9, 1, 1, 1, 1, 1, 1, 4), (8, 0, 17, 1, 1, 1, 1, 1, 4), (8, 0, 0, 1, 1, 1, 1, 1, 4),
                (8, 0, 2, 2, 1, 1, 1, 3, 4), (8, 0, 2, 1, 1, 2, 1, 3, 4), (8, 4, 2, 1, 2, 1, 1, 3, 4), (8, 0, 2, 1, 1, 1, 1 << 12, 1 << 10, 1 << 9)):
        assert acc(*bad) == -2, bad
    assert lib.frl_probe_accumulate(p(x), 1, 8, None, 1, 0, p(x), 1, 2, p(m), 1, 1, 4, p(x), 0, p(S), p(n), p(ws), 16, None) == -4
    assert lib.frl_probe_workspace_bytes(129, 1, 0) == 0 and lib.frl_probe_workspace_bytes(64, 17, 0) == 0
    with pytest.raises(ValueError):
        ops.probe_workspace(129, 5, DEV)


# ---- 8. the reference's entry points ---------------------------------------------------------------------------------------------
class _Views:
    """The model of the helpers' tests: z_type and z_phase are channels-first views of channels-last latents, as this project's
    models return them."""

    def __init__(self, z_phase=None):
        self.z_phase = z_phase

    def __call__(self, ximg):
        return ximg

    def forward_phase(self, xphase, z_type):
        return self.z_phase


def test_helpers_with_the_reference_signatures(golden_dir):
    fx, r = _fx(golden_dir, "a"), _inputs("a")
    ximg, yimg = r["feats"].permute(0, 3, 1, 2), r["targets"].permute(0, 3, 1, 2)
    W, b = P.fit_closed_form_ridge([(ximg, yimg, r["mask"])], _Views(), DEV, ridge_lambda=PC.RIDGE)
    g = _fit("a")
    W0, b0 = g.solve()
    assert torch.equal(W, W0) and torch.equal(b, b0)
    mt = P.evaluate_probe([(ximg, yimg, _t(fx["eval_mask"]))], _Views(), fx["W"], fx["b"], DEV)
    assert mt.n_pixels == int(fx["n_pixels"]) and list(mt.mse_per_metric) == PC.TARGET_METRICS
    rb = PC.reference_metric_bounds(r["X"], r["Y"], fx["eval_mask"].reshape(-1), fx["W"], fx["b"])
    assert abs(mt.mse_total - float(fx["mse_total"])) <= 2 * rb["mse"].mean() and abs(mt.spearman_rho2_total - float(fx["rho2_total"])) <= 1e-6
    empty = P.evaluate_probe([(ximg, yimg, torch.zeros_like(r["mask"]))], _Views(), fx["W"], fx["b"], DEV)
    assert empty.n_pixels == 0 and empty.mse_total == 0.0 and empty.r2_total == 0.0 and empty.spearman_rho2_total == 0.0
    assert P.fit_closed_form_ridge([(ximg, yimg, r["mask"])] * 3, _Views(), DEV, PC.RIDGE, max_batches_train=1)[0].equal(W)
    with pytest.raises(RuntimeError, match="No valid pixels"):
        P.fit_closed_form_ridge([(ximg, yimg, torch.zeros_like(r["mask"]))], _Views(), DEV)

    fc, c = _fx(golden_dir, "c"), _inputs("c")
    zt, zp = c["feats"]
    batch = (zt.permute(0, 3, 1, 2), torch.zeros(1, device=DEV), c["targets"].permute(0, 4, 1, 2, 3), c["mask"])
    Wc, bc, pre = P.fit_phase_probe([batch], _Views(zp.permute(0, 4, 1, 2, 3)), DEV, PC.RIDGE, halo=4, design="additive")
    g = _fit("c", standardize=True)
    W0, b0 = g.solve()
    assert torch.equal(Wc, W0) and torch.equal(bc, b0) and torch.equal(pre.mean_, g.mean_) and torch.equal(pre.std_, g.std_)
    assert tuple(Wc.shape) == fc["W"].shape
    Wt, _, _ = P.fit_phase_probe([batch], _Views(zp.permute(0, 4, 1, 2, 3)), DEV, PC.RIDGE, halo=4, design="type-only")
    Wp, _, _ = P.fit_phase_probe([batch], _Views(zp.permute(0, 4, 1, 2, 3)), DEV, PC.RIDGE, halo=4, design="phase-only")
    assert tuple(Wt.shape) == (64, 7) and tuple(Wp.shape) == (12, 7)
    with pytest.raises(RuntimeError, match="No valid observations"):
        P.fit_phase_probe([batch], _Views(zp.permute(0, 4, 1, 2, 3)), DEV, PC.RIDGE, halo=16, design="additive")
