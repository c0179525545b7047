"""GPU tests of the phase probe's "full" design (csrc/probe_full.hip, frl_hip/probe.py: InteractionProbe) against the float64 restatement
of tests/probe_full_cases.py and what the reference's own transform gave (tests/golden/probe_full_*.npz).

Tolerances (u = 2^-24; probe_full_cases.py derives each from float64 quantities of the case, never from the kernel's output):

Moments.  Every entry of S, Scq and Sqq against the float64 product of the same float32 rows c and q', which the test forms itself from
the pivot the kernel reports (q' by the same single float32 multiplication): 6 u sqrt(n) / 3 sum |v_i v_j| + 2 u |S_ij|, asserted for
every `workgroups`.  The count is exact, S and Sqq are symmetric, two runs give the same bits.

Evaluate.  pred within (2 Dt + 2 Dp + 2) u (|beta| + sum |x' u| + sum |p' v| + sum |x'| |Omega| |p'|) of the float64 value of the same
float32 model; SSE within sum 2 |err| dpred + dpred^2; the y sums within 2 n 2^-53 of sum |terms|; n exact.

End to end.  Predictions of the fit on the device against the golden's pred_64.  The host algebra is run again on the restatement's
moments pushed to the edge of the moment bound by a few seeded sign patterns; four times the largest change of a prediction, plus the
float32 storage of the model (3 u sum |z| |W|) and the evaluate bound, is the tolerance, and it must stay below 1e-3 of the largest
|pred_64| for the test to say anything.  DESIGN.md lists the tolerances and the reference's own d_ref.
"""
import os

import numpy as np
import pytest
import torch

import probe_cases as PC
import probe_full_cases as FC
from frl_hip import _lib, ops, probe as P
from frl_hip.probe import InteractionProbe

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = FC.U32
_IN = {}


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"probe_full_{name}.npz"))


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _inputs(case):
    """Inputs, their flattened form and device tensors (channels-last; z_type [B, H, W, Dt] where it is shared over t): once per case."""
    if case not in _IN:
        inp = FC.make_inputs(case)
        zt, zp, Y, m = FC.flatten(inp)
        a = inp["A"]
        _IN[case] = dict(inp=inp, zt=zt, zp=zp, Y=Y, m=m, feats=(_t(a[:, 0] if a.shape[1] == 1 else a), _t(inp["Bs"])), targets=_t(inp["Y"]),
                         mask=_t(inp["M"]), halo=inp["halo"], k=inp["k"])
    return _IN[case]


def _fit(case, workgroups=0, k=None):
    r = _inputs(case)
    g = InteractionProbe(FC.RIDGE, r["k"] if k is None else k, workgroups)
    return g.partial_fit(r["feats"], r["targets"], r["mask"], halo=r["halo"], channels_last=True)


def _check_moments(g, r, what):
    """-> (float64 moments, their bounds, pivot) after asserting the count, the symmetry and every entry of S, Scq, Sqq."""
    S, Scq, Sqq, n, pivot = g.moments()
    S, Scq, Sqq, pivot = S.numpy(), Scq.numpy(), Sqq.numpy(), pivot.numpy().astype(np.float32)
    assert n == int(r["m"].sum()), f"{what}: count {n}, expected {int(r['m'].sum())}"
    assert np.array_equal(S, S.T) and np.array_equal(Sqq, Sqq.T)
    c, q = FC.pivoted_rows(r["zt"], r["zp"], r["Y"], r["m"], pivot)
    want = [FC.product_moments(c, c), FC.product_moments(c, q), FC.product_moments(q, q)]
    for name, got, (s64, bound) in zip(("S", "Scq", "Sqq"), (S, Scq, Sqq), want):
        assert got.shape == s64.shape
        ratio = (np.abs(got - s64) / np.maximum(bound, 1e-300)).max()
        print(f"{what}: n {n}, {name} at {ratio:.3f} of the bound")
        assert np.all(np.abs(got - s64) <= bound), f"{what}: {name} at {ratio:.3f} of the bound"
    return want, pivot


def _same_state(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("_S", "_Scq", "_Sqq", "_n", "_pivot"))


# ---- 1. moments and count ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list("abcdef"))
def test_moments_and_count(case):
    r = _inputs(case)
    for wg in (1, 3, 0):
        g = _fit(case, wg)
        _check_moments(g, r, f"case {case} workgroups={wg}")
        assert _same_state(g, _fit(case, wg)), f"workgroups={wg}: two runs differ"


def test_folded_moments_are_those_of_the_plain_probe():
    """S, n and the pivot are frl_probe_accumulate's on the same inputs: bit for bit what RidgeProbe accumulates."""
    r = _inputs("b")
    g = _fit("b")
    plain = P.RidgeProbe(FC.RIDGE).partial_fit(r["feats"], r["targets"], r["mask"], halo=r["halo"], channels_last=True)
    assert torch.equal(g._S, plain._S) and torch.equal(g._n, plain._n) and torch.equal(g._pivot, plain._pivot)


# ---- 2. streaming --------------------------------------------------------------------------------------------------------------
def test_streaming_one_call_per_sample():
    r = _inputs("g")
    whole = _fit("g")
    parts = InteractionProbe(FC.RIDGE, r["k"])
    zt, zp = r["feats"]
    for i in range(zt.shape[0]):
        parts.partial_fit((zt[i:i + 1], zp[i:i + 1]), r["targets"][i:i + 1], r["mask"][i:i + 1], halo=r["halo"], channels_last=True)
    _check_moments(whole, r, "one call")
    _check_moments(parts, r, "one call per sample")
    assert int(parts._n.item()) == int(whole._n.item())
    first = InteractionProbe(FC.RIDGE, r["k"]).partial_fit((zt[:1], zp[:1]), r["targets"][:1], r["mask"][:1], halo=r["halo"], channels_last=True)
    assert torch.equal(first._pivot, parts._pivot) and not torch.equal(whole._pivot, parts._pivot)
    # an empty call changes nothing, and does not move the pivot
    before = [t.clone() for t in (parts._S, parts._Scq, parts._Sqq, parts._n)]
    parts.partial_fit((zt, zp), r["targets"], torch.zeros_like(r["mask"]), channels_last=True)
    assert all(torch.equal(a, b) for a, b in zip(before, (parts._S, parts._Scq, parts._Sqq, parts._n)))


# ---- 3. evaluate and metrics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list("abcdef"))
def test_evaluate_and_metrics(case):
    r = _inputs(case)
    zt, zp, Y = r["zt"], r["zp"], r["Y"]
    g = _fit(case)
    g.solve()
    pivot, beta, u, v, omega = (t.numpy() for t in g.pivoted_model())
    want, dp = FC.pivoted_pred(zt, zp, pivot, beta, u, v, omega)
    # predictions of every pixel, masked or not
    out = g.predict(r["feats"], channels_last=True)
    b_, h, w = r["inp"]["M"].shape
    t = r["inp"]["T"]
    cy = Y.shape[1]
    assert tuple(out.shape) == (b_, t, h, w, cy) and out.dtype == torch.float32
    pred = out.cpu().numpy().reshape(-1, cy)
    print(f"case {case}: pred at most {(np.abs(pred - want) / dp).max():.3f} of its bound")
    assert np.all(np.abs(pred - want) <= dp)
    assert torch.equal(out, g.predict(r["feats"], channels_last=True))
    assert torch.equal(out, InteractionProbe(FC.RIDGE, r["k"], 3).set_model(
        g.coef_, g.intercept_, g.mean_, g.std_, g.pca_components_, d_type=zt.shape[1], d_phase=zp.shape[1], pivot=pivot).predict(r["feats"], channels_last=True)), \
        "the prediction depends on the grid"
    _sums_and_metrics(g, r, want, dp, pivot, r["m"].reshape(b_, t, h, w)[:, 0], case, rho=False)
    # Spearman's rho^2 on a split without near-ties of the prediction (a pixel stays when all its timesteps do): a prediction that is
    # off by at most dp.max() reorders no pair that is 2 dp.max() apart
    keep = PC.separated_mask(want, r["m"], 2.0 * dp.max()).reshape(b_, t, h, w).all(1) & r["m"].reshape(b_, t, h, w)[:, 0]
    g.reset_evaluation()
    _sums_and_metrics(g, r, want, dp, pivot, keep, case, rho=True)


def _sums_and_metrics(g, r, want, dp, pivot, keep, case, rho):
    want_rho = rho
    zt, zp, Y = r["zt"], r["zp"], r["Y"]
    b_, h, w = r["inp"]["M"].shape
    t, cy = r["inp"]["T"], Y.shape[1]
    mm = np.ascontiguousarray(np.broadcast_to(keep[:, None], (b_, t, h, w))).reshape(-1)
    g.partial_evaluate(r["feats"], r["targets"], _t(keep), channels_last=True)
    E, n = g.evaluation_sums()
    assert n == int(mm.sum()) and n > (8 if rho else 64), f"the split of case {case} has {n} observations"
    y64 = Y[mm].astype(np.float64)
    err = np.abs(want[mm] - y64)
    d_sse = (2 * err * dp[mm] + dp[mm] ** 2).sum(0)
    sse64 = ((want[mm] - y64) ** 2).sum(0)
    yq = y64 - pivot[zt.shape[1] + zp.shape[1]:].astype(np.float64)
    dsum = 2 * n * FC.U64
    print(f"   n {n}, SSE {np.abs(E[:, 0] - sse64).max():.2e} (bound {d_sse.max():.2e})")
    assert np.all(np.abs(E[:, 0] - sse64) <= d_sse + dsum * sse64)
    assert np.all(np.abs(E[:, 1] - yq.sum(0)) <= dsum * np.abs(yq).sum(0)) and np.all(np.abs(E[:, 2] - (yq * yq).sum(0)) <= dsum * (yq * yq).sum(0))
    # without the ranks no prediction is written and empty tiles are skipped: the same sums, bit for bit
    g2 = _fit(case)
    g2.partial_evaluate(r["feats"], r["targets"], _t(keep), channels_last=True, rank=False)
    E2, n2 = g2.evaluation_sums()
    assert n2 == n and np.array_equal(E, E2)
    # metrics against the restatement's: MSE, R^2 and rho^2 of the float64 predictions of the same model on the same split
    names = [f"y{i}" for i in range(cy)]
    rho64 = [PC.spearman_rho2(want[mm][:, i], y64[:, i]) for i in range(cy)]
    ref = PC.metrics_from_sums(sse64, y64.sum(0), (y64 * y64).sum(0), n, rho64, names)
    mt = g.metrics(names)
    sst = (y64 * y64).sum(0) - y64.sum(0) ** 2 / n
    own_mse = (d_sse + dsum * sse64) / n
    d_sst = dsum * ((yq * yq).sum(0) + 2 * np.abs(yq.sum(0)) * np.abs(yq).sum(0) / n)
    own_r2 = own_mse * n / sst + sse64 * d_sst / sst ** 2
    mse = np.asarray([mt.mse_per_metric[k] for k in names])
    r2 = np.asarray([mt.r2_per_metric[k] for k in names])
    rho = np.asarray([mt.spearman_rho2_per_metric[k] for k in names])
    assert mt.n_pixels == n
    assert np.all(np.abs(mse - np.asarray([ref["mse_per_metric"][k] for k in names])) <= own_mse)
    assert np.all(np.abs(r2 - np.asarray([ref["r2_per_metric"][k] for k in names])) <= own_r2 + 1e-12)
    assert abs(mt.mse_total - ref["mse_total"]) <= own_mse.mean()
    if want_rho:
        print(f"   rho2 against float64 {np.abs(rho - np.asarray(rho64)).max():.2e} on {n} observations, R2 {r2.mean():.4f}")
        assert np.all(np.abs(rho - np.asarray(rho64)) <= 1e-6) and abs(mt.spearman_rho2_total - ref["spearman_rho2_total"]) <= 1e-6
    with pytest.raises(ValueError):
        g.metrics(names[:-1])


# ---- 4. end to end -------------------------------------------------------------------------------------------------------------
def _end_to_end_tolerance(g, r, k=None, patterns=3):
    """-> (tolerance, moment part, evaluate part): see the module docstring.  Float64 quantities of the case only; of the fit on the
    device it takes the pivot and the float32 model the evaluate bound is stated for."""
    zt, zp, Y, m = r["zt"], r["zp"], r["Y"], r["m"]
    dt, dp = zt.shape[1], zp.shape[1]
    pivot = g.moments()[4].numpy().astype(np.float32)
    c, q = FC.pivoted_rows(zt, zp, Y, m, pivot)
    (S, dS), (Scq, dScq), (Sqq, dSqq) = FC.product_moments(c, c), FC.product_moments(c, q), FC.product_moments(q, q)
    n = int(m.sum())

    def preds(S_, Scq_, Sqq_):
        h = InteractionProbe.from_moments(S_, Scq_, Sqq_, n, pivot, dt, dp, FC.RIDGE, r["k"] if k is None else k)
        h.solve()
        own = dict(mean=h.mean_.numpy(), std=h.std_.numpy(), comp=None if h.pca_components_ is None else h.pca_components_.numpy())
        return FC.predict64(own, h.coef64_.numpy(), h.intercept64_.numpy(), zt[m], zp[m]), own, h

    base, own, h = preds(S, Scq, Sqq)
    rng = np.random.default_rng(2024)
    change = 0.0
    for _ in range(patterns):
        sg = np.triu(rng.choice([-1.0, 1.0], size=S.shape))
        sq = np.triu(rng.choice([-1.0, 1.0], size=Sqq.shape))
        sg, sq = sg + np.triu(sg, 1).T, sq + np.triu(sq, 1).T
        sg[-1, -1] = 0.0                                                         # the count is exact
        pert, _, _ = preds(S + sg * dS, Scq + rng.choice([-1.0, 1.0], size=Scq.shape) * dScq, Sqq + sq * dSqq)
        change = max(change, float(np.abs(pert - base).max()))
    z = np.abs(FC.transform(own, zt[m], zp[m], round32=False))
    store = float((3 * U * (z @ np.abs(h.coef64_.numpy()) + np.abs(h.intercept64_.numpy()))).max())
    ev = float(FC.pivoted_pred(zt[m], zp[m], *(t.numpy() for t in g.pivoted_model()))[1].max())
    return 4.0 * change + store + ev, 4.0 * change, store + ev


@pytest.mark.parametrize("case", list("abcdef"))
def test_end_to_end_against_pred_64(golden_dir, case):
    fx, r = _fx(golden_dir, case), _inputs(case)
    assert FC.checksum(r["inp"]) == int(fx["checksum"])
    zt, zp = r["feats"]
    ximg = zt.permute(0, 3, 1, 2) if zt.dim() == 4 else zt.permute(0, 4, 1, 2, 3)    # the reference's channels-first shapes, as views
    batch = (ximg, torch.zeros(1, device=DEV), r["targets"].permute(0, 4, 1, 2, 3), r["mask"])
    W, b, g = P.fit_phase_probe_full([batch], _Views(zp.permute(0, 4, 1, 2, 3)), DEV, FC.RIDGE, halo=r["halo"], interaction_pca_k=r["k"])
    assert W.dtype == torch.float32 and tuple(W.shape) == (P.full_design_dim(r["zt"].shape[1], r["zp"].shape[1], r["k"]), r["Y"].shape[1])
    assert g.n_obs_ == int(fx["n_obs"]) and _same_state(g, _fit(case))
    pred = g.predict(r["feats"], channels_last=True).cpu().numpy().reshape(-1, r["Y"].shape[1])[r["m"]].astype(np.float64)
    tol, mom, rest = _end_to_end_tolerance(g, r)
    big = float(np.abs(fx["pred_64"]).max())
    err = float(np.abs(pred - fx["pred_64"]).max())
    print(f"case {case}: |pred - pred_64| {err:.3g}, tolerance {tol:.3g} (moments {mom:.3g}, model storage and evaluate {rest:.3g}), "
          f"{tol / big:.2e} of the largest |pred_64| {big:.3g}; the reference's own d_ref {float(fx['d_ref']):.3g}")
    assert tol < 1e-3 * big, "the tolerance says nothing"
    assert err <= tol
    with pytest.raises(RuntimeError, match="No valid observations found in training data; cannot fit probe."):
        P.fit_phase_probe_full([batch[:3] + (torch.zeros_like(r["mask"]),)], _Views(zp.permute(0, 4, 1, 2, 3)), DEV)


def test_fit_without_pca():
    """k = 0: the ridge fit on all Dt + Dp + Dq standardised columns."""
    r = _inputs("a")
    g = _fit("a", k=0)
    W, b = g.solve()
    assert g.pca_components_ is None and tuple(W.shape) == (5 + 3 + 15, 3)
    m = r["m"]
    own = dict(mean=g.mean_.numpy(), std=g.std_.numpy(), comp=None)
    want = FC.two_passes(r["inp"], 0)
    pred = g.predict(r["feats"], channels_last=True).cpu().numpy().reshape(-1, 3)[m]
    ref = FC.predict64(want["pre"], want["W"], want["b"], r["zt"][m], r["zp"][m])
    tol = _end_to_end_tolerance(g, r, k=0)[0]
    print(f"k = 0: |pred - pred_64| {np.abs(pred - ref).max():.3g}, tolerance {tol:.3g}")
    assert tol < 1e-3 * np.abs(ref).max()
    assert np.abs(pred - ref).max() <= tol and np.abs(FC.predict64(own, W.numpy(), b.numpy(), r["zt"][m], r["zp"][m]) - ref).max() <= tol


# ---- 5. layouts and refusals ---------------------------------------------------------------------------------------------------
class _Views:
    """The model of the helper's test: z_type and z_phase are channels-first views of channels-last latents."""

    def __init__(self, z_phase):
        self.z_phase = z_phase

    def __call__(self, ximg):
        return ximg

    def forward_phase(self, xphase, z_type):
        return self.z_phase


def test_abi_refuses_what_it_cannot_run():
    lib = _lib.load()
    x = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)
    m = torch.ones(64, dtype=torch.uint8, device=DEV)
    Sd = torch.zeros(768 * 768, dtype=torch.float64, device=DEV)
    ws = ops.probe_full_workspace(8, 4, 2, DEV)
    p = lambda t: t.data_ptr()                                                   # noqa: E731

    def acc(dt, dp, cy, ta, tb, ty, b, t, pp, wg=0, nbytes=None):
        return lib.frl_probe_full_accumulate(p(x), ta, dt, p(x) if dp else None, tb, dp, p(x), ty, cy, p(m), b, t, pp, p(x), wg, p(Sd), p(Sd), p(ws),
                                             ws.numel() if nbytes is None else nbytes, None)

    assert acc(8, 4, 2, 1, 1, 1, 1, 1, 4) == 0
    torch.cuda.synchronize()
    for bad in ((65, 2, 2, 1, 1, 1, 1, 1, 4), (8, 17, 2, 1, 1, 1, 1, 1, 4), (64, 13, 2, 1, 1, 1, 1, 1, 4), (8, 0, 2, 1, 1, 1, 1, 1, 4),
                (8, 4, 17, 1, 1, 1, 1, 1, 4), (8, 4, 0, 1, 1, 1, 1, 1, 4), (8, 4, 2, 2, 1, 1, 1, 3, 4), (8, 4, 2, 1, 2, 1, 1, 3, 4),
                (8, 4, 2, 1, 1, 2, 1, 3, 4), (8, 4, 2, 1, 1, 1, 1 << 12, 1 << 10, 1 << 9), (8, 4, 2, 1, 1, 1, 1, 1, 4, 4097)):
        assert acc(*bad) == -2, bad
    assert acc(8, 4, 2, 1, 1, 1, 1, 1, 4, 0, 16) == -4
    assert lib.frl_probe_full_workspace_bytes(65, 2, 2, 0) == 0 and lib.frl_probe_full_workspace_bytes(64, 13, 2, 0) == 0
    assert lib.frl_probe_full_workspace_bytes(64, 12, 17, 0) == 0 and lib.frl_probe_full_workspace_bytes(64, 12, 7, 4097) == 0
    with pytest.raises(ValueError):
        ops.probe_full_workspace(64, 13, 7, DEV)
    r = _inputs("a")
    with pytest.raises(ValueError, match="Dt = 5"):
        _fit("a").partial_fit(_inputs("b")["feats"], _inputs("b")["targets"][..., :3].contiguous(), _inputs("b")["mask"], channels_last=True)
    assert r["feats"][0].dim() == 5
