"""Cases, inputs, the float64 restatement and the error bounds for the linear-probe tests (test_cpu_probe.py, test_gpu_probe.py).

Inputs are regenerated from numpy's default_rng, never stored; tests/golden/probe_*.npz (tests/golden/make_probe_golden.py) holds what
the reference's own functions gave for them, and a checksum of the inputs.  No product code is imported here.

Layout of a case: A [B, Ta, H, W, Da], Bs [B, Tb, H, W, Db] | None, Y [B, Ty, H, W, Cy] float32 (T_s = 1: shared over t), M [B, H, W]
bool.  An observation is (b, t, h, w); `flatten` lists them in that order, as the reference's reshape(-1, D)[m_flat] does.

The restatement writes the masked normal equations with the ones column exactly as fit_closed_form_ridge and fit_phase_probe do
(A = Xaug^T Xaug, B = Xaug^T Y in float64, no penalty on the bias row), the statistics of _compute_feature_statistics, and the sums of
evaluate_probe, all in float64.

Bounds (u = 2^-24), none of them taken from the code under test:

Moments.  S_ij is a sum over the n unmasked rows of float32 products v_i v_j: fmaf chains inside a workgroup, double beyond.  The
repo's chain model (test_gpu_gmm.py): independent roundings, each at most u times a partial sum that grows linearly, give a standard
deviation u sqrt(n) / 3 of sum |v_i v_j|; six of them, plus 2 u |S_ij| for the float32 slab.  The worst split is one workgroup.

W and b.  With M = Sigma_xx + lambda I, the first-order elementwise perturbation bound of M W = Sigma_xy is
|dW| <= |M^-1| (dB + dA |W|), doubled for the higher orders; dA and dB follow from the moment bounds through
Sigma = S_vv - s s^T / n.  b = ybar - xbar^T W gives |db| <= sum |xbar| dW + the bound on ybar.

Evaluate.  pred_c = bc_c + sum_d (x_d - p_d) Wc_dc is D fused multiply-adds after one float32 subtraction per feature:
(D + 2) u (|bc| + sum |x_d - p_d| |Wc_dc|).  SSE moves by at most sum 2 |err| dpred + dpred^2.  The double sums carry n 2^-53 of
sum |terms| each, in the test's order and in the kernel's.
"""
from __future__ import annotations

import zlib

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
RIDGE = 1e-3
TARGET_METRICS = ["static.mean_ndvi", "static.mean_ndmi", "static.mean_nbr", "static.mean_seasonal_amp_nir", "static.variance_ndvi"]

CASES = {
    "a": dict(b=2, h=23, w=23, t=1, da=64, db=0, cy=5, ta=1, ty=1, keep=0.6, seed=11),          # the static probe; P no multiple of 64 or 4
    "b": dict(b=2, h=9, w=31, t=3, da=12, db=0, cy=7, ta=3, ty=3, keep=0.6, seed=12),           # fewer than 16 columns
    "c": dict(b=2, h=23, w=23, t=3, da=64, db=12, cy=7, ta=1, tb=3, ty=3, keep=0.7, halo=4, seed=13),   # two sources, broadcast, halo
    "d": dict(b=1, h=10, w=20, t=1, da=128, db=0, cy=16, ta=1, ty=1, keep=0.9, seed=14),        # the limits
    "e": dict(b=3, h=23, w=23, t=2, da=12, db=0, cy=3, ta=2, ty=1, keep=0.5, seed=15, holes=True),  # a masked sample, a masked tile
    "f": dict(base="a", shift=1000.0),                                                         # the pivot
    "g": dict(b=3, h=23, w=23, t=1, da=64, db=0, cy=5, ta=1, ty=1, keep=0.6, seed=17),          # streaming: three calls against one
}
GOLDEN_REFERENCE_CASES = ["a", "f", "g"]          # D = 64 and five targets, as the reference hard-codes
PHASE_CASES = ["b", "c"]


def _features(rng, n, d):
    """Well conditioned: an orthogonal mix of unit normals, column scales 0.5 to 2, a small offset."""
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    return (rng.normal(size=(n, d)) @ q) * rng.uniform(0.5, 2.0, size=d) + rng.normal(0.0, 0.3, size=d)


def make_inputs(case: str):
    c = CASES[case]
    if "base" in c:
        out = dict(make_inputs(c["base"]))
        out["A"] = (out["A"] + np.float32(c["shift"])).astype(np.float32)
        if out["Bs"] is not None:
            out["Bs"] = (out["Bs"] + np.float32(c["shift"])).astype(np.float32)
        return out
    rng = np.random.default_rng(c["seed"])
    b, h, w, t = c["b"], c["h"], c["w"], c["t"]
    a = _features(rng, b * c["ta"] * h * w, c["da"]).reshape(b, c["ta"], h, w, c["da"])
    bs = _features(rng, b * c["tb"] * h * w, c["db"]).reshape(b, c["tb"], h, w, c["db"]) if c["db"] else None
    x = np.broadcast_to(a, (b, t, h, w, c["da"]))
    if bs is not None:
        x = np.concatenate([x, np.broadcast_to(bs, (b, t, h, w, c["db"]))], -1)
    d = c["da"] + c["db"]
    w0 = rng.normal(0.0, 1.0 / np.sqrt(d), size=(d, c["cy"]))
    y = x @ w0 + rng.normal(0.0, 0.5, size=c["cy"]) + rng.normal(0.0, 0.3, size=(b, t, h, w, c["cy"]))
    if c["ty"] == 1:
        y = y[:, :1]
    m = rng.random((b, h, w)) < c["keep"]
    if c.get("holes"):
        m[1] = False                                                             # one sample wholly masked
        m[0].reshape(-1)[64:128] = False                                         # one whole 64-tile masked
    return dict(A=a.astype(np.float32), Bs=None if bs is None else bs.astype(np.float32), Y=np.ascontiguousarray(y).astype(np.float32), M=m,
                T=t, halo=c.get("halo", 0))


def checksum(inp) -> int:
    h = 0
    for key in ("A", "Bs", "Y", "M"):
        if inp.get(key) is not None:
            h = zlib.crc32(np.ascontiguousarray(inp[key]).tobytes(), h)
    return h


def halo_mask(h, w, halo):
    m = np.zeros((h, w), bool)
    if 2 * halo >= h or 2 * halo >= w:
        return m
    m[halo:h - halo, halo:w - halo] = True
    return m


def flatten(inp):
    """-> (X f32 [N, D], Y f32 [N, Cy], m bool [N]) over all observations (b, t, h, w), the halo folded into the mask."""
    a, bs, y, m, t = inp["A"], inp["Bs"], inp["Y"], inp["M"], inp["T"]
    b, _, h, w, _ = a.shape
    x = np.broadcast_to(a, (b, t, h, w, a.shape[-1]))
    if bs is not None:
        x = np.concatenate([x, np.broadcast_to(bs, (b, t, h, w, bs.shape[-1]))], -1)
    yy = np.broadcast_to(y, (b, t, h, w, y.shape[-1]))
    mm = m & halo_mask(h, w, inp["halo"])[None] if inp["halo"] else m
    mm = np.broadcast_to(mm[:, None], (b, t, h, w))
    return np.ascontiguousarray(x).reshape(-1, x.shape[-1]), np.ascontiguousarray(yy).reshape(-1, y.shape[-1]), np.ascontiguousarray(mm).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def normal_equations(X, Y):
    """A = Xaug^T Xaug, B = Xaug^T Y in float64 with the ones column last."""
    xa = np.concatenate([np.asarray(X, np.float64), np.ones((len(X), 1))], 1)
    return xa.T @ xa, xa.T @ np.asarray(Y, np.float64)


def ridge_from_normal(A, B, lam):
    """-> (W float64 [D, Cy], b float64 [Cy], cond(A + reg)): the penalty leaves the bias row out."""
    reg = np.eye(len(A)) * lam
    reg[-1, -1] = 0.0
    wb = np.linalg.solve(A + reg, B)
    return wb[:-1], wb[-1], float(np.linalg.cond(A + reg))


def ridge_fit(X, Y, m, lam=RIDGE):
    if not m.any():
        raise RuntimeError("No valid pixels found in training data; cannot fit probe.")
    A, B = normal_equations(X[m], Y[m])
    return ridge_from_normal(A, B, lam)


def feature_statistics(X, m):
    """_compute_feature_statistics: float64 sums -> (mean float32, std float32)."""
    x = np.asarray(X[m], np.float64)
    n = len(x)
    mean = x.sum(0) / n
    var = (x * x).sum(0) / n - mean * mean
    return mean.astype(np.float32), np.sqrt(np.maximum(var, 1e-16)).astype(np.float32)


def standardise(X, mean, std):
    """ProbePreprocessor.transform for a design without interaction: float64 arithmetic, rounded to float32."""
    return ((np.asarray(X, np.float64) - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)


def phase_fit(X, Y, m, lam=RIDGE):
    """fit_phase_probe: pass 1 statistics, pass 2 ridge on the standardised float32 columns -> (W, b, cond, mean, std)."""
    if not m.any():
        raise RuntimeError("No valid observations found in training data; cannot fit probe.")
    mean, std = feature_statistics(X, m)
    W, b, cond = ridge_fit(standardise(X, mean, std), Y, m, lam)
    return W, b, cond, mean, std


def spearman_rho2(p, t):
    n = len(p)
    if n < 2:
        return 0.0
    pr = np.argsort(np.argsort(np.asarray(p, np.float64), kind="stable"), kind="stable").astype(np.float64)
    tr = np.argsort(np.argsort(np.asarray(t, np.float64), kind="stable"), kind="stable").astype(np.float64)
    pc, tc = pr - pr.mean(), tr - tr.mean()
    den = np.sqrt((pc * pc).sum() * (tc * tc).sum())
    return 0.0 if den < 1e-12 else float(((pc * tc).sum() / den) ** 2)


def separated_mask(pred, m, sep):
    """m without every row whose prediction lies within `sep` of another unmasked row's in some column: on what is left a prediction
    error below sep / 2 reorders no pair, so Spearman's rho^2 does not feel it."""
    keep = m.copy()
    rows = np.flatnonzero(m)
    for c in range(pred.shape[1]):
        order = rows[np.argsort(pred[rows, c], kind="stable")]
        close = np.flatnonzero(np.diff(pred[order, c]) < sep)
        keep[order[close]] = False
        keep[order[close + 1]] = False
    return keep


def eval_sums(X, Y, m, W, b):
    """float64 predictions of the float32 model over the unmasked rows -> dict(pred, sse, sum_y, sum_y2, n)."""
    x, y = np.asarray(X[m], np.float64), np.asarray(Y[m], np.float64)
    pred = x @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
    err = pred - y
    return dict(pred=pred, y=y, sse=(err * err).sum(0), sum_y=y.sum(0), sum_y2=(y * y).sum(0), n=int(m.sum()))


def reference_metric_bounds(X, Y, m, W, b):
    """What the reference's own float32 arithmetic (the einsum, err * err, the pairwise sums) can move its SSE, MSE and R2 by
    -> dict(sse, mse, r2) [Cy] around the float64 values of eval_sums."""
    s = eval_sums(X, Y, m, W, b)
    n = s["n"]
    lg = (np.ceil(np.log2(max(n, 2))) + 3) * U32
    dp = (X.shape[1] + 2) * U32 * (np.abs(np.asarray(b, np.float64)) + np.abs(X[m].astype(np.float64)) @ np.abs(np.asarray(W, np.float64)))
    err = np.abs(s["pred"] - s["y"])
    d_sse = (2 * err * dp + dp * dp).sum(0) + lg * s["sse"]
    sst = s["sum_y2"] - s["sum_y"] ** 2 / n
    d_sst = lg * (s["sum_y2"] + 2 * np.abs(s["sum_y"]) * np.abs(s["y"]).sum(0) / n)
    return dict(sse=d_sse, mse=d_sse / n, r2=d_sse / sst + s["sse"] * d_sst / sst ** 2, sst=sst)


def metrics_from_sums(sse, sum_y, sum_y2, n, rho2, names):
    """The rules of evaluate_probe: R2 is 0 where SST <= 1e-8, everything 0 where n = 0."""
    mse, r2, rho = {}, {}, {}
    for i, k in enumerate(names):
        if n == 0:
            mse[k] = r2[k] = rho[k] = 0.0
            continue
        mse[k] = float(sse[i]) / n
        sst = max(0.0, float(sum_y2[i]) - float(sum_y[i]) ** 2 / n)
        r2[k] = 1.0 - float(sse[i]) / sst if sst > 1e-8 else 0.0
        rho[k] = float(rho2[i])
    return dict(mse_per_metric=mse, r2_per_metric=r2, spearman_rho2_per_metric=rho, mse_total=float(np.mean([mse[k] for k in names])),
                r2_total=float(np.mean([r2[k] for k in names])), spearman_rho2_total=float(np.mean([rho[k] for k in names])), n_pixels=n)


def metrics(X, Y, m, W, b, names):
    s = eval_sums(X, Y, m, W, b)
    rho2 = [spearman_rho2(s["pred"][:, i], s["y"][:, i]) for i in range(Y.shape[1])]
    return metrics_from_sums(s["sse"], s["sum_y"], s["sum_y2"], s["n"], rho2, names)


# ---------------------------------------------------------------------------------------------------------------------------------
# moments of the pivoted rows, and the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def pivoted_rows(X, Y, m, pivot):
    """v = [x - p_x | y - p_y | 1] of the unmasked rows, the subtraction in float32 as the kernel does it -> float32 [n, C + 1]."""
    p = np.asarray(pivot, np.float32)
    d = X.shape[1]
    v = np.concatenate([X[m] - p[:d], Y[m] - p[d:], np.ones((int(m.sum()), 1), np.float32)], 1)
    assert v.dtype == np.float32
    return v


def moments(v):
    """-> (S float64 = v^T v, bound) with the chain model of the module docstring."""
    v64 = v.astype(np.float64)
    S = v64.T @ v64
    n = max(len(v), 1)
    return S, 6.0 * U32 * np.sqrt(n) / 3.0 * (np.abs(v64).T @ np.abs(v64)) + 2.0 * U32 * np.abs(S)


def exact_moments(X, Y, m, pivot):
    """S = v^T v for the exact v = [x - p | y - p | 1] in float64 (no float32 subtraction): what from_moments is fed on the CPU."""
    p = np.asarray(pivot, np.float64)
    d = X.shape[1]
    v = np.concatenate([X[m].astype(np.float64) - p[:d], Y[m].astype(np.float64) - p[d:], np.ones((int(m.sum()), 1))], 1)
    return v.T @ v


def solve_bounds(S, dS, n, pivot, d, lam=RIDGE, std=None):
    """The elementwise bounds of the module docstring on W [D, Cy] and b [Cy], from float64 moments S, their bounds dS and the count.
    std: the solve is for the standardised columns."""
    c = S.shape[0] - 1
    s, ds = S[:c, c], dS[:c, c]
    cov = S[:c, :c] - np.outer(s, s) / n
    dcov = dS[:c, :c] + (np.outer(np.abs(s), ds) + np.outer(ds, np.abs(s))) / n
    mean = np.asarray(pivot, np.float64) + s / n
    sc = np.ones(d) if std is None else 1.0 / np.asarray(std, np.float64)
    Mx = cov[:d, :d] * sc[:, None] * sc[None, :] + lam * np.eye(d)
    Bx = cov[:d, d:] * sc[:, None]
    dA = dcov[:d, :d] * sc[:, None] * sc[None, :]
    dB = dcov[:d, d:] * sc[:, None]
    if std is not None:                                                          # what ProbePreprocessor.transform's float32 rounding moves
        zA, zB = standardise_bounds(n, Mx - lam * np.eye(d), cov[d:, d:])
        dA, dB = dA + zA, dB + zB
    W = np.linalg.solve(Mx, Bx)
    dW = 2.0 * np.abs(np.linalg.inv(Mx)) @ (dB + dA @ np.abs(W))
    # the mean of a standardised column is what rounding the mean to float32 leaves
    xbar = np.abs(mean[:d]) if std is None else np.abs(mean[:d] - mean[:d].astype(np.float32).astype(np.float64)) * sc
    db = xbar @ dW + ds[d:] / n
    if std is not None:                                                          # the column means of the rounded entries: u mean |z| <= u rms z
        db = db + U32 * np.sqrt(np.diagonal(Mx - lam * np.eye(d)) / n) @ np.abs(W)
    return dW, db


def standardise_bounds(n, szz, syy):
    """ProbePreprocessor.transform rounds every standardised entry to float32 (relative u) before the float64 accumulation, and its
    columns are centred only up to the float32 rounding of the mean.  By Cauchy-Schwarz sum |z_i z_j| <= sqrt(sum z_i^2 sum z_j^2),
    so the scatter moves by at most 2 u (doubled: the uncentred second moment of a column is its scatter plus n times a squared
    mean that is itself of relative size u) times that -> (dA [D, D], dB [D, Cy]) from the centred scatters szz and syy."""
    z, y = np.sqrt(np.diagonal(szz)), np.sqrt(np.diagonal(syy))
    return 4.0 * U32 * np.outer(z, z), 2.0 * U32 * np.outer(z, y)


def pred_bound(X, pivot, Wc, bc):
    """(D + 2) u (|bc| + sum |x_d - p_d| |Wc_dc|) per observation -> [N, Cy]."""
    d = X.shape[1]
    xc = np.abs(X.astype(np.float64) - np.asarray(pivot, np.float64)[:d])
    return (d + 2) * U32 * (np.abs(np.asarray(bc, np.float64)) + xc @ np.abs(np.asarray(Wc, np.float64)))


def pivoted_pred(X, pivot, Wc, bc):
    """float64 predictions of the pivoted float32 model the kernel is handed."""
    d = X.shape[1]
    return (X.astype(np.float64) - np.asarray(pivot, np.float64)[:d]) @ np.asarray(Wc, np.float64) + np.asarray(bc, np.float64)
