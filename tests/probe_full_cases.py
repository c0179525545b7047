"""Cases, inputs, the float64 restatement and the error bounds for the tests of the phase probe's "full" design
(test_cpu_probe_full.py, test_gpu_probe_full.py).  No product code is imported here.

Inputs are regenerated from numpy's default_rng, never stored; tests/golden/probe_full_*.npz (tests/golden/make_probe_full_golden.py) holds
what the reference's own ProbePreprocessor.transform gave for them, and a checksum of the inputs.

Layout of a case: A = z_type [B, Ta, H, W, Dt] (Ta = 1: shared over t), Bs = z_phase [B, T, H, W, Dp], Y [B, T, H, W, Cy] float32,
M [B, H, W] bool.  An observation is (b, t, h, w); `flatten` lists them in that order, as the reference's reshape(-1, D)[m_flat] does.

The restatement is the reference's two passes as written, in float64: pass 1 (`statistics`) sums x, x^2 and the interaction outer
product of the raw design matrix [z_type | z_phase | z_type (x) z_phase] (the interaction a float32 product, column i Dp + a), then mean,
std, the eigenvectors of the standardised interaction covariance, all rounded to float32 as ProbePreprocessor stores them; pass 2
(`ridge`) transforms every row with the stored values and solves the normal equations with the ones column, no penalty on the bias.
`round32` reproduces the reference's rounding of the transformed row to float32; without it the fit is float64 throughout.

Bounds (u = 2^-24, e = 2^-53), none of them taken from the code under test:

Moments.  The chain model of probe_cases.py: an entry of c^T q' or q'^T q' is a sum over the n unmasked rows of float32 products
v_i v_j, fmaf chains inside a workgroup and double beyond: 6 u sqrt(n) / 3 sum |v_i v_j| + 2 u |S_ij|.  The rows v are formed by the
test exactly as the kernel forms them: x' = x - pivot and p' = p - pivot are float32 subtractions and q'_ia = x'_i p'_a is one float32
multiplication, so the rounding of the factor product is in v itself and adds no term of its own (it would be one more u per factor
product, 2 u sum |v_i v_j| at the most, were the test to take q' exact).

Two algebras (CPU).  The product goes from moments about a pivot through the maps L and R, the restatement from raw sums.  Both are
float64; what separates them is the rounding of sums of n terms, e sqrt(n) in the chain model, magnified by (1 + max mean^2 / var) where
the raw sums cancel: eps = 4 e sqrt(n) (1 + max mean^2 / var).  mean and std carry eps (and one float32 rounding).  An eigenvector
turns by at most 4 eps / gap with gap = (lambda_k - lambda_k+1) / lambda_1, so comp comp^T moves by that fraction of
sum_j |v_j| |v_j|^T / lambda_j, plus 2 u of it for the float32 rounding of the components.  W and b solve a system of condition
cond(A + lambda I): they move by 8 cond (eps + 4 eps / gap) of max |W|.

Evaluate.  With h_a a chain of Dt fused multiply-adds and the outer chain of Dt + 2 Dp after beta,
|pred - pred64| <= (2 Dt + 2 Dp + 2) u (|beta| + sum |x'_i u_i| + sum |p'_a v_a| + sum |x'_i| |Omega_ia| |p'_a|), both sides from the
same float32 x', p'.
"""
from __future__ import annotations

import zlib

import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
RIDGE = 1e-3

CASES = {
    "a": dict(b=2, t=3, h=9, w=13, dt=5, dp=3, cy=3, k=4, ta=3, keep=0.7, seed=31),      # Dq = 15: under one block; P no multiple of 64
    "b": dict(b=2, t=3, h=23, w=23, dt=16, dp=4, cy=7, k=8, ta=1, keep=0.7, halo=4, seed=32),    # z_type shared over T, halo
    "c": dict(b=1, t=2, h=10, w=13, dt=64, dp=12, cy=7, k=20, ta=1, keep=1.0, seed=33),   # fewer observations than columns
    "d": dict(b=2, t=2, h=23, w=23, dt=64, dp=12, cy=7, k=20, ta=1, keep=0.8, seed=34),   # the production widths
    "e": dict(base="b", shift=3.0),                                                      # the pivot
    "f": dict(base="b", holes=True),                                                     # a masked sample, a masked tile
    "g": dict(base="d"),                                                                 # streaming: one call per sample
}
GOLDEN_CASES = ["a", "b", "c", "d", "e", "f"]
GOLDEN_ROWS = 6                                                                          # observations whose transformed rows are stored
CCT_ROWS = 16                                                                            # rows of comp comp^T that are stored


def _features(rng, n, d):
    """Well conditioned: an orthogonal mix of unit normals, column scales 0.5 to 2, a small offset."""
    q, _ = np.linalg.qr(rng.normal(size=(d, d)))
    return (rng.normal(size=(n, d)) @ q) * rng.uniform(0.5, 2.0, size=d) + rng.normal(0.0, 0.3, size=d)


def make_inputs(case: str):
    c = CASES[case]
    if "base" in c:
        out = dict(make_inputs(c["base"]))
        if "shift" in c:
            out["A"] = (out["A"] + np.float32(c["shift"])).astype(np.float32)
            out["Bs"] = (out["Bs"] - np.float32(c["shift"])).astype(np.float32)
        if c.get("holes"):
            m = out["M"].copy()
            m[1] = False                                                         # one sample wholly masked
            m[0].reshape(-1)[64:128] = False                                     # one whole 64-tile masked
            out["M"] = m
        return out
    rng = np.random.default_rng(c["seed"])
    b, t, h, w, dt, dp, cy = c["b"], c["t"], c["h"], c["w"], c["dt"], c["dp"], c["cy"]
    a = _features(rng, b * c["ta"] * h * w, dt).reshape(b, c["ta"], h, w, dt)
    bs = _features(rng, b * t * h * w, dp).reshape(b, t, h, w, dp)
    x = np.broadcast_to(a, (b, t, h, w, dt))
    q = (x[..., :, None] * bs[..., None, :]).reshape(b, t, h, w, dt * dp)
    y = (x @ rng.normal(0.0, 1.0 / np.sqrt(dt), size=(dt, cy)) + bs @ rng.normal(0.0, 1.0 / np.sqrt(dp), size=(dp, cy))
         + q @ rng.normal(0.0, 0.5 / np.sqrt(dt * dp), size=(dt * dp, cy)) + rng.normal(0.0, 0.5, size=cy) + rng.normal(0.0, 0.3, size=(b, t, h, w, cy)))
    m = rng.random((b, h, w)) < c["keep"]
    return dict(A=a.astype(np.float32), Bs=bs.astype(np.float32), Y=y.astype(np.float32), M=m, T=t, halo=c.get("halo", 0), k=c["k"])


def checksum(inp) -> int:
    h = 0
    for key in ("A", "Bs", "Y", "M"):
        h = zlib.crc32(np.ascontiguousarray(inp[key]).tobytes(), h)
    return h


def halo_mask(h, w, halo):
    m = np.zeros((h, w), bool)
    if 2 * halo >= h or 2 * halo >= w:
        return m
    m[halo:h - halo, halo:w - halo] = True
    return m


def flatten(inp):
    """-> (zt f32 [N, Dt], zp f32 [N, Dp], Y f32 [N, Cy], m bool [N]) over all observations (b, t, h, w), the halo folded into the mask."""
    a, bs, y, m, t = inp["A"], inp["Bs"], inp["Y"], inp["M"], inp["T"]
    b, _, h, w, _ = a.shape
    zt = np.ascontiguousarray(np.broadcast_to(a, (b, t, h, w, a.shape[-1]))).reshape(-1, a.shape[-1])
    mm = m & halo_mask(h, w, inp["halo"])[None] if inp["halo"] else m
    mm = np.ascontiguousarray(np.broadcast_to(mm[:, None], (b, t, h, w))).reshape(-1)
    return zt, bs.reshape(-1, bs.shape[-1]), y.reshape(-1, y.shape[-1]), mm


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def design_matrix(zt, zp):
    """[z_type | z_phase | z_type (x) z_phase] float32, the interaction in the reference's column order i Dp + a."""
    zt, zp = np.asarray(zt, np.float32), np.asarray(zp, np.float32)
    q = (zt[:, :, None] * zp[:, None, :]).reshape(len(zt), -1)
    assert q.dtype == np.float32
    return np.concatenate([zt, zp, q], 1)


def statistics(zt, zp, k):
    """Pass 1 -> dict(mean, std float32 [Dt + Dp + Dq]; comp float32 [Dq, k] | None; evr float32 [k] | None; eigvals, gap, offset_ratio)."""
    x = design_matrix(zt, zp).astype(np.float64)
    n, dm = len(x), zt.shape[1] + zp.shape[1]
    mean = x.sum(0) / n
    var = (x * x).sum(0) / n - mean * mean
    std = np.sqrt(np.maximum(var, 1e-16))
    out = dict(mean=mean.astype(np.float32), std=std.astype(np.float32), comp=None, evr=None, gap=np.inf,
               offset_ratio=float((mean * mean / np.maximum(var, 1e-16)).max()), n=n)
    dq = x.shape[1] - dm
    k = min(int(k), dq)
    if k > 0:
        xi = x[:, dm:]
        cov_raw = xi.T @ xi / n - np.outer(mean[dm:], mean[dm:])
        inv = 1.0 / std[dm:]
        cov_std = inv[:, None] * cov_raw * inv[None, :]
        vals, vecs = np.linalg.eigh(cov_std)
        top_vecs, top_vals = vecs[:, ::-1][:, :k], vals[::-1][:k]
        out["comp"] = (top_vecs / np.sqrt(np.maximum(top_vals, 1e-12))[None, :]).astype(np.float32)
        out["evr"] = (np.maximum(top_vals, 0.0) / np.maximum(vals, 0.0).sum()).astype(np.float32)
        nxt = vals[::-1][k] if k < dq else 0.0
        out["gap"] = float((top_vals[-1] - nxt) / vals[-1])
        out["eigvals"] = vals[::-1].copy()
        out["weight"] = (np.abs(top_vecs) / np.maximum(top_vals, 1e-12)[None, :]) @ np.abs(top_vecs).T   # sum_j |v_j| |v_j|^T / lambda_j
    return out


def transform(pre, zt, zp, round32=True):
    """ProbePreprocessor.transform with the stored float32 mean, std and components: float64 arithmetic, then float32 (round32)."""
    x = (design_matrix(zt, zp).astype(np.float64) - pre["mean"].astype(np.float64)) / pre["std"].astype(np.float64)
    if pre.get("comp") is not None:
        dm = zt.shape[1] + zp.shape[1]
        x = np.concatenate([x[:, :dm], x[:, dm:] @ pre["comp"].astype(np.float64)], 1)
    return x.astype(np.float32) if round32 else x


def ridge(pre, zt, zp, Y, lam=RIDGE, round32=False):
    """Pass 2 -> (W float64 [D_out, Cy], b float64 [Cy], cond(A + reg))."""
    xa = np.concatenate([transform(pre, zt, zp, round32).astype(np.float64), np.ones((len(zt), 1))], 1)
    A, B = xa.T @ xa, xa.T @ np.asarray(Y, np.float64)
    reg = np.eye(len(A)) * lam
    reg[-1, -1] = 0.0
    wb = np.linalg.solve(A + reg, B)
    return wb[:-1], wb[-1], float(np.linalg.cond(A + reg))


def two_passes(inp, k=None, lam=RIDGE):
    """The reference's fit on the unmasked rows of a case -> dict(pre, W, b, cond, n, zt, zp, Y, m)."""
    zt, zp, Y, m = flatten(inp)
    if not m.any():
        raise RuntimeError("No valid observations found in training data; cannot fit probe.")
    pre = statistics(zt[m], zp[m], inp["k"] if k is None else k)
    W, b, cond = ridge(pre, zt[m], zp[m], Y[m], lam)
    return dict(pre=pre, W=W, b=b, cond=cond, n=int(m.sum()), zt=zt, zp=zp, Y=Y, m=m)


def predict64(pre, W, b, zt, zp):
    """Predictions in float64 throughout of the stored float32 preprocessor and a model (W, b)."""
    return transform(pre, zt, zp, round32=False) @ np.asarray(W, np.float64) + np.asarray(b, np.float64)


def algebra_tolerances(n, cond, gap, offset_ratio):
    """The 'two algebras' bounds of the module docstring -> dict(eps, turn, solve): relative sizes."""
    eps = 4.0 * U64 * np.sqrt(n) * (1.0 + offset_ratio)
    turn = 4.0 * eps / gap if np.isfinite(gap) else 0.0
    return dict(eps=eps, turn=turn, solve=8.0 * cond * (eps + turn))


# ---------------------------------------------------------------------------------------------------------------------------------
# moments of the pivoted rows, and the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def pivoted_rows(zt, zp, Y, m, pivot):
    """-> (c = [x' | p' | y' | 1] float32 [n, C + 1], q' = x' (x) p' float32 [n, Dq]) of the unmasked rows, formed as the kernel forms them."""
    p = np.asarray(pivot, np.float32)
    dt, dp = zt.shape[1], zp.shape[1]
    xs, ps = zt[m] - p[:dt], zp[m] - p[dt:dt + dp]
    c = np.concatenate([xs, ps, Y[m] - p[dt + dp:], np.ones((int(m.sum()), 1), np.float32)], 1)
    q = (xs[:, :, None] * ps[:, None, :]).reshape(len(xs), -1)
    assert c.dtype == np.float32 and q.dtype == np.float32
    return c, q


def product_moments(v, w):
    """-> (v^T w in float64, its chain-model bound)."""
    v64, w64 = v.astype(np.float64), w.astype(np.float64)
    S = v64.T @ w64
    n = max(len(v), 1)
    return S, 6.0 * U32 * np.sqrt(n) / 3.0 * (np.abs(v64).T @ np.abs(w64)) + 2.0 * U32 * np.abs(S)


def exact_moments(zt, zp, Y, m, pivot):
    """(S, Scq, Sqq) for the exact float64 rows about `pivot` (no float32 subtraction or product): what from_moments is fed on the CPU."""
    p = np.asarray(pivot, np.float64)
    dt, dp = zt.shape[1], zp.shape[1]
    xs, ps = zt[m].astype(np.float64) - p[:dt], zp[m].astype(np.float64) - p[dt:dt + dp]
    c = np.concatenate([xs, ps, Y[m].astype(np.float64) - p[dt + dp:], np.ones((int(m.sum()), 1))], 1)
    # the raw interaction column is the float32 product of the reference; about the pivot it is q - pi_x p' - pi_p x' - pi_x pi_p
    q = design_matrix(zt[m], zp[m])[:, dt + dp:].astype(np.float64).reshape(len(xs), dt, dp)
    q = (q - p[:dt][None, :, None] * ps[:, None, :] - xs[:, :, None] * p[dt:dt + dp][None, None, :]
         - (p[:dt][:, None] * p[dt:dt + dp][None, :])[None]).reshape(len(xs), -1)
    return c.T @ c, c.T @ q, q.T @ q


def pivoted_pred(zt, zp, pivot, beta, u, v, omega):
    """-> (float64 predictions of the float32 model (beta [Cy], u [Cy, Dt], v [Cy, Dp], omega [Cy, Dt, Dp]) about the pivot, from the
    float32 x' and p' the kernel forms; the fmaf-chain bound of the module docstring) [N, Cy] each."""
    p = np.asarray(pivot, np.float32)
    dt, dp = zt.shape[1], zp.shape[1]
    xs, ps = (zt - p[:dt]).astype(np.float64), (zp - p[dt:dt + dp]).astype(np.float64)
    beta, u, v, omega = (np.asarray(t, np.float64) for t in (beta, u, v, omega))
    pred = beta + xs @ u.T + ps @ v.T + np.einsum("ni,cia,na->nc", xs, omega, ps)
    mag = np.abs(beta) + np.abs(xs) @ np.abs(u).T + np.abs(ps) @ np.abs(v).T + np.einsum("ni,cia,na->nc", np.abs(xs), np.abs(omega), np.abs(ps))
    return pred, (2 * dt + 2 * dp + 2) * U32 * mag
