"""Cases, inputs and the float64 restatement for the diagonal-covariance GMM tests (test_cpu_gmm.py, test_gpu_gmm.py).

Inputs are regenerated from numpy's default_rng, never stored; tests/golden/gmm_<case>.npz (tests/golden/make_gmm_golden.py) holds what
sklearn 1.7.2 and the reference's _compute_phase_summary gave for them, and a checksum of the inputs.

The restatement follows sklearn.mixture (_estimate_log_gaussian_prob, _estimate_gaussian_parameters, _m_step and the loop of
BaseMixture.fit for covariance_type="diag"), with row weights added: nk = sum_n w_n r_nk, lower bound = sum w lse / sum w.  Every
function takes `dtype`: float64 is the expected answer, float32 the same loop as an error yardstick.

Seeds.  Whole-fit tests compare n_iter, so a case is used for them only where the float64 lower bound moves by >= 2 tol at the last
iteration that does not stop and by <= tol / 2 at the one that does (tol = 1e-3).  Seeds 0 (case a) and 4 (case e) of the first draft
stop at 5.7e-4 and 8.2e-4; the seeds below were taken as the first ones from 0 upwards that satisfy the rule (test_cpu_gmm.py checks
it for every whole-fit case), and so that the hard-assignment tests exclude far fewer than 1 % of rows.
"""
from __future__ import annotations

import zlib

import numpy as np

EPS10 = 10 * np.finfo(np.float64).eps
U32 = 2.0 ** -24
TOL, REG_COVAR, MAX_ITER = 1e-3, 1e-6, 200

CASES = {
    "a": dict(n=1003, d=3, k=2, sep=3.0, seed=2),      # row and lane tails
    "b": dict(n=2000, d=36, k=5, sep=1.5, seed=6),     # the phase-summary width
    "c": dict(n=4099, d=64, k=17, sep=1.0, seed=10),    # the type width; K not a multiple of 16
    "d": dict(n=700, d=1, k=3, sep=4.0, seed=4),       # one column
    "e": dict(n=3001, d=65, k=7, sep=0.6, seed=2),     # D one past a multiple of 16; overlapping blobs
    "f": dict(n=257, d=128, k=64, sep=1.0, seed=5),    # K D at the limit (single step only)
    "g": dict(n=600, d=64, k=128, sep=1.0, seed=6),    # K at the limit (single step only)
    "h": dict(n=2, d=1, k=1, sep=1.0, seed=7),         # smallest legal fit
    "i": dict(base="b", shift=1000.0),                 # data far from the origin (the pivot)
    "j": dict(base="a", weighted=True, seed=9),        # integer weights 0..3, zeros included
}
STEP_CASES = list("abcdefghij")
FIT_CASES = ["a", "b", "c", "d", "e", "i", "j"]
SCORE_CASES = list("abcde")
HARD_CASES = ["a", "b", "d"]


def blobs(n, d, k, sep, rng):
    centres = rng.normal(0.0, sep, size=(k, d))
    scales = rng.uniform(0.5, 1.5, size=(k, d))
    comp = rng.integers(0, k, size=n)
    return (centres[comp] + rng.normal(size=(n, d)) * scales[comp]).astype(np.float32), comp


def make_inputs(case: str):
    """-> dict(X f32 [N, D], w f32 [N] | None, weights_init, means_init, variances_init (float32), init_rows)."""
    c = CASES[case]
    if "base" in c:
        out = dict(make_inputs(c["base"]))
        if "shift" in c:
            out["X"] = (out["X"] + np.float32(c["shift"])).astype(np.float32)
            out["means_init"] = out["X"][out["init_rows"]].copy()
            out["variances_init"] = np.tile(out["X"].astype(np.float64).var(0), (out["means_init"].shape[0], 1)).astype(np.float32)
        if c.get("weighted"):
            out["w"] = np.random.default_rng(c["seed"]).integers(0, 4, size=out["X"].shape[0]).astype(np.float32)
        return out
    rng = np.random.default_rng(c["seed"])
    X, _ = blobs(c["n"], c["d"], c["k"], c["sep"], rng)
    rows = np.sort(rng.choice(c["n"], size=c["k"], replace=False))
    var = np.tile(X.astype(np.float64).var(0), (c["k"], 1)) + (1.0 if c["n"] < 3 else 0.0)
    return dict(X=X, w=None, init_rows=rows, weights_init=np.full(c["k"], 1.0 / c["k"], np.float32), means_init=X[rows].copy(),
                variances_init=var.astype(np.float32))


def checksum(inp) -> int:
    h = 0
    for key in ("X", "w", "init_rows", "weights_init", "means_init", "variances_init"):
        if inp.get(key) is not None:
            h = zlib.crc32(np.ascontiguousarray(inp[key]).tobytes(), h)
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def log_prob(X, pi, mu, var, dtype=np.float64):
    """lp [N, K] = log pi_k - (D log 2 pi + sum log var + sum (x - mu)^2 / var) / 2, as sklearn expands it for "diag"."""
    X, pi, mu, var = (np.asarray(a, dtype) for a in (X, pi, mu, var))
    prec = dtype(1.0) / var
    q = (mu ** 2 * prec).sum(1) - dtype(2.0) * (X @ (mu * prec).T) + (X ** 2) @ prec.T
    return (dtype(-0.5) * (dtype(X.shape[1] * np.log(2 * np.pi)) + q) + dtype(0.5) * np.log(prec).sum(1) + np.log(pi)).astype(dtype)


def log_prob_direct(X, pi, mu, var):
    """The same in float64 from the differences (x - mu): free of the cancellation of the expanded form; the expected answer."""
    X, pi, mu, var = (np.asarray(a, np.float64) for a in (X, pi, mu, var))
    q = np.stack([(((X - mu[k]) ** 2) / var[k]).sum(1) for k in range(mu.shape[0])], 1)
    return -0.5 * (X.shape[1] * np.log(2 * np.pi) + q + np.log(var).sum(1)) + np.log(pi)


def logsumexp(lp):
    m = lp.max(1, keepdims=True)
    return (m + np.log(np.exp(lp - m).sum(1, keepdims=True)))[:, 0]


def e_step(X, pi, mu, var, dtype=np.float64):
    lp = log_prob_direct(X, pi, mu, var) if dtype == np.float64 else log_prob(X, pi, mu, var, dtype)
    lse = logsumexp(lp)
    return lp, lse, np.exp(lp - lse[:, None])


def m_step(X, w, resp, reg_covar=REG_COVAR, dtype=np.float64):
    """sklearn's _estimate_gaussian_parameters + _m_step for "diag", taken about the column mean (the same algebra, no cancellation)."""
    X = np.asarray(X, dtype)
    rw = resp if w is None else resp * np.asarray(w, dtype)[:, None]
    nk = rw.sum(0) + dtype(EPS10)
    p = X.mean(0, dtype=np.float64).astype(dtype)
    Y = X - p
    m = (rw.T @ Y) / nk[:, None]
    var = (rw.T @ (Y * Y)) / nk[:, None] - m ** 2 + dtype(reg_covar)
    return (nk / nk.sum()).astype(dtype), (m + p).astype(dtype), var.astype(dtype)


def em_step(X, w, pi, mu, var, reg_covar=REG_COVAR, dtype=np.float64):
    """-> (pi, mu, var, lower_bound) after one E and one M step."""
    _, lse, resp = e_step(X, pi, mu, var, dtype)
    lb = lse.mean(dtype=np.float64) if w is None else float((np.asarray(w, np.float64) * lse).sum() / np.asarray(w, np.float64).sum())
    return (*m_step(X, w, resp, reg_covar, dtype), float(lb))


def fit(X, w, pi, mu, var, tol=TOL, reg_covar=REG_COVAR, max_iter=MAX_ITER, dtype=np.float64):
    """The loop of BaseMixture.fit -> dict(weights, means, covariances, n_iter, converged, lower_bounds)."""
    lbs, prev, conv = [], -np.inf, False
    for _ in range(max_iter):
        pi, mu, var, lb = em_step(X, w, pi, mu, var, reg_covar, dtype)
        lbs.append(lb)
        if abs(lb - prev) < tol:
            conv = True
            break
        prev = lb
    return dict(weights=pi, means=mu, covariances=var, n_iter=len(lbs), converged=conv, lower_bounds=np.asarray(lbs))


def stop_margins(lbs):
    """(change at the last iteration that went on, change at the one that stopped)."""
    ch = np.abs(np.diff(lbs))
    return (ch[-2] if len(ch) > 1 else np.inf), ch[-1]


def sq_dist(X, centres):
    X, centres = np.asarray(X, np.float64), np.asarray(centres, np.float64)
    return np.stack([((X - c) ** 2).sum(1) for c in centres], 1)


def lloyd_step(X, w, centres):
    """-> (labels, new centres, float64 gap between the best and the second-best squared distance); empty centres keep their value."""
    d2 = sq_dist(X, centres)
    labels = d2.argmin(1)
    s = np.sort(d2, 1)
    gap = s[:, 1] - s[:, 0] if d2.shape[1] > 1 else np.full(len(d2), np.inf)
    ww = np.ones(len(d2)) if w is None else np.asarray(w, np.float64)
    new = np.array(centres, np.float64)
    for k in range(d2.shape[1]):
        m = ww * (labels == k)
        if m.sum() > 0:
            new[k] = (m[:, None] * np.asarray(X, np.float64)).sum(0) / m.sum()
    return labels, new, gap


def hard_gap_bound(X, centres):
    """Float32 bound on the error of a difference of two squared distances as the kernel forms them: lp_k = a_k + sum_d (-y^2 / 2 + y m_kd)
    about the pivot p, a chain of 2 D fused multiply-adds and one add, each rounding at most u times the largest partial sum
    M_n = max_k (|a_k| + sum_d (y^2 / 2 + |y m_kd|)); the difference of two carries twice that, and distance = -2 lp."""
    X, centres = np.asarray(X, np.float64), np.asarray(centres, np.float64)
    Y, M = X - X.mean(0), centres - X.mean(0)
    mag = 0.5 * (Y ** 2).sum(1)[:, None] + np.abs(Y) @ np.abs(M).T + 0.5 * (M ** 2).sum(1) + 0.5 * X.shape[1] * np.log(2 * np.pi) + np.log(len(M))
    return 2 * 2 * (2 * X.shape[1] + 4) * U32 * mag.max(1)


def kmeans_init(X, w, rows, iters, reg_covar=REG_COVAR):
    """init_rows -> `iters` Lloyd steps -> one M step from the one-hot responsibilities (sklearn's _initialize given labels)."""
    centres = np.asarray(X, np.float64)[rows]
    for _ in range(iters):
        _, centres, _ = lloyd_step(X, w, centres)
    labels = sq_dist(X, centres).argmin(1)
    return m_step(X, w, np.eye(len(rows))[labels], reg_covar)


def n_parameters(k, d):
    return 2 * k * d + k - 1


def bic(X, pi, mu, var):
    lse = logsumexp(log_prob_direct(X, pi, mu, var))
    return -2 * lse.mean() * len(lse) + n_parameters(*mu.shape) * np.log(len(lse))


def aic(X, pi, mu, var):
    lse = logsumexp(log_prob_direct(X, pi, mu, var))
    return -2 * lse.mean() * len(lse) + 2 * n_parameters(*mu.shape)


def phase_summary(z, ysfc, low_max=1.0, high_min=5.0):
    """_compute_phase_summary of the reference's fit_landscape_categories.py in float64."""
    z, y = np.asarray(z, np.float64), np.asarray(ysfc, np.float64)
    mean = z.mean(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        tvar = (((z - mean[:, None]) ** 2).sum(1) / (z.shape[1] - 1)).mean(-1)
        fin = np.isfinite(y)
        out = []
        for m in (fin & (y <= low_max), fin & (y >= high_min)):
            c = (z * m[..., None]).sum(1) / np.maximum(m.sum(1), 1)[:, None]
            out.append(np.where(m.any(1)[:, None], c, mean))
    return np.concatenate(out + [mean], 1), tvar


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 error bounds of one EM step, from the operation count (test_gpu_gmm.py's docstring has the derivation)
# ---------------------------------------------------------------------------------------------------------------------------------
CONF = 6.0   # independent roundings add as a random walk; the largest of ~10^4 outputs stays within 6 standard deviations
RMS = 1.0 / 3.0  # a rounding is uniform within u |partial| (std u |partial| / sqrt 3) and the partial sums grow linearly (rms max / sqrt 3)


def step_bounds(X, w, pi, mu, var):
    """-> dict(mu, var_rel, pi, lb): absolute bounds on means, weights and the lower bound, relative (to the largest variance the step
    gives) on variances."""
    X, pi, mu, var = (np.asarray(a, np.float64) for a in (X, pi, mu, var))
    n, d = X.shape
    ww = np.ones(n) if w is None else np.asarray(w, np.float64)
    p = X.mean(0)
    Y, M = X - p, mu - p
    lp, lse, r = e_step(X, pi, mu, var)
    a = np.log(pi) - 0.5 * (d * np.log(2 * np.pi) + np.log(var).sum(1) + (M ** 2 / var).sum(1))
    mag = np.abs(a) + 0.5 * (Y ** 2) @ (1 / var).T + np.abs(Y) @ np.abs(M / var).T       # [N, K]: the largest partial sum of the chain
    live = r > 1e-7
    d_lp = RMS * U32 * np.sqrt(2 * d + 3) * np.sqrt((mag ** 2 * live).sum() / max(live.sum(), 1))  # rms lp error over pairs that matter
    rw = r * ww[:, None]
    nk = rw.sum(0) + EPS10
    nz = np.maximum((rw > 1e-7 * rw.max()).sum(0), 1)                                   # rows that move an accumulator at all
    # responsibilities: d r_k = r_k (1 - r_k) d lp_k - r_k sum_{j != k} r_j d lp_j, both of size <= r (1 - r) sqrt(2) d_lp
    sens = rw * (1 - r)
    m_new = (rw.T @ Y) / nk[:, None]                                                     # the step's own output, about the pivot
    v_new = (rw.T @ (Y ** 2)) / nk[:, None] - m_new ** 2 + REG_COVAR
    dev = np.stack([np.abs(Y - m_new[k]).max(1) for k in range(len(M))], 1)              # |x - mu_k| per row, largest column
    s1 = np.sqrt(((sens * dev) ** 2).sum(0)) / nk
    s2 = np.sqrt(((sens * np.stack([((Y - m_new[k]) ** 2 + v_new[k]).max(1) for k in range(len(M))], 1)) ** 2).sum(0)) / nk
    s0 = np.sqrt((sens ** 2).sum(0)) / nk
    a1 = (rw.T @ np.abs(Y)).max(1) / nk                                                  # sum r |y| / nk: scale of the S1 chain
    a2 = ((rw.T @ (Y ** 2)) / nk[:, None]).max(1)                                        # sum r y^2 / nk: scale of the S2 chain
    cancel = 2 * np.abs(m_new).max(1)                                                    # var = S2 / nk - m^2: d var = ... - 2 m d m
    chain = RMS * U32 * np.sqrt(nz)
    b_mu = CONF * (np.sqrt(2) * d_lp * s1 + chain * a1).max() + 2 * U32 * np.abs(m_new + p).max() + 2 * U32 * np.abs(m_new).max()
    b_var = (CONF * (np.sqrt(2) * d_lp * (s2 + cancel * s1) + chain * (a2 + cancel * a1)).max()) / v_new.max() + 4 * U32
    b_pi = CONF * ((np.sqrt(2) * d_lp * s0 + chain) * (nk / nk.sum())).max() + 2 * U32
    b_lb = U32 * (np.abs(a).max() + np.abs(lse).max()) + CONF * d_lp / np.sqrt(n)
    return dict(mu=float(b_mu), var_rel=float(b_var), pi=float(b_pi), lb=float(b_lb), d_lp=float(d_lp),
                lp_max=float(CONF * U32 * np.sqrt(2 * d + 3) * (mag * live).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs of the sweep, phase-summary and taxonomy tests
# ---------------------------------------------------------------------------------------------------------------------------------
BIC_K_VALUES = [1, 2, 3, 4, 6]
BIC_N_INIT_FINAL = 3
KMEANS_ITERS = 10
PHASE_SHAPES = [(1, 1, 1), (65, 5, 12), (1001, 15, 12), (65, 15, 64), (65, 1, 12), (1001, 5, 1), (1, 15, 64)]   # (N, T, D)


def init_rows_for(n, k, n_init, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(n, size=k, replace=False)) for _ in range(n_init)]).astype(np.int64)


def make_bic_inputs():
    """Three well-separated blobs, N = 1500, D = 8, sep = 6; init rows for every (K, n_init) of the sweep and the refit."""
    rng = np.random.default_rng(21)
    X, _ = blobs(1500, 8, 3, 6.0, rng)
    rows = {(k, 1): init_rows_for(1500, k, 1, 100 + k) for k in BIC_K_VALUES}
    rows.update({(k, BIC_N_INIT_FINAL): init_rows_for(1500, k, BIC_N_INIT_FINAL, 200 + k) for k in BIC_K_VALUES})
    return X, rows


def make_phase_inputs(shape):
    """z_phase [N, T, D] and ysfc [N, T] mixing NaN, <= 1, >= 5 and in-between values; rows 0 mod 3 have no disturbed timestep and rows
    1 mod 3 no recovered one (where T allows anything else), so both fallbacks run."""
    n, t, d = shape
    rng = np.random.default_rng(1000 * n + 10 * t + d)
    z = rng.normal(size=shape).astype(np.float32)
    y = rng.choice(np.array([np.nan, 0.0, 1.0, 2.5, 5.0, 9.0, -1.0, np.inf], np.float32), size=(n, t))
    r = np.arange(n)
    y[r % 3 == 0] = np.where(y[r % 3 == 0] <= 1.0, np.float32(3.0), y[r % 3 == 0])
    y[r % 3 == 1] = np.where(y[r % 3 == 1] >= 5.0, np.float32(np.nan), y[r % 3 == 1])
    return z, y.astype(np.float32)


def make_taxonomy_inputs():
    """Three type blobs of 1200 rows (D = 8, far apart); the rows of the last one carry two far-apart phase-summary blobs (D = 6), the
    others one."""
    rng = np.random.default_rng(33)
    centres = np.array([[-8.0] * 8, [0.0] * 8, [8.0] * 8])
    comp = np.repeat(np.arange(3), 1200)
    z = (centres[comp] + rng.normal(size=(3600, 8))).astype(np.float32)
    s = rng.normal(size=(3600, 6))
    s[(comp == 2) & (rng.random(3600) < 0.5)] += 7.0
    perm = rng.permutation(3600)
    return z[perm], s[perm].astype(np.float32)


TAXONOMY = dict(k_type_values=[2, 3, 4], k_phase_max=3, min_cluster_pixels=1000, n_init_sweep=1, n_init_final=2, seed=42)
