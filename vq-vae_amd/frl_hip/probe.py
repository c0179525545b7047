"""Closed-form linear probes on the GPU: the streamed ridge fit and the evaluation of the reference's frl/training/fit_linear_probe.py
(z_type against five static metrics) and fit_phase_linear_probe.py (z_type and z_phase against per-year targets).

`RidgeProbe.partial_fit` adds one batch into a device-resident moment state with one pass of csrc/probe.hip over the latents as they
sit in memory (channels-last; a channels-first tensor whose channels-last permutation is contiguous is used in place): no gathered
copy, no ones column, no float64 matmul.  The state is S = v^T v for v = [x - p_x | y - p_y | m] (p: a pivot fixed on the first batch)
and the integer count n, from which `solve()` forms in float64
    Sigma = S_vv - s s^T / n,   W = (Sigma_xx + lambda I)^-1 Sigma_xy,   b = ybar - xbar^T W,
the minimiser of the reference's ||X W + b - Y||^2 + lambda ||W||^2 (its penalty leaves the bias row out).  The column means and
standard deviations of the reference's ProbePreprocessor come out of the same moments, so its two passes over the training split are
one here (`standardize=True`).  `partial_evaluate` is one fused pass as well: predictions as a float32 fmaf chain, error sums in double.

`InteractionProbe` is the phase script's default design "full", [z_type | z_phase | z_type (x) z_phase] with a PCA of the interaction
block, over csrc/probe_full.hip: the same pass also accumulates the moments of the pivoted interaction, and statistics, PCA, ridge
fit and the model for the fused evaluation follow on the host in float64 (see the class).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

__all__ = ["RidgeProbe", "ProbeMetrics", "TARGET_METRICS", "DESIGN_CHOICES", "halo_mask", "spearman_rho2", "design_features", "design_dim",
           "fit_closed_form_ridge", "evaluate_probe", "fit_phase_probe", "InteractionProbe", "fit_phase_probe_full", "full_design_dim"]

TARGET_METRICS = [
    "static.mean_ndvi",
    "static.mean_ndmi",
    "static.mean_nbr",
    "static.mean_seasonal_amp_nir",
    "static.variance_ndvi",
]
DESIGN_CHOICES = ("full", "additive", "type-only", "phase-only")


@dataclass
class ProbeMetrics:
    mse_per_metric: Dict[str, float]
    r2_per_metric: Dict[str, float]
    spearman_rho2_per_metric: Dict[str, float]
    mse_total: float
    r2_total: float
    spearman_rho2_total: float
    n_pixels: int


def halo_mask(H: int, W: int, halo: int, device=None) -> torch.Tensor:
    """[H, W] bool, True for pixels at least `halo` from every edge; all False where nothing survives."""
    mask = torch.zeros(H, W, dtype=torch.bool, device=device)
    if 2 * halo >= H or 2 * halo >= W:
        return mask
    mask[halo:H - halo, halo:W - halo] = True
    return mask


def spearman_rho2(pred: torch.Tensor, target: torch.Tensor) -> float:
    """Spearman's rank correlation squared of two 1-D tensors: double ranks by argsort of argsort, on the tensors' device."""
    n = pred.shape[0]
    if n < 2:
        return 0.0
    pr = pred.double().argsort().argsort().double()
    tr = target.double().argsort().argsort().double()
    p = pr - pr.mean()
    t = tr - tr.mean()
    num = (p * t).sum()
    den = torch.sqrt((p * p).sum() * (t * t).sum())
    if den < 1e-12:
        return 0.0
    return float((num / den).item() ** 2)


def design_dim(design: str, d_type: int, d_phase: int) -> int:
    """The number of feature columns of a phase-probe design."""
    _check_design(design)
    return {"type-only": d_type, "phase-only": d_phase, "additive": d_type + d_phase}[design]


def design_features(design: str, z_type, z_phase):
    """The sources of a design: z_type, z_phase or the pair (the two are never concatenated)."""
    _check_design(design)
    return {"type-only": z_type, "phase-only": z_phase, "additive": (z_type, z_phase)}[design]


def _check_design(design: str):
    if design == "full":
        raise NotImplementedError("probe: design='full' (the interaction columns with PCA) has entry points of its own: InteractionProbe, "
                                  "fit_phase_probe_full and full_design_dim; here use 'additive', 'type-only' or 'phase-only'")
    if design not in DESIGN_CHOICES:
        raise ValueError(f"probe: design must be one of {DESIGN_CHOICES}, got {design!r}")


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor, channels_last: bool, what: str):
    """-> (tensor [B, T_s, P, C] float32 contiguous, (H, W)).  Channels-first [B, C, H, W] / [B, C, T, H, W] as the reference passes
    them, or channels-last [B, H, W, C] / [B, T, H, W, C]; a channels-last view that is already contiguous is used in place."""
    if not isinstance(t, torch.Tensor) or t.dim() not in (4, 5):
        raise ValueError(f"probe: {what} must be a 4-D or 5-D tensor, got {type(t).__name__} {tuple(getattr(t, 'shape', ()))}")
    if t.dtype != torch.float32:
        raise ValueError(f"probe: {what} must be float32, got {t.dtype}")
    if not channels_last:
        t = t.permute(0, 2, 3, 1) if t.dim() == 4 else t.permute(0, 2, 3, 4, 1)
    if not t.is_contiguous():
        t = t.contiguous()                                                       # the one channels-last copy
    if t.dim() == 4:
        b, h, w, c = t.shape
        return t.view(b, 1, h * w, c), (h, w)
    b, ts, h, w, c = t.shape
    return t.view(b, ts, h * w, c), (h, w)


def _mask_rows(mask: torch.Tensor, hw, halo: int) -> torch.Tensor:
    if not isinstance(mask, torch.Tensor) or mask.dim() != 3 or tuple(mask.shape[1:]) != tuple(hw):
        raise ValueError(f"probe: mask must be [B, H, W] = [B, {hw[0]}, {hw[1]}], got {tuple(getattr(mask, 'shape', ()))}")
    m = mask if mask.dtype == torch.bool else mask != 0
    if halo:
        m = m & halo_mask(hw[0], hw[1], int(halo), m.device).unsqueeze(0)
    return m.contiguous().view(torch.uint8).view(m.shape[0], hw[0] * hw[1])


def _sources(features, channels_last: bool):
    fs = tuple(features) if isinstance(features, (tuple, list)) else (features,)
    if not 1 <= len(fs) <= 2:
        raise ValueError(f"probe: features must be a tensor or a pair of tensors, got {len(fs)}")
    out = [_rows(f, channels_last, "features") for f in fs]
    if any(o[1] != out[0][1] for o in out):
        raise ValueError("probe: the feature sources differ in H, W")
    a, bs = out[0][0], out[1][0] if len(out) == 2 else None
    d = a.shape[3] + (0 if bs is None else bs.shape[3])
    if d > ops.PROBE_MAX_D:
        raise ValueError(f"probe: supports D <= {ops.PROBE_MAX_D} feature columns, got {d}")
    return a, bs, out[0][1]


class RidgeProbe:
    """A streamed closed-form ridge probe; see the module docstring."""

    def __init__(self, ridge_lambda: float = 1e-3, standardize: bool = False, workgroups: int = 0):
        ops.chk_workgroups("RidgeProbe", workgroups, hint="")
        self.ridge_lambda, self.standardize, self.workgroups = float(ridge_lambda), bool(standardize), int(workgroups)
        self._S = self._n = self._pivot = self._ws = None                        # device state of the fit
        self._moments = None                                                     # (S, n, pivot) on the host, float64
        self._d = self._cy = None
        self._E = self._en = None
        self._pairs = []
        self._rank = True

    # ---- construction without a GPU ---------------------------------------------------------------------------------------------
    @classmethod
    def from_moments(cls, S, n: int, pivot, n_targets: int, ridge_lambda: float = 1e-3, standardize: bool = False, **kw) -> "RidgeProbe":
        """A probe from moments S [C+1, C+1] = v^T v of v = [x - p_x | y - p_y | 1], the count n and the pivot [C]; needs no GPU."""
        S = torch.as_tensor(np.asarray(S, np.float64))
        pivot = torch.as_tensor(np.asarray(pivot, np.float64))
        c = pivot.numel()
        if S.shape != (c + 1, c + 1) or not 1 <= int(n_targets) < c:
            raise ValueError(f"RidgeProbe.from_moments: expected S [C+1, C+1] and pivot [C] with C > n_targets, got {tuple(S.shape)}, {c}, {n_targets}")
        ops.chk_probe_dims(c - int(n_targets), int(n_targets), 0, "RidgeProbe.from_moments")
        g = cls(ridge_lambda, standardize, **kw)
        g._d, g._cy = c - int(n_targets), int(n_targets)
        g._moments = (S, int(n), pivot)
        return g

    # ---- fit --------------------------------------------------------------------------------------------------------------------
    def _prepare(self, features, targets, mask, halo, channels_last, name):
        a, bs, hw = _sources(features, channels_last)
        y, hwy = _rows(targets, channels_last, "targets")
        if hwy != hw:
            raise ValueError(f"{name}: features and targets differ in H, W: {hw} and {hwy}")
        m = _mask_rows(mask, hw, halo)
        if m.device != a.device:
            m = m.to(a.device)
        dims = self._chk(a, bs, y, m, name)
        d, cy = dims[3] + dims[4], dims[5]
        if self._d is None:
            self._d, self._cy = d, cy
        elif (d, cy) != (self._d, self._cy):
            raise ValueError(f"{name}: this probe has D = {self._d}, Cy = {self._cy}; got D = {d}, Cy = {cy}")
        if self._ws is None or self._ws.device != a.device:
            self._ws = self._new_workspace(a.device)
        return a, bs, y, m

    # what a subclass with kernels of its own replaces
    def _chk(self, a, bs, y, m, name):
        return ops.chk_probe(a, bs, y, m, self.workgroups, name)

    def _new_workspace(self, device):
        return ops.probe_workspace(self._d, self._cy, device, self.workgroups)

    def _run_evaluate(self, a, bs, y, m, model, e, n, ws, want_pred):
        pivot, wc, bc = model
        return ops.probe_evaluate(a, bs, y, m, pivot, wc, bc, e, n, ws, want_pred=want_pred, workgroups=self.workgroups)

    def partial_fit(self, features, targets, mask, halo: int = 0, channels_last: bool = False) -> "RidgeProbe":
        a, bs, y, m = self._prepare(features, targets, mask, halo, channels_last, "RidgeProbe.partial_fit")
        if self._S is None:
            c = self._d + self._cy
            self._S = torch.zeros(c + 1, c + 1, dtype=torch.float64, device=a.device)
            self._n = torch.zeros(1, dtype=torch.int64, device=a.device)
            self._seeded = False
        if not self._seeded:                                                     # the first batch with a valid pixel fixes the pivot
            self._pivot = ops.probe_pivot(a, bs, y, m, self._ws)
        ops.probe_accumulate(a, bs, y, m, self._pivot, self._S, self._n, self._ws, self.workgroups)
        if not self._seeded:
            self._seeded = int(self._n.item()) > 0                               # one host read per batch until then
        self._moments = None
        if hasattr(self, "coef_"):
            del self.coef_
        return self

    def moments(self):
        """-> (S [C+1, C+1], n, pivot [C]) in float64 on the host."""
        if self._moments is None:
            if self._S is None:
                raise RuntimeError("No valid pixels found in training data; cannot fit probe.")
            self._moments = (self._S.cpu(), int(self._n.item()), self._pivot.double().cpu())
        return self._moments

    def solve(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (W [D, Cy] float32, b [Cy] float32); with standardize=True for the standardised columns (x - mean_) / std_."""
        S, n, pivot = self.moments()
        if n == 0:
            raise RuntimeError("No valid pixels found in training data; cannot fit probe.")
        d, c = self._d, self._d + self._cy
        s = S[:c, c]
        cov = S[:c, :c] - torch.outer(s, s) / n
        mean = pivot + s / n
        sxx, sxy = cov[:d, :d], cov[:d, d:]
        xbar, ybar = mean[:d], mean[d:]
        eye = torch.eye(d, dtype=torch.float64)
        if self.standardize:
            var = torch.diagonal(sxx) / n
            self.mean_ = xbar.to(torch.float32)
            self.std_ = var.clamp(min=1e-16).sqrt().to(torch.float32)
            sd = self.std_.double()
            w = torch.linalg.solve(sxx / sd[:, None] / sd[None, :] + self.ridge_lambda * eye, sxy / sd[:, None])
            # the mean of a standardised column is what the rounding of mean_ leaves: formed from the small parts, not from xbar
            b = ybar - (((pivot[:d] - self.mean_.double()) + s[:d] / n) / sd) @ w
        else:
            self.mean_, self.std_ = xbar.to(torch.float32), (torch.diagonal(sxx) / n).clamp(min=1e-16).sqrt().to(torch.float32)
            w = torch.linalg.solve(sxx + self.ridge_lambda * eye, sxy)
            b = ybar - xbar @ w
        self.coef64_, self.intercept64_ = w, b                                   # before the rounding to the reference's float32
        self.coef_, self.intercept_, self.n_obs_ = w.to(torch.float32), b.to(torch.float32), n
        return self.coef_, self.intercept_

    def set_model(self, W: torch.Tensor, b: torch.Tensor, pivot=None, mean=None, std=None) -> "RidgeProbe":
        """Takes (W, b) from elsewhere (the reference's checkpoint) for evaluation; mean and std as its preprocessor stores them."""
        W, b = torch.as_tensor(W).detach().cpu().to(torch.float32), torch.as_tensor(b).detach().cpu().to(torch.float32)
        if W.dim() != 2 or b.shape != (W.shape[1],):
            raise ValueError(f"RidgeProbe.set_model: expected W [D, Cy] and b [Cy], got {tuple(W.shape)} and {tuple(b.shape)}")
        ops.chk_probe_dims(W.shape[0], W.shape[1], 0, "RidgeProbe.set_model")
        self._d, self._cy = W.shape
        self.coef_, self.intercept_ = W, b
        self.standardize = mean is not None
        if mean is not None:
            self.mean_, self.std_ = torch.as_tensor(mean).cpu().to(torch.float32), torch.as_tensor(std).cpu().to(torch.float32)
        if pivot is not None:
            self._model_pivot = torch.as_tensor(pivot).cpu().to(torch.float32)
        return self

    # ---- evaluation -------------------------------------------------------------------------------------------------------------
    def pivoted_model(self, device=None):
        """-> (pivot [C], Wc [D, Cy], bc [Cy]) float32: the model on pivoted features, pred = bc + (x - pivot_x) Wc."""
        if not hasattr(self, "coef_"):
            self.solve()
        d, cy = self._d, self._cy
        if self._pivot is not None:
            pivot = self._pivot.detach().cpu()
        elif self._moments is not None:
            pivot = self._moments[2].to(torch.float32)
        else:
            pivot = getattr(self, "_model_pivot", torch.zeros(d + cy, dtype=torch.float32))
        w, b, px = self.coef_.double(), self.intercept_.double(), pivot[:d].double()
        if self.standardize:
            mu, sd = self.mean_.double(), self.std_.double()
            wc = w / sd[:, None]
            bc = b + ((px - mu) / sd) @ w
        else:
            wc, bc = w, b + px @ w
        out = (pivot, wc.to(torch.float32).contiguous(), bc.to(torch.float32).contiguous())
        return tuple(t.to(device) for t in out) if device is not None else out

    def _eval_state(self, a, bs, y, m):
        if self._E is None:
            if self._pivot is None and self._moments is None and not hasattr(self, "_model_pivot"):
                self._model_pivot = ops.probe_pivot(a, bs, y, m, self._ws).cpu()  # a model from elsewhere: the first batch's means serve
            self._E = torch.zeros(self._cy, 3, dtype=torch.float64, device=a.device)
            self._en = torch.zeros(1, dtype=torch.int64, device=a.device)
            self._eval_model = self.pivoted_model(a.device)
            self._pairs = []

    def reset_evaluation(self) -> None:
        self._E = self._en = None
        self._pairs = []

    def partial_evaluate(self, features, targets, mask, halo: int = 0, channels_last: bool = False, rank: bool = True) -> "RidgeProbe":
        """Adds one batch into the error sums.  rank=False leaves Spearman's rho^2 out: no prediction is written and tiles without a
        valid pixel are skipped."""
        a, bs, y, m = self._prepare(features, targets, mask, halo, channels_last, "RidgeProbe.partial_evaluate")
        self._eval_state(a, bs, y, m)
        pred = self._run_evaluate(a, bs, y, m, self._eval_model, self._E, self._en, self._ws, rank)
        self._rank = self._rank and rank
        if rank:
            b, t, p, cy = pred.shape
            sel = m.bool().unsqueeze(1).expand(b, t, p)
            self._pairs.append((pred[sel], y.expand(b, t, p, cy)[sel]))
        return self

    def evaluation_sums(self):
        """-> (E float64 [Cy, 3] = SSE | sum (y - q) | sum (y - q)^2 with q the target pivot, n) of what was evaluated so far."""
        if self._E is None:
            raise RuntimeError("RidgeProbe.evaluation_sums: nothing was evaluated")
        return self._E.cpu().numpy(), int(self._en.item())

    def metrics(self, target_names: Optional[Sequence[str]] = None) -> ProbeMetrics:
        names = list(TARGET_METRICS if target_names is None else target_names)
        if self._E is None:
            raise RuntimeError("RidgeProbe.metrics: nothing was evaluated")
        if len(names) != self._cy:
            raise ValueError(f"RidgeProbe.metrics: {len(names)} names for {self._cy} targets")
        E, n = self._E.cpu().numpy(), int(self._en.item())
        mse, r2, rho = {}, {}, {}
        if n and self._rank and self._pairs:
            P, Y = torch.cat([p for p, _ in self._pairs]), torch.cat([y for _, y in self._pairs])
        for i, name in enumerate(names):
            if n == 0:
                mse[name] = r2[name] = rho[name] = 0.0
                continue
            sse, sy, sy2 = (float(v) for v in E[i])
            mse[name] = sse / n
            sst = max(0.0, sy2 - sy * sy / n)
            r2[name] = 1.0 - sse / sst if sst > 1e-8 else 0.0
            rho[name] = spearman_rho2(P[:, i], Y[:, i]) if self._rank and self._pairs else 0.0
        return ProbeMetrics(mse, r2, rho, float(np.mean([mse[k] for k in names])), float(np.mean([r2[k] for k in names])),
                            float(np.mean([rho[k] for k in names])), n)

    def predict(self, features, channels_last: bool = False) -> torch.Tensor:
        """-> predictions [B, T, H, W, Cy] (T dropped for static features) float32 of every pixel."""
        a, bs, hw = _sources(features, channels_last)
        if not a.is_cuda:
            raise _lib.FrlHipError("RidgeProbe.predict: tensors must live on the GPU (no CPU fallback)")
        model = self.pivoted_model(a.device)
        b, p = a.shape[0], a.shape[2]
        cy = self._cy
        y = torch.zeros(b, 1, p, cy, dtype=torch.float32, device=a.device)
        m = torch.ones(b, p, dtype=torch.uint8, device=a.device)
        ws = self._new_workspace(a.device)
        e, n = torch.zeros(cy, 3, dtype=torch.float64, device=a.device), torch.zeros(1, dtype=torch.int64, device=a.device)
        pred = self._run_evaluate(a, bs, y, m, model, e, n, ws, True)
        t = pred.shape[1]
        return pred.view(b, hw[0], hw[1], cy) if t == 1 else pred.view(b, t, hw[0], hw[1], cy)


# ---- the "full" design: [z_type | z_phase | z_type (x) z_phase], the interaction block through a PCA -------------------------------
def full_design_dim(d_type: int, d_phase: int, interaction_pca_k: int = 0) -> int:
    """The columns the "full" design hands the ridge fit: the main effects and the interaction block, or its k components."""
    dq = int(d_type) * int(d_phase)
    return int(d_type) + int(d_phase) + (min(int(interaction_pca_k), dq) if interaction_pca_k > 0 else dq)


class InteractionProbe(RidgeProbe):
    """The reference's default phase probe (fit_phase_linear_probe.py, design="full", interaction_pca_k=20) in one pass.

    `partial_fit((z_type, z_phase), targets, mask)` adds a batch into the moments of [c | q'], c = [x' | p' | y' | 1] and q' = x' (x) p'
    about the pivot of the first batch: S = c^T c and n by frl_probe_accumulate, Scq = c^T q' and Sqq = q'^T q' by
    frl_probe_full_accumulate; the interaction columns never exist in memory.  `solve()` is float64 algebra on the host:
      1. the raw row [x | p | q | y] is L [c | q'] for a matrix L of the pivot (q_ia = q'_ia + pi_x,i p'_a + pi_p,a x'_i + pi_x,i pi_p,a),
         so its mean is L m and its covariance L (S_all / n - m m^T) L^T, m the mean of [c | q'];
      2. pass 1 of the reference: mean, std = sqrt(clamp(var, 1e-16)) over all Dt + Dp + Dt Dp columns, the eigenvectors of the
         standardised interaction covariance scaled to unit variance, all stored in float32;
      3. pass 2 without a second pass: the preprocessed row is z = G (f - mean_) with G built from the stored float32 std_ and
         pca_components_, so W = (n G Cov_ff G^T + lambda I)^-1 n G Cov_fy and b = ybar - zbar W, the minimiser of the reference's
         normal equations (no penalty on the bias) for what ProbePreprocessor.transform computes from the stored values.  Its float32
         rounding of the transformed columns is not reproduced.
    `partial_evaluate` folds W, b and the preprocessor into pred = beta + x' u + p' v + x'^T Omega p' about the pivot (float64, then
    rounded) and runs frl_probe_full_evaluate."""

    def __init__(self, ridge_lambda: float = 1e-3, interaction_pca_k: int = 20, workgroups: int = 0):
        super().__init__(ridge_lambda, True, workgroups)
        if int(interaction_pca_k) < 0:
            raise ValueError(f"InteractionProbe: interaction_pca_k must be >= 0 (0: no PCA), got {interaction_pca_k}")
        self.interaction_pca_k = int(interaction_pca_k)
        self._dt = self._dp = self._Scq = self._Sqq = None

    @classmethod
    def from_moments(cls, S, Scq, Sqq, n: int, pivot, d_type: int, d_phase: int, ridge_lambda: float = 1e-3, interaction_pca_k: int = 20,
                     **kw) -> "InteractionProbe":
        """A probe from S [C+1, C+1] = c^T c, Scq [C+1, Dq] = c^T q', Sqq [Dq, Dq] = q'^T q', the count n and the pivot [C]; needs no GPU."""
        S, Scq, Sqq, pivot = (torch.as_tensor(np.asarray(v, np.float64)) for v in (S, Scq, Sqq, pivot))
        dt, dp = int(d_type), int(d_phase)
        c, dq = pivot.numel(), dt * dp
        ops.chk_probe_full_dims(dt, dp, max(c - dt - dp, 0), 0, "InteractionProbe.from_moments")
        if S.shape != (c + 1, c + 1) or Scq.shape != (c + 1, dq) or Sqq.shape != (dq, dq):
            raise ValueError(f"InteractionProbe.from_moments: expected S [C+1, C+1], Scq [C+1, Dq], Sqq [Dq, Dq] with C = {c}, Dq = {dq}, got "
                             f"{tuple(S.shape)}, {tuple(Scq.shape)}, {tuple(Sqq.shape)}")
        g = cls(ridge_lambda, interaction_pca_k, **kw)
        g._dt, g._dp, g._d, g._cy = dt, dp, dt + dp, c - dt - dp
        g._moments = (S, Scq, Sqq, int(n), pivot)
        return g

    # ---- the hooks of RidgeProbe ------------------------------------------------------------------------------------------------
    def _chk(self, a, bs, y, m, name):
        name = name.replace("RidgeProbe", "InteractionProbe")
        dims = ops.chk_probe_full(a, bs, y, m, self.workgroups, name)
        if self._dt is None:
            self._dt, self._dp = dims[3], dims[4]
        elif (dims[3], dims[4]) != (self._dt, self._dp):
            raise ValueError(f"{name}: this probe has Dt = {self._dt}, Dp = {self._dp}; got Dt = {dims[3]}, Dp = {dims[4]}")
        return dims

    def _new_workspace(self, device):
        return ops.probe_full_workspace(self._dt, self._dp, self._cy, device, self.workgroups)

    def _run_evaluate(self, a, bs, y, m, model, e, n, ws, want_pred):
        pivot, beta, u, v, omega = model
        return ops.probe_full_evaluate(a, bs, y, m, pivot, beta, u, v, omega, e, n, ws, want_pred=want_pred, workgroups=self.workgroups)

    # ---- fit --------------------------------------------------------------------------------------------------------------------
    def partial_fit(self, features, targets, mask, halo: int = 0, channels_last: bool = False) -> "InteractionProbe":
        a, bs, y, m = self._prepare(features, targets, mask, halo, channels_last, "InteractionProbe.partial_fit")
        if self._S is None:
            c, dq = self._d + self._cy, self._dt * self._dp
            self._S = torch.zeros(c + 1, c + 1, dtype=torch.float64, device=a.device)
            self._Scq = torch.zeros(c + 1, dq, dtype=torch.float64, device=a.device)
            self._Sqq = torch.zeros(dq, dq, dtype=torch.float64, device=a.device)
            self._n = torch.zeros(1, dtype=torch.int64, device=a.device)
            self._seeded = False
        if not self._seeded:                                                     # the first batch with a valid pixel fixes the pivot
            self._pivot = ops.probe_pivot(a, bs, y, m, self._ws)
        ops.probe_accumulate(a, bs, y, m, self._pivot, self._S, self._n, self._ws, self.workgroups)
        ops.probe_full_accumulate(a, bs, y, m, self._pivot, self._Scq, self._Sqq, self._ws, self.workgroups)
        if not self._seeded:
            self._seeded = int(self._n.item()) > 0                               # one host read per batch until then
        self._moments = None
        if hasattr(self, "coef_"):
            del self.coef_
        return self

    def moments(self):
        """-> (S [C+1, C+1], Scq [C+1, Dq], Sqq [Dq, Dq], n, pivot [C]) in float64 on the host."""
        if self._moments is None:
            if self._S is None:
                raise RuntimeError("No valid observations found in training data; cannot fit probe.")
            self._moments = (self._S.cpu(), self._Scq.cpu(), self._Sqq.cpu(), int(self._n.item()), self._pivot.double().cpu())
        return self._moments

    def _raw_map(self, pivot: torch.Tensor) -> torch.Tensor:
        """L [Dt + Dp + Dq + Cy, C + 1 + Dq]: [x | p | q | y] = L [x' | p' | y' | 1 | q']."""
        dt, dp, cy = self._dt, self._dp, self._cy
        dm, dq = dt + dp, dt * dp
        one = dm + cy
        L = torch.zeros(dm + dq + cy, one + 1 + dq, dtype=torch.float64)
        idx = torch.arange(dm)
        L[idx, idx] = 1.0
        L[:dm, one] = pivot[:dm]
        iy = torch.arange(cy)
        L[dm + dq + iy, dm + iy] = 1.0
        L[dm + dq:, one] = pivot[dm:]
        i, a = torch.arange(dq) // dp, torch.arange(dq) % dp
        rows = dm + torch.arange(dq)
        L[rows, one + 1 + torch.arange(dq)] = 1.0
        L[rows, dt + a] = pivot[i]
        L[rows, i] = pivot[dt + a]
        L[rows, one] = pivot[i] * pivot[dt + a]
        return L

    def _design_map(self) -> torch.Tensor:
        """G [D_out, Dt + Dp + Dq] float64 of the stored float32 values: ProbePreprocessor.transform is z = G (f - mean_)."""
        dm = self._dt + self._dp
        inv = 1.0 / self.std_.double()
        if self.pca_components_ is None:
            return torch.diag(inv)
        k = self.pca_components_.shape[1]
        G = torch.zeros(dm + k, inv.numel(), dtype=torch.float64)
        G[:dm, :dm] = torch.diag(inv[:dm])
        G[dm:, dm:] = self.pca_components_.double().T * inv[dm:][None, :]
        return G

    def solve(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (W [D_out, Cy] float32, b [Cy] float32) for the rows ProbePreprocessor.transform makes of mean_, std_, pca_components_."""
        S, Scq, Sqq, n, pivot = self.moments()
        if n == 0:
            raise RuntimeError("No valid observations found in training data; cannot fit probe.")
        dt, dp = self._dt, self._dp
        dm, dq = dt + dp, dt * dp
        nf, one = dm + dq, dm + self._cy
        sall = torch.cat([torch.cat([S, Scq], 1), torch.cat([Scq.T, Sqq], 1)], 0)
        mw = sall[:, one] / n
        L = self._raw_map(pivot)
        mean = L @ mw
        cov = L @ (sall / n - torch.outer(mw, mw)) @ L.T
        cov = 0.5 * (cov + cov.T)
        std = torch.diagonal(cov)[:nf].clamp(min=1e-16).sqrt()
        self.mean_, self.std_ = mean[:nf].to(torch.float32), std.to(torch.float32)
        k = min(self.interaction_pca_k, dq)
        self.pca_components_ = self.pca_explained_variance_ratio_ = None
        if k > 0:
            inv = 1.0 / std[dm:]
            eigvals, eigvecs = torch.linalg.eigh(inv[:, None] * cov[dm:nf, dm:nf] * inv[None, :])
            top_vecs, top_vals = eigvecs[:, -k:].flip(dims=[1]), eigvals[-k:].flip(dims=[0])
            self.pca_components_ = (top_vecs / top_vals.clamp(min=1e-12).sqrt().unsqueeze(0)).to(torch.float32)
            self.pca_explained_variance_ratio_ = (top_vals.clamp(min=0.0) / eigvals.clamp(min=0.0).sum()).to(torch.float32)
        G = self._design_map()
        szz, szy = n * (G @ cov[:nf, :nf] @ G.T), n * (G @ cov[:nf, nf:])
        w = torch.linalg.solve(szz + self.ridge_lambda * torch.eye(G.shape[0], dtype=torch.float64), szy)
        # the mean of a transformed column is what the rounding of mean_ leaves
        b = mean[nf:] - (G @ (mean[:nf] - self.mean_.double())) @ w
        self.coef64_, self.intercept64_ = w, b
        self.coef_, self.intercept_, self.n_obs_ = w.to(torch.float32), b.to(torch.float32), n
        return self.coef_, self.intercept_

    @property
    def output_dim(self) -> int:
        k = 0 if getattr(self, "pca_components_", None) is None else self.pca_components_.shape[1]
        return full_design_dim(self._dt, self._dp, k)

    def preprocessor_dict(self) -> dict:
        """The keys of the reference's ProbePreprocessor.to_dict; interaction_pca_k is the number of components kept."""
        if not hasattr(self, "mean_"):
            self.solve()
        pca = self.pca_components_
        return {"preprocessor_mean": self.mean_, "preprocessor_std": self.std_, "preprocessor_pca_components": pca,
                "preprocessor_interaction_pca_k": 0 if pca is None else int(pca.shape[1]), "preprocessor_design": "full",
                "preprocessor_pca_explained_variance_ratio": self.pca_explained_variance_ratio_, "preprocessor_d_type": self._dt,
                "preprocessor_d_phase": self._dp}

    def transform(self, z_type_flat: torch.Tensor, z_phase_flat: torch.Tensor) -> torch.Tensor:
        """What the reference's ProbePreprocessor.transform computes of z_type [N, Dt] and z_phase [N, Dp] -> float32 [N, D_out]: stock
        torch, kept for checking and for callers of the reference's predict."""
        if not hasattr(self, "mean_"):
            self.solve()
        q = (z_type_flat.unsqueeze(2) * z_phase_flat.unsqueeze(1)).reshape(z_type_flat.shape[0], -1)
        x = (torch.cat([z_type_flat, z_phase_flat, q], dim=1).double() - self.mean_.double()) / self.std_.double()
        if self.pca_components_ is None:
            return x.float()
        dm = self._dt + self._dp
        return torch.cat([x[:, :dm], x[:, dm:] @ self.pca_components_.double()], dim=1).float()

    def set_model(self, W, b, mean, std, pca_components=None, pca_explained_variance_ratio=None, d_type: int = 64, d_phase: int = 12,
                  pivot=None) -> "InteractionProbe":
        """Takes (W, b) and the preprocessor of a reference checkpoint for evaluation."""
        f32 = lambda t: torch.as_tensor(t).detach().cpu().to(torch.float32)         # noqa: E731
        W, b, mean, std = f32(W), f32(b), f32(mean), f32(std)
        dt, dp = int(d_type), int(d_phase)
        ops.chk_probe_full_dims(dt, dp, W.shape[1] if W.dim() == 2 else 0, 0, "InteractionProbe.set_model")
        nf = dt + dp + dt * dp
        pca = None if pca_components is None else f32(pca_components)
        dout = dt + dp + (dt * dp if pca is None else pca.shape[-1])
        if W.dim() != 2 or W.shape[0] != dout or b.shape != (W.shape[1],) or mean.shape != (nf,) or std.shape != (nf,) or \
                (pca is not None and (pca.dim() != 2 or pca.shape[0] != dt * dp)):
            raise ValueError(f"InteractionProbe.set_model: expected W [{dout}, Cy], b [Cy], mean and std [{nf}], pca_components [{dt * dp}, k], got "
                             f"{tuple(W.shape)}, {tuple(b.shape)}, {tuple(mean.shape)}, {tuple(std.shape)}")
        self._dt, self._dp, self._d, self._cy = dt, dp, dt + dp, W.shape[1]
        self.coef_, self.intercept_, self.mean_, self.std_, self.pca_components_ = W, b, mean, std, pca
        self.pca_explained_variance_ratio_ = None if pca_explained_variance_ratio is None else f32(pca_explained_variance_ratio)
        if pivot is not None:
            self._model_pivot = f32(pivot)
        return self

    # ---- evaluation -------------------------------------------------------------------------------------------------------------
    def pivoted_model(self, device=None):
        """-> (pivot [C], beta [Cy], u [Cy, Dt], v [Cy, Dp], omega [Cy, Dt, Dp]) float32: the model about the pivot,
        pred_c = beta_c + x' . u_c + p' . v_c + x'^T omega_c p' with x' = x - pivot_x, p' = p - pivot_p; folded in float64."""
        if not hasattr(self, "coef_"):
            self.solve()
        dt, dp, cy = self._dt, self._dp, self._cy
        dm = dt + dp
        if self._pivot is not None:
            pivot = self._pivot.detach().cpu()
        elif self._moments is not None:
            pivot = self._moments[4].to(torch.float32)
        else:
            pivot = getattr(self, "_model_pivot", torch.zeros(dm + cy, dtype=torch.float32))
        G, w, px, pp = self._design_map(), self.coef_.double(), pivot[:dt].double(), pivot[dt:dm].double()
        gw = G.T @ w                                                             # the model on the raw columns [x | p | q]
        gq = gw[dm:].reshape(dt, dp, cy)
        fpi = torch.cat([px, pp, torch.outer(px, pp).reshape(-1)])
        beta = self.intercept_.double() + (G @ (fpi - self.mean_.double())) @ w
        u = gw[:dt] + torch.einsum("a,iac->ic", pp, gq)
        v = gw[dt:dm] + torch.einsum("i,iac->ac", px, gq)
        out = (pivot, beta.to(torch.float32).contiguous(), u.T.to(torch.float32).contiguous(), v.T.to(torch.float32).contiguous(),
               gq.permute(2, 0, 1).to(torch.float32).contiguous())
        return tuple(t.to(device) for t in out) if device is not None else out


def fit_phase_probe_full(batches, model, device, ridge_lambda: float = 1e-3, halo: int = 16, max_batches_train: int = 0,
                         interaction_pca_k: int = 20):
    """fit_phase_linear_probe.fit_phase_probe with its default design="full" in one pass over batches of (Ximg, Xphase, Yimg, M)
    -> (W [D_out, Cy], b [Cy], probe); probe.preprocessor_dict() is its ProbePreprocessor."""
    probe = InteractionProbe(ridge_lambda, interaction_pca_k)
    with torch.no_grad():
        for Ximg, Xphase, Yimg, M in _capped(batches, max_batches_train):
            z_type = model(Ximg.to(device))
            z_phase = model.forward_phase(Xphase.to(device), z_type.detach())
            probe.partial_fit((z_type, z_phase), Yimg.to(device), M.to(device), halo=halo)
    if probe._S is None or int(probe._n.item()) == 0:
        raise RuntimeError("No valid observations found in training data; cannot fit probe.")
    W, b = probe.solve()
    return W, b, probe


# ---- the reference's entry points ---------------------------------------------------------------------------------------------------
def _capped(batches: Iterable, max_batches: int):
    for i, batch in enumerate(batches):
        if max_batches and i >= max_batches:
            break
        yield batch


def fit_closed_form_ridge(batches, model, device, ridge_lambda: float = 1e-3, max_batches_train: int = 0):
    """fit_linear_probe.fit_closed_form_ridge over batches of (Ximg, Yimg, M) as its extract_batch_tensors returns them
    -> (W [D, T] float32, b [T] float32)."""
    probe = RidgeProbe(ridge_lambda)
    with torch.no_grad():
        for Ximg, Yimg, M in _capped(batches, max_batches_train):
            probe.partial_fit(model(Ximg.to(device)), Yimg.to(device), M.to(device))
    return probe.solve()


def evaluate_probe(batches, model, W, b, device, max_batches_eval: int = 0, target_names: Sequence[str] = TARGET_METRICS) -> ProbeMetrics:
    """fit_linear_probe.evaluate_probe over batches of (Ximg, Yimg, M)."""
    probe = RidgeProbe().set_model(W, b)
    with torch.no_grad():
        for Ximg, Yimg, M in _capped(batches, max_batches_eval):
            probe.partial_evaluate(model(Ximg.to(device)), Yimg.to(device), M.to(device))
    if probe._E is None:
        zeros = {k: 0.0 for k in target_names}
        return ProbeMetrics(dict(zeros), dict(zeros), dict(zeros), 0.0, 0.0, 0.0, 0)
    return probe.metrics(target_names)


def fit_phase_probe(batches, model, device, ridge_lambda: float = 1e-3, halo: int = 16, max_batches_train: int = 0, design: str = "additive"):
    """fit_phase_linear_probe.fit_phase_probe in one pass over batches of (Ximg, Xphase, Yimg, M) -> (W, b, probe): W and b for the
    standardised columns, probe.mean_ and probe.std_ the statistics of its preprocessor."""
    _check_design(design)
    probe = RidgeProbe(ridge_lambda, standardize=True)
    with torch.no_grad():
        for Ximg, Xphase, Yimg, M in _capped(batches, max_batches_train):
            z_type = model(Ximg.to(device))
            z_phase = model.forward_phase(Xphase.to(device), z_type.detach()) if design != "type-only" else None
            probe.partial_fit(design_features(design, z_type, z_phase), Yimg.to(device), M.to(device), halo=halo)
    if probe._S is None or int(probe._n.item()) == 0:
        raise RuntimeError("No valid observations found in training data; cannot fit probe.")
    W, b = probe.solve()
    return W, b, probe
