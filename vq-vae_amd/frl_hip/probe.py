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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

__all__ = ["RidgeProbe", "ProbeMetrics", "TARGET_METRICS", "DESIGN_CHOICES", "halo_mask", "spearman_rho2", "design_features", "design_dim",
           "fit_closed_form_ridge", "evaluate_probe", "fit_phase_probe"]

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
        raise NotImplementedError("probe: design='full' (768 interaction columns with PCA) is not built; use 'additive', 'type-only' or 'phase-only'")
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
        dims = ops.chk_probe(a, bs, y, m, self.workgroups, name)
        d, cy = dims[3] + dims[4], dims[5]
        if self._d is None:
            self._d, self._cy = d, cy
        elif (d, cy) != (self._d, self._cy):
            raise ValueError(f"{name}: this probe has D = {self._d}, Cy = {self._cy}; got D = {d}, Cy = {cy}")
        if self._ws is None or self._ws.device != a.device:
            self._ws = ops.probe_workspace(d, cy, a.device, self.workgroups)
        return a, bs, y, m

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
        pivot, wc, bc = self._eval_model
        pred = ops.probe_evaluate(a, bs, y, m, pivot, wc, bc, self._E, self._en, self._ws, want_pred=rank, workgroups=self.workgroups)
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
        pivot, wc, bc = self.pivoted_model(a.device)
        b, p = a.shape[0], a.shape[2]
        cy = wc.shape[1]
        y = torch.zeros(b, 1, p, cy, dtype=torch.float32, device=a.device)
        m = torch.ones(b, p, dtype=torch.uint8, device=a.device)
        ws = ops.probe_workspace(wc.shape[0], cy, a.device, self.workgroups)
        e, n = torch.zeros(cy, 3, dtype=torch.float64, device=a.device), torch.zeros(1, dtype=torch.int64, device=a.device)
        pred = ops.probe_evaluate(a, bs, y, m, pivot, wc, bc, e, n, ws, want_pred=True, workgroups=self.workgroups)
        t = pred.shape[1]
        return pred.view(b, hw[0], hw[1], cy) if t == 1 else pred.view(b, t, hw[0], hw[1], cy)


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
