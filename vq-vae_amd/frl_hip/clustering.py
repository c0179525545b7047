"""Embeddings to categories on the GPU: diagonal-covariance Gaussian mixtures, the BIC sweep over K, the phase summary and the
"forest type x recovery phase" taxonomy of the reference's frl/training/fit_gmm_clusters.py and fit_landscape_categories.py.

`DiagGMM` mirrors the names of sklearn.mixture.GaussianMixture(covariance_type="diag") that those scripts use.  One EM iteration is
three launches of csrc/gmm.hip (a fused E pass that reads X once, and the two small kernels of the M step); the lower bounds, the
iteration count and the convergence flag stay on the device, so iterations are enqueued without reading anything and the host looks
every `poll_every` iterations.  There are no float atomics: a fit is a bit-reproducible function of (X, sample_weight, init_rows or
the explicit initial parameters).  Row weights are native (sklearn has none; the reference resamples X instead).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops

__all__ = ["DiagGMM", "bic_sweep", "phase_summary", "fit_landscape_taxonomy", "draw_init_rows"]


def _f32(a, device=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device=device if device is not None else t.device, dtype=torch.float32).contiguous()


def _f64(a, device) -> torch.Tensor:
    t = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(torch.float64).to(device)


def _as_rows(X) -> torch.Tensor:
    t = X if isinstance(X, torch.Tensor) else torch.as_tensor(np.asarray(X))
    if t.dim() != 2:
        raise ValueError(f"DiagGMM: expected X [N, D], got {tuple(t.shape)}")
    return t


def draw_init_rows(n: int, k: int, n_init: int, seed: Optional[int]) -> np.ndarray:
    """init_rows [n_init][K]: K distinct rows of X per restart, drawn on the host from `seed`."""
    rng = np.random.default_rng(seed)
    return np.stack([np.sort(rng.choice(n, size=k, replace=False)) for _ in range(n_init)]).astype(np.int64)


class DiagGMM:
    """sklearn.mixture.GaussianMixture(covariance_type="diag") on the GPU; see the module docstring."""

    def __init__(self, n_components: int = 1, *, covariance_type: str = "diag", tol: float = 1e-3, reg_covar: float = 1e-6,
                 max_iter: int = 200, n_init: int = 1, seed: Optional[int] = None, init: str = "kmeans", kmeans_iters: int = 10,
                 weights_init=None, means_init=None, precisions_init=None, poll_every: int = 8, init_rows=None, workgroups: int = 0):
        if covariance_type != "diag":
            raise ValueError(f"DiagGMM: only covariance_type='diag' is built (the reference's default), got {covariance_type!r}")
        if init != "kmeans":
            raise ValueError(f"DiagGMM: only init='kmeans' is built, got {init!r}")
        if int(n_components) < 1 or int(max_iter) < 1 or int(n_init) < 1 or int(poll_every) < 1 or int(kmeans_iters) < 0:
            raise ValueError("DiagGMM: n_components, max_iter, n_init and poll_every must be >= 1 and kmeans_iters >= 0")
        if not 1 <= int(n_components) <= ops.GMM_MAX_K:
            raise ValueError(f"DiagGMM: supports 1 <= n_components <= {ops.GMM_MAX_K}, got {n_components}")
        self.n_components, self.covariance_type = int(n_components), "diag"
        self.tol, self.reg_covar, self.max_iter, self.n_init = float(tol), float(reg_covar), int(max_iter), int(n_init)
        self.seed, self.init, self.kmeans_iters, self.poll_every = seed, init, int(kmeans_iters), int(poll_every)
        self.weights_init, self.means_init, self.precisions_init = weights_init, means_init, precisions_init
        self.init_rows, self.workgroups = init_rows, int(workgroups)
        self.launches_ = 0
        self._pivot = None

    # ---- construction without a GPU ---------------------------------------------------------------------------------------------
    @classmethod
    def from_params(cls, weights, means, covariances, **kw) -> "DiagGMM":
        """A fitted object from parameters (numpy or torch, any device); needs no GPU until it scores data."""
        w, m, c = _f32(weights).cpu(), _f32(means).cpu(), _f32(covariances).cpu()
        if m.dim() != 2 or w.shape != (m.shape[0],) or c.shape != m.shape:
            raise ValueError(f"DiagGMM.from_params: expected weights [K], means [K, D], covariances [K, D], got {tuple(w.shape)}, "
                             f"{tuple(m.shape)}, {tuple(c.shape)}")
        ops.chk_gmm_dims(m.shape[0], m.shape[1], m.shape[0], "DiagGMM.from_params")
        g = cls(m.shape[0], **kw)
        g._set(w, m, c, converged=True, n_iter=0, lbs=np.zeros(0))
        return g

    def _set(self, w, m, c, converged, n_iter, lbs):
        self.weights_, self.means_, self.covariances_ = w, m, c
        self.precisions_cholesky_ = 1.0 / torch.sqrt(c)
        self.converged_, self.n_iter_ = bool(converged), int(n_iter)
        self.lower_bounds_ = np.asarray(lbs, np.float64)
        self.lower_bound_ = float(self.lower_bounds_[n_iter - 1]) if n_iter > 0 else float("-inf")

    def to_sklearn(self):
        """A sklearn.mixture.GaussianMixture with the fitted attributes set (the reference's .pkl payloads and predict callers)."""
        from sklearn.mixture import GaussianMixture
        self._fitted()
        g = GaussianMixture(n_components=self.n_components, covariance_type="diag", tol=self.tol, reg_covar=self.reg_covar,
                            max_iter=self.max_iter, n_init=self.n_init, random_state=self.seed)
        g.weights_ = self.weights_.double().cpu().numpy()
        g.means_ = self.means_.double().cpu().numpy()
        g.covariances_ = self.covariances_.double().cpu().numpy()
        g.precisions_cholesky_ = 1.0 / np.sqrt(g.covariances_)
        g.precisions_ = g.precisions_cholesky_ ** 2
        g.converged_, g.n_iter_, g.lower_bound_ = self.converged_, self.n_iter_, self.lower_bound_
        g.n_features_in_ = g.means_.shape[1]
        return g

    def _fitted(self):
        if not hasattr(self, "weights_"):
            raise RuntimeError("DiagGMM: not fitted")

    # ---- fit --------------------------------------------------------------------------------------------------------------------
    def _check_fit_inputs(self, X, sample_weight):
        X = _as_rows(X)
        k = self.n_components
        ops.chk_gmm(X, k, sample_weight if isinstance(sample_weight, torch.Tensor) else None, self.workgroups, "DiagGMM.fit")
        n, d = X.shape
        if sample_weight is not None:
            if not isinstance(sample_weight, torch.Tensor):
                raise ValueError("DiagGMM.fit: sample_weight must be a float32 tensor [N] on the device of X")
        for name, a, shape in (("weights_init", self.weights_init, (k,)), ("means_init", self.means_init, (k, d)),
                               ("precisions_init", self.precisions_init, (k, d))):
            if a is not None and tuple(np.shape(a)) != shape:
                raise ValueError(f"DiagGMM.fit: {name} must have shape {shape}, got {tuple(np.shape(a))}")
        if self.init_rows is not None:
            r = np.asarray(self.init_rows)
            if r.shape != (self.n_init, k) or r.min() < 0 or r.max() >= n:
                raise ValueError(f"DiagGMM.fit: init_rows must be [n_init, K] = {(self.n_init, k)} row indices below N = {n}")
        if not X.is_cuda:
            raise _lib.FrlHipError("DiagGMM.fit: X must live on the GPU (no CPU fallback)")
        if sample_weight is not None and sample_weight.device != X.device:
            raise ValueError("DiagGMM.fit: sample_weight must be on the device of X")
        return X

    def _initial(self, X, w, pivot, rows, state, ws):
        """-> (pi, mu, mc, var) of one restart: Lloyd steps from `rows`, then the M step of the one-hot responsibilities; the
        explicit *_init arguments override what they name, as in sklearn."""
        k, (n, d), dev = self.n_components, X.shape, X.device
        pi = torch.full((k,), 1.0 / k, dtype=torch.float32, device=dev)
        var = torch.ones(k, d, dtype=torch.float32, device=dev)
        mu = X[torch.as_tensor(rows, device=dev)].contiguous()
        mc = (mu.double() - pivot.double()).float()
        if self.means_init is None or self.weights_init is None or self.precisions_init is None:
            for _ in range(self.kmeans_iters):
                ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, hard=True, workgroups=self.workgroups)
                ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, mode=ops.GMM_M_LLOYD, workgroups=self.workgroups)
                self.launches_ += 3
            ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, hard=True, workgroups=self.workgroups)
            ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, reg_covar=self.reg_covar, mode=ops.GMM_M_INIT, workgroups=self.workgroups)
            self.launches_ += 3
        if self.weights_init is not None:
            pi = _f64(self.weights_init, dev).float().contiguous()
        if self.means_init is not None:
            m64 = _f64(self.means_init, dev)
            mu, mc = m64.float().contiguous(), (m64 - pivot.double()).float().contiguous()
        if self.precisions_init is not None:
            var = (1.0 / _f64(self.precisions_init, dev)).float().contiguous()
        return pi, mu, mc, var

    def init_params(self, X, sample_weight=None, restart: int = 0):
        """-> (weights, means, covariances) that restart `restart` of fit(X, sample_weight) starts from."""
        X = self._check_fit_inputs(X, sample_weight)
        (n, d), k = X.shape, self.n_components
        ws = ops.gmm_workspace(n, d, k, X.device, self.workgroups)
        pivot = ops.gmm_pivot(X, ws)
        rows = np.asarray(self.init_rows) if self.init_rows is not None else draw_init_rows(n, k, self.n_init, self.seed)
        pi, mu, _, var = self._initial(X, sample_weight, pivot, rows[restart], torch.zeros(2, dtype=torch.int32, device=X.device), ws)
        return pi, mu, var

    def fit(self, X, sample_weight=None) -> "DiagGMM":
        X = self._check_fit_inputs(X, sample_weight)
        (n, d), k, dev = X.shape, self.n_components, X.device
        w = sample_weight
        ws = ops.gmm_workspace(n, d, k, dev, self.workgroups)
        pivot = ops.gmm_pivot(X, ws)
        self.launches_ = 2
        rows = np.asarray(self.init_rows) if self.init_rows is not None else draw_init_rows(n, k, self.n_init, self.seed)
        best = None
        for r in range(self.n_init):
            state = torch.zeros(2, dtype=torch.int32, device=dev)
            history = torch.full((self.max_iter,), float("nan"), dtype=torch.float64, device=dev)
            pi, mu, mc, var = self._initial(X, w, pivot, rows[r], state, ws)
            done = 0
            while done < self.max_iter:
                for _ in range(min(self.poll_every, self.max_iter - done)):
                    ops.gmm_em_step(X, w, pivot, pi, mc, var, state, ws, workgroups=self.workgroups)
                    ops.gmm_m_step(n, pivot, pi, mu, mc, var, state, ws, history, self.reg_covar, self.tol, ops.GMM_M_EM, self.workgroups)
                    done += 1
                    self.launches_ += 3
                if int(state[1].item()):
                    break
            n_iter, conv = (int(v) for v in state.tolist())
            lbs = history.cpu().numpy()
            if best is None or lbs[n_iter - 1] > best[5][best[4] - 1]:
                best = (pi, mu, var, bool(conv), n_iter, lbs)
        self._set(best[0], best[1], best[2], best[3], best[4], best[5])
        self._pivot = pivot
        return self

    # ---- scoring ----------------------------------------------------------------------------------------------------------------
    def _score(self, X, want_resp=False):
        self._fitted()
        X = _as_rows(X)
        ops.chk_gmm(X, self.n_components, name="DiagGMM", need_rows=False)
        if X.shape[1] != self.means_.shape[1]:
            raise ValueError(f"DiagGMM: X has {X.shape[1]} columns, the mixture {self.means_.shape[1]}")
        if not X.is_cuda:
            raise _lib.FrlHipError("DiagGMM: X must live on the GPU (no CPU fallback)")
        dev = X.device
        pi, mu, var = (t.to(dev) for t in (self.weights_, self.means_, self.covariances_))
        # any pivot near the data serves: the one of the fit, else the mixture's own mean
        p64 = self._pivot.to(dev).double() if self._pivot is not None and self._pivot.device == dev else (pi.double()[:, None] * mu.double()).sum(0)
        pivot = p64.float().contiguous()
        mc = (mu.double() - pivot.double()).float().contiguous()
        return ops.gmm_score(X, pivot, pi.contiguous(), mc, var.contiguous(), want_resp)

    def score_samples(self, X) -> torch.Tensor:
        return self._score(X)[0]

    def predict(self, X) -> torch.Tensor:
        return self._score(X)[1].long()

    def predict_proba(self, X) -> torch.Tensor:
        return self._score(X, True)[2]

    def score(self, X) -> float:
        return float(self.score_samples(X).double().mean().item())

    def _n_parameters(self) -> int:
        k, d = self.means_.shape
        return 2 * k * d + k - 1

    def bic(self, X) -> float:
        return -2.0 * self.score(X) * X.shape[0] + self._n_parameters() * float(np.log(X.shape[0]))

    def aic(self, X) -> float:
        return -2.0 * self.score(X) * X.shape[0] + 2.0 * self._n_parameters()


def bic_sweep(X, k_values: Sequence[int], n_init_sweep: int = 1, n_init_final: int = 3, max_iter: int = 200, seed: Optional[int] = 42,
              sample_weight=None, **gmm_kw):
    """The reference's _bic_sweep: one fit per K with n_init_sweep restarts, the K of the lowest BIC refitted with n_init_final.
    -> (best_k, best_gmm, {K: BIC}).  `init_rows` in gmm_kw may map (K, n_init) -> rows [n_init, K] to pin every initialisation."""
    rows = gmm_kw.pop("init_rows", None)
    bics: Dict[int, float] = {}
    for k in k_values:
        g = DiagGMM(int(k), n_init=n_init_sweep, max_iter=max_iter, seed=seed, init_rows=None if rows is None else rows[(int(k), n_init_sweep)],
                    **gmm_kw).fit(X, sample_weight)
        bics[int(k)] = g.bic(X)
    best_k = min(bics, key=bics.__getitem__)
    best = DiagGMM(best_k, n_init=n_init_final, max_iter=max_iter, seed=seed,
                   init_rows=None if rows is None else rows[(best_k, n_init_final)], **gmm_kw).fit(X, sample_weight)
    return best_k, best, bics


def phase_summary(z_phase: torch.Tensor, ysfc: torch.Tensor, low_max: float = 1.0, high_min: float = 5.0):
    """The reference's _compute_phase_summary: z_phase [N, T, D], ysfc [N, T] (NaN: unobserved) -> (summary [N, 3 D] = disturbed
    centroid | recovered centroid | overall mean, temporal_var [N])."""
    return ops.phase_summary(z_phase, ysfc, low_max, high_min)


def fit_landscape_taxonomy(z_type: torch.Tensor, summary: torch.Tensor, k_type_values: Sequence[int], k_phase_max: int = 5,
                           min_cluster_pixels: int = 1000, n_init_sweep: int = 1, n_init_final: int = 3, max_iter: int = 200,
                           seed: Optional[int] = 42, **gmm_kw):
    """Steps 2-4 of fit_landscape_categories.py over tensors: a BIC sweep over z_type [N, Dz], its labels, and per type cluster with at
    least min_cluster_pixels rows a BIC sweep over K = 1..k_phase_max on its rows of summary [N, Ds].
    -> {"type_gmm", "bic_type", "phase_gmms": {k: DiagGMM | None}, "taxonomy": {k: {n_pixels, k_phase, is_dynamic}}}."""
    if z_type.dim() != 2 or summary.dim() != 2 or z_type.shape[0] != summary.shape[0]:
        raise ValueError(f"fit_landscape_taxonomy: expected z_type [N, Dz] and summary [N, Ds], got {tuple(z_type.shape)} and {tuple(summary.shape)}")
    k_type, type_gmm, bic_type = bic_sweep(z_type, k_type_values, n_init_sweep, n_init_final, max_iter, seed, **gmm_kw)
    labels = type_gmm.predict(z_type)
    phase_gmms, taxonomy = {}, {}
    for k in range(k_type):
        sel = labels == k
        n_k = int(sel.sum().item())
        if n_k < max(int(min_cluster_pixels), 1):
            phase_gmms[k] = None
            taxonomy[k] = dict(n_pixels=n_k, k_phase=1, is_dynamic=False)
            continue
        rows = summary[sel].contiguous()
        ks = [kk for kk in range(1, int(k_phase_max) + 1) if kk <= n_k]
        k_phase, g, _ = bic_sweep(rows, ks, n_init_sweep, n_init_final, max_iter, seed, **gmm_kw)
        phase_gmms[k] = g
        taxonomy[k] = dict(n_pixels=n_k, k_phase=int(k_phase), is_dynamic=k_phase > 1)
    return dict(type_gmm=type_gmm, bic_type=bic_type, phase_gmms=phase_gmms, taxonomy=taxonomy)
