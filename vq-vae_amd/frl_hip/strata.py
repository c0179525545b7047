"""EVT-stratified diagnostics on the GPU: the grouped accumulation behind the reference's frl/training/compare_gmm_evt.py (cluster x EVT
contingency table and its clustering metrics), phase_evt_diagnostics.py (`EvtAccumulators`: per-EVT FiLM gamma mean and std, temporal
variance fraction of z_phase, per-EVT probe R^2) and ysfc_evt_histograms.py (ysfc-bin x EVT counts).

All three stream over the valid pixels of a split, key every row by its EVT code and accumulate counts or first and second moments per
key.  Here the labels, gamma, z_phase and the probe predictions stay on the device, channels-last as `DiagGMM.predict`,
`forward_phase_nhwc(return_parts=True)` and `RidgeProbe.predict` return them, and csrc/strata.hip accumulates in one pass: no per-pixel
data crosses to the host.  NMI, homogeneity, completeness, V-measure and purity are functions of the contingency table alone
(`clustering_metrics`), so they are exact over every pixel where the reference computes them on a 500 k reservoir sample.

Moments are kept about a pivot p (float32, fixed on the first call): S1 = sum (x - p), S2 = sum (x - p)^2 per group and column, from which
mean = p + S1 / n and var = S2 / n - (S1 / n)^2 lose nothing to a large offset; `sum()` and `sumsq()` undo the pivot on the host in float64.
"""
from __future__ import annotations

import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

__all__ = ["clustering_metrics", "ContingencyTable", "GroupedMoments", "EvtAccumulators", "ysfc_evt_histogram", "YSFC_BINS", "YSFC_BIN_LABELS",
           "RecoveryCurves", "RECOVERY_YSFC_BINS", "RECOVERY_YSFC_BIN_LABELS"]

# years since fire/change; the right endpoint is exclusive
YSFC_BINS: List[Tuple[int, int]] = [(0, 1), (1, 2), (2, 3), (3, 5), (5, 8), (8, 13), (13, 20), (20, 31), (31, 41)]
YSFC_BIN_LABELS: List[str] = ["0", "1", "2", "3–4", "5–7", "8–12", "13–19", "20–30", "31–40"]
# the 8 bins of phase_recovery_curves.py (it stops at 30 years)
RECOVERY_YSFC_BINS: List[Tuple[int, int]] = YSFC_BINS[:8]
RECOVERY_YSFC_BIN_LABELS: List[str] = YSFC_BIN_LABELS[:8]


# ---- metrics of a contingency table -------------------------------------------------------------------------------------------------
def _entropy(counts: np.ndarray) -> float:
    pi = counts[counts > 0].astype(np.float64)
    if pi.size <= 1:
        return 0.0
    tot = pi.sum()
    return float(-np.sum((pi / tot) * (np.log(pi) - np.log(tot))))


def _mutual_information(t: np.ndarray) -> float:
    r, c = np.nonzero(t)
    nz = t[r, c].astype(np.float64)
    tot = nz.sum()
    pi, pj = t.sum(axis=1).astype(np.float64), t.sum(axis=0).astype(np.float64)
    nm = nz / tot
    log_outer = -np.log(pi[r] * pj[c]) + np.log(pi.sum()) + np.log(pj.sum())
    mi = nm * (np.log(nz) - np.log(tot)) + nm * log_outer
    mi = np.where(np.abs(mi) < np.finfo(np.float64).eps, 0.0, mi)
    return float(np.clip(mi.sum(), 0.0, None))


def clustering_metrics(table) -> dict:
    """The reference's compute_metrics from the full table [clusters, EVT classes] of counts, in float64 on the host: `nmi` (arithmetic
    normalisation; 1.0 when both entropies are 0), `homogeneity`, `completeness`, `v_measure` (labels-true is EVT, labels-pred is the
    cluster, as the reference calls sklearn), `purity` and `n_pixels_metrics`.  Needs neither sklearn nor a GPU."""
    t = np.asarray(table)
    if t.ndim != 2 or t.size == 0 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"clustering_metrics: expected an integer table [R, G], got {t.dtype} {t.shape}")
    if (t < 0).any():
        raise ValueError("clustering_metrics: negative count")
    t = t.astype(np.int64)
    n = int(t.sum())
    if n == 0:
        raise ValueError("clustering_metrics: the table is empty")
    h_class, h_cluster = _entropy(t.sum(axis=0)), _entropy(t.sum(axis=1))
    mi = _mutual_information(t)
    if (t.sum(axis=0) > 0).sum() == 1 and (t.sum(axis=1) > 0).sum() == 1:
        nmi = 1.0
    elif mi == 0.0:
        nmi = 0.0
    else:
        nmi = mi / (0.5 * (h_class + h_cluster))
    hom = mi / h_class if h_class else 1.0
    comp = mi / h_cluster if h_cluster else 1.0
    vm = 0.0 if hom + comp == 0.0 else 2.0 * hom * comp / (hom + comp)
    purity = int(t.max(axis=1).sum()) / n
    return {"nmi": float(nmi), "homogeneity": float(hom), "completeness": float(comp), "v_measure": float(vm), "purity": float(purity),
            "n_pixels_metrics": n}


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def _vocab(codes, name: str) -> np.ndarray:
    """The vocabulary as increasing int32 codes (sorted, duplicates dropped)."""
    if isinstance(codes, torch.Tensor):
        codes = codes.cpu().numpy()
    v = np.asarray(codes if isinstance(codes, np.ndarray) else list(codes))
    if v.ndim != 1 or v.size == 0 or not np.issubdtype(v.dtype, np.integer):
        raise ValueError(f"{name}: codes must be a non-empty 1-D sequence of integers, got {v.dtype} {v.shape}")
    if v.min() < -2 ** 31 or v.max() >= 2 ** 31:
        raise ValueError(f"{name}: codes must fit int32")
    v = np.unique(v.astype(np.int64)).astype(np.int32)
    if v.size > ops.STRATA_MAX_G:
        raise ValueError(f"{name}: supports 1 <= G <= {ops.STRATA_MAX_G} codes in the vocabulary, got {v.size}")
    return v


def _need_gpu(name: str, *ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")


def _codes_rows(codes: torch.Tensor, name: str):
    """-> (codes [B, P] int32 or float32 contiguous, B, pixel shape)."""
    if not isinstance(codes, torch.Tensor) or codes.dim() < 1:
        raise ValueError(f"{name}: codes must be a tensor [N] or [B, ...], got {type(codes).__name__}")
    if codes.dtype not in (torch.int32, torch.float32):
        codes = codes.to(torch.float32 if codes.dtype.is_floating_point else torch.int32)
    b, shape = (1, tuple(codes.shape)) if codes.dim() == 1 else (codes.shape[0], tuple(codes.shape[1:]))
    return codes.contiguous().view(b, -1), b, shape


def _per_pixel_or_step(t: torch.Tensor, b: int, shape, what: str, name: str):
    """[*codes.shape] -> [B, 1, P]; [B, T, *pixel shape] -> [B, T, P]."""
    shape = tuple(shape)
    if tuple(t.shape) == (b,) + shape or (b == 1 and tuple(t.shape) == shape):
        return t.contiguous().view(b, 1, -1)
    if t.dim() == len(shape) + 2 and t.shape[0] == b and tuple(t.shape[2:]) == shape:
        return t.contiguous().view(b, t.shape[1], -1)
    raise ValueError(f"{name}: {what} {tuple(t.shape)} is neither per pixel {(b,) + tuple(shape)} nor per timestep {(b, 'T') + tuple(shape)}")


def _mask_rows(mask: Optional[torch.Tensor], b: int, shape, name: str):
    if mask is None:
        return None
    m = mask if mask.dtype == torch.bool else mask != 0
    return _per_pixel_or_step(m, b, shape, "mask", name).view(torch.uint8)


# ---- the contingency table ----------------------------------------------------------------------------------------------------------
class ContingencyTable:
    """table[r][g] = the number of unmasked observations with row label r (0 <= r < n_rows) and EVT code codes[g].

    With `codes` given nothing is read back until `table()`.  With codes=None the vocabulary is discovered: every `partial_fit` runs
    torch.unique on its valid unmasked codes (one host read per call) and re-indexes the table's columns as the vocabulary grows."""

    def __init__(self, n_rows: int, codes: Optional[Sequence[int]] = None, workgroups: int = 0):
        self.n_rows, self.workgroups = int(n_rows), int(workgroups)
        self._discover = codes is None
        self._codes = None if codes is None else _vocab(codes, "ContingencyTable")
        ops.chk_strata_table_dims(self.n_rows, 1 if self._codes is None else self._codes.size, self.workgroups, "ContingencyTable")
        self._vocab_dev = self._table = self._unm = self._rej = self._host = None

    @classmethod
    def from_table(cls, table, codes: Sequence[int], unmatched: int = 0, rejected: int = 0) -> "ContingencyTable":
        """A table held on the host (int [R, G] with the code of every column); needs no GPU."""
        t = np.asarray(table)
        g = cls(t.shape[0], codes)
        if t.ndim != 2 or t.shape[1] != g._codes.size or not np.issubdtype(t.dtype, np.integer):
            raise ValueError(f"ContingencyTable.from_table: expected an integer table [R, {g._codes.size}], got {t.dtype} {t.shape}")
        g._host = (t.astype(np.int64), int(unmatched), int(rejected))
        return g

    def _state(self, device):
        if self._unm is None:
            self._unm = torch.zeros(1, dtype=torch.int64, device=device)
            self._rej = torch.zeros(1, dtype=torch.int64, device=device)
        if self._table is None and self._codes is not None:
            self._vocab_dev = torch.from_numpy(self._codes).to(device)
            self._table = torch.zeros(self.n_rows, self._codes.size, dtype=torch.int64, device=device)

    def _grow(self, codes: torch.Tensor, mask: Optional[torch.Tensor]):
        c = codes
        if mask is not None:
            c = c[mask.bool().any(dim=1)]
        c = c[torch.isfinite(c) & (c > 0)] if c.dtype.is_floating_point else c[c > 0]
        seen = torch.unique(c.to(torch.int32)).cpu().numpy()                       # the host read of a discovering call
        union = seen if self._codes is None else np.union1d(self._codes, seen).astype(np.int32)
        if union.size == 0 or (self._codes is not None and union.size == self._codes.size):
            return
        ops.chk_strata_table_dims(self.n_rows, union.size, self.workgroups, "ContingencyTable")
        table = torch.zeros(self.n_rows, union.size, dtype=torch.int64, device=codes.device)
        if self._table is not None:
            table[:, torch.from_numpy(np.searchsorted(union, self._codes)).to(codes.device)] = self._table
        self._codes, self._table, self._vocab_dev = union, table, torch.from_numpy(union).to(codes.device)

    def partial_fit(self, labels: torch.Tensor, codes: torch.Tensor, mask: Optional[torch.Tensor] = None) -> "ContingencyTable":
        """labels int [N] / [B, ...] (per pixel) or [B, T, ...] (per timestep); codes int32 or float32 [N] / [B, ...]; mask like either."""
        name = "ContingencyTable.partial_fit"
        c, b, shape = _codes_rows(codes, name)
        if not isinstance(labels, torch.Tensor) or labels.dtype.is_floating_point:
            raise ValueError(f"{name}: labels must be an integer tensor")
        rows = _per_pixel_or_step(labels if labels.dtype == torch.int32 else labels.to(torch.int32), b, shape, "labels", name)
        m = _mask_rows(mask, b, shape, name)
        if m is not None and rows.shape[1] != m.shape[1] and 1 not in (rows.shape[1], m.shape[1]):
            raise ValueError(f"{name}: labels and mask differ in T: {rows.shape[1]} and {m.shape[1]}")
        _need_gpu(name, c, rows, m)
        self._state(c.device)
        if self._discover:
            self._grow(c, m)
            if self._table is None:                                              # no valid code yet
                return self
        ops.strata_contingency(rows, c, m, self._vocab_dev, self._table, self._unm, self._rej, self.workgroups)
        self._host = None
        return self

    def _read(self):
        if self._host is None:
            if self._table is None:
                raise RuntimeError("ContingencyTable: nothing was accumulated")
            flat = torch.cat([self._table.reshape(-1), self._unm, self._rej]).cpu().numpy()   # the one host read
            self._host = (flat[:-2].reshape(self.n_rows, -1).copy(), int(flat[-2]), int(flat[-1]))
        return self._host

    def table(self) -> Tuple[np.ndarray, List[int]]:
        """-> (int64 [R, G], the EVT code of every column)."""
        return self._read()[0], [int(c) for c in self._codes]

    @property
    def unmatched_(self) -> int:
        """Observations with a valid code that the vocabulary does not hold."""
        return self._read()[1]

    @property
    def rejected_(self) -> int:
        """Observations whose row label lies outside [0, n_rows)."""
        return self._read()[2]

    def top_codes(self, k: int) -> List[int]:
        """The k codes of largest column total, descending, ties by the lower code."""
        t, codes = self.table()
        order = np.lexsort((np.asarray(codes), -t.sum(axis=0)))
        return [codes[i] for i in order[:int(k)]]

    def metrics(self) -> dict:
        t, _ = self.table()
        if self.rejected_ > 0:
            raise ValueError(f"ContingencyTable.metrics: {self.rejected_} observations had a row label outside [0, {self.n_rows})")
        if self.unmatched_ > 0:
            warnings.warn(f"ContingencyTable.metrics: {self.unmatched_} observations had an EVT code outside the vocabulary and are not counted")
        out = clustering_metrics(t)
        out["n_unmatched"] = self.unmatched_
        return out


def ysfc_evt_histogram(ysfc: torch.Tensor, codes: torch.Tensor, mask: Optional[torch.Tensor] = None, bins: Sequence[Tuple[int, int]] = YSFC_BINS,
                       max_ysfc: float = 40.0, evt_codes: Optional[Sequence[int]] = None, table: Optional[ContingencyTable] = None) -> ContingencyTable:
    """ysfc-bin x EVT counts of ysfc_evt_histograms.py over every observation (no reservoir): ysfc [B, T, ...] in years, codes [B, ...],
    mask per pixel or per timestep; an observation counts where 0 <= ysfc <= max_ysfc.  Adds into `table` when one is given."""
    edges = [float(lo) for lo, _ in bins] + [float(bins[-1][1])]
    if any(float(bins[i][1]) != edges[i + 1] for i in range(len(bins))) or any(a >= b for a, b in zip(edges, edges[1:])):
        raise ValueError("ysfc_evt_histogram: bins must be contiguous and increasing")
    if table is None:
        table = ContingencyTable(len(bins), evt_codes)
    elif table.n_rows != len(bins):
        raise ValueError(f"ysfc_evt_histogram: the table has {table.n_rows} rows for {len(bins)} bins")
    _need_gpu("ysfc_evt_histogram", ysfc, codes, mask)
    _, b, shape = _codes_rows(codes, "ysfc_evt_histogram")
    if ysfc.dim() != len(shape) + 2 or ysfc.shape[0] != b or tuple(ysfc.shape[2:]) != tuple(shape):
        raise ValueError(f"ysfc_evt_histogram: ysfc must be [B, T, ...] = {(b, 'T') + tuple(shape)}, got {tuple(ysfc.shape)}")
    y = ysfc.float()
    keep = (y >= 0) & (y <= float(max_ysfc)) & (y < edges[-1])
    if mask is not None:
        m = mask if mask.dtype == torch.bool else mask != 0
        keep = keep & (m.unsqueeze(1) if m.dim() == ysfc.dim() - 1 else m)
    idx = torch.bucketize(y, torch.tensor(edges, dtype=torch.float32, device=y.device), right=True) - 1
    return table.partial_fit(torch.where(keep, idx, torch.zeros_like(idx)).to(torch.int32), codes, keep)


# ---- grouped moments ----------------------------------------------------------------------------------------------------------------
class GroupedMoments:
    """Per EVT code and column: the count and the first and second moments of the rows, or (temporal=True) of the per-pixel means over t
    together with the sum of the per-pixel population variances over t.

    pivot: None or "mean" (the masked column mean of the first call, from a zero-pivot call of the same kernel; one host read per call
    until a call had a valid row), "zero", or a vector [n_columns].  Vocabularies longer than the kernel's window are walked in chunks.
    Results are float64 on the host from one read: `count_`, `sum()`, `sumsq()`, `mean()`, `var()`, `within_`, `unmatched_`."""

    def __init__(self, codes: Sequence[int], n_columns: int, temporal: bool = False, pivot=None, workgroups: int = 0):
        self._codes = _vocab(codes, "GroupedMoments")
        self.n_columns, self.temporal, self.workgroups = int(n_columns), bool(temporal), int(workgroups)
        self.window = max(1, min(self._codes.size, ops.STRATA_MAX_GC, ops.STRATA_MAX_GD // max(self.n_columns, 1)))
        ops.chk_strata_moment_dims(self.window, self.n_columns, self.workgroups, "GroupedMoments")
        if pivot is None or (isinstance(pivot, str) and pivot == "mean"):
            self._pivot_host = None
        elif isinstance(pivot, str):
            if pivot != "zero":
                raise ValueError(f"GroupedMoments: pivot must be None, 'mean', 'zero' or a vector, got {pivot!r}")
            self._pivot_host = np.zeros(self.n_columns, np.float32)
        else:
            self._pivot_host = np.asarray(pivot, np.float32).reshape(-1)
            if self._pivot_host.size != self.n_columns:
                raise ValueError(f"GroupedMoments: pivot has {self._pivot_host.size} entries for {self.n_columns} columns")
        self._pivot = self._vocab_dev = self._count = self._s1 = self._s2 = self._sw = self._unm = self._ws = self._host = None

    @property
    def codes(self) -> List[int]:
        return [int(c) for c in self._codes]

    @classmethod
    def from_sums(cls, codes, count, s1, s2, pivot, within=None) -> "GroupedMoments":
        """Moments from pivoted sums held on the host (count [G], S1 and S2 [G, D] about pivot [D]); needs no GPU."""
        s1 = np.asarray(s1, np.float64)
        g = cls(codes, s1.shape[1], temporal=within is not None, pivot=np.asarray(pivot, np.float32))
        if s1.shape != (g._codes.size, g.n_columns):
            raise ValueError(f"GroupedMoments.from_sums: S1 {s1.shape} for {g._codes.size} codes and {g.n_columns} columns")
        g._host = (np.asarray(count, np.int64), s1, np.asarray(s2, np.float64), None if within is None else np.asarray(within, np.float64), 0,
                   np.asarray(pivot, np.float32).astype(np.float64))
        return g

    # ---- accumulation -----------------------------------------------------------------------------------------------------------
    def _rows(self, values: torch.Tensor, channels_last: bool, name: str):
        if not isinstance(values, torch.Tensor) or values.dim() not in (2, 4, 5):
            raise ValueError(f"{name}: values must be [N, D], [B, H, W, D] or [B, T, H, W, D], got {tuple(getattr(values, 'shape', ()))}")
        if values.dtype != torch.float32:
            raise ValueError(f"{name}: values must be float32, got {values.dtype}")
        v = values
        if not channels_last and v.dim() > 2:
            v = v.permute(0, 2, 3, 1) if v.dim() == 4 else v.permute(0, 2, 3, 4, 1)
        if v.shape[-1] != self.n_columns:
            raise ValueError(f"{name}: values have {v.shape[-1]} columns, this accumulator {self.n_columns}")
        v = v.contiguous()
        if v.dim() == 2:
            return v.view(1, 1, v.shape[0], v.shape[1]), (v.shape[0],), 1
        if v.dim() == 4:
            return v.view(v.shape[0], 1, -1, v.shape[-1]), tuple(v.shape[1:3]), v.shape[0]
        return v.view(v.shape[0], v.shape[1], -1, v.shape[-1]), tuple(v.shape[2:4]), v.shape[0]

    def _call(self, x, c, m, pivot, count, s1, s2, sw, unm):
        g = self._codes.size
        for g0 in range(0, g, self.window):
            ops.strata_moments(x, c, m, self._vocab_dev, g0, min(self.window, g - g0), pivot, count, s1, s2, sw, unm if g0 == 0 else None, self._ws,
                               self.temporal, self.workgroups)

    def _zeros(self, device):
        g, d = self._codes.size, self.n_columns
        return (torch.zeros(g, dtype=torch.int64, device=device), torch.zeros(g, d, dtype=torch.float64, device=device),
                torch.zeros(g, d, dtype=torch.float64, device=device), torch.zeros(g, d, dtype=torch.float64, device=device) if self.temporal else None)

    def partial_fit(self, values: torch.Tensor, codes: torch.Tensor, mask: Optional[torch.Tensor] = None, channels_last: bool = True) -> "GroupedMoments":
        name = "GroupedMoments.partial_fit"
        x, shape, b = self._rows(values, channels_last, name)
        c, bc, cshape = _codes_rows(codes, name)
        if (bc, tuple(cshape)) != (b, tuple(shape)) and not (b == 1 and c.numel() == x.shape[2]):
            raise ValueError(f"{name}: codes {tuple(codes.shape)} do not match values {tuple(values.shape)}")
        c = c.view(b, -1)
        m = _mask_rows(mask, b, shape, name)
        if m is not None and m.shape[1] not in (1, x.shape[1]):
            raise ValueError(f"{name}: mask {tuple(mask.shape)} does not match T = {x.shape[1]}")
        if self.temporal and m is not None and m.shape[1] != 1:
            raise ValueError(f"{name}: the temporal mode takes a per-pixel mask")
        _need_gpu(name, x, c, m)
        dev = x.device
        if self._count is None:
            self._vocab_dev = torch.from_numpy(self._codes).to(dev)
            self._ws = ops.strata_workspace(self.window, self.n_columns, self.temporal, dev, self.workgroups)
            self._count, self._s1, self._s2, self._sw = self._zeros(dev)
            self._unm = torch.zeros(1, dtype=torch.int64, device=dev)
            if self._pivot_host is not None:
                self._pivot = torch.from_numpy(self._pivot_host).to(dev)
        if self._pivot is None:                                                  # the masked column mean of this call, by the kernel itself
            n0, a1, a2, aw = self._zeros(dev)
            self._call(x, c, m, torch.zeros(self.n_columns, dtype=torch.float32, device=dev), n0, a1, a2, aw, None)
            n = int(n0.sum().item())                                             # one host read per call until a row counted
            if n == 0:
                return self
            self._pivot = (a1.sum(dim=0) / n).to(torch.float32)
        self._call(x, c, m, self._pivot, self._count, self._s1, self._s2, self._sw, self._unm)
        self._host = None
        return self

    # ---- results ----------------------------------------------------------------------------------------------------------------
    def _read(self):
        if self._host is None:
            g, d = self._codes.size, self.n_columns
            if self._count is None or self._pivot is None:
                z = np.zeros((g, d))
                self._host = (np.zeros(g, np.int64), z, z.copy(), z.copy() if self.temporal else None, 0, np.zeros(d))
            else:
                parts = [self._count.double(), self._unm.double(), self._pivot.double(), self._s1.reshape(-1), self._s2.reshape(-1)]
                if self.temporal:
                    parts.append(self._sw.reshape(-1))
                flat = torch.cat(parts).cpu().numpy()                            # the one host read
                o = g + 1 + d
                self._host = (flat[:g].astype(np.int64), flat[o:o + g * d].reshape(g, d), flat[o + g * d:o + 2 * g * d].reshape(g, d),
                              flat[o + 2 * g * d:].reshape(g, d) if self.temporal else None, int(flat[g]), flat[g + 1:o])
        return self._host

    @property
    def count_(self) -> np.ndarray:
        return self._read()[0]

    @property
    def within_(self) -> Optional[np.ndarray]:
        """[G, D]: the sum over the group's pixels of the population variance over t (temporal mode)."""
        return self._read()[3]

    @property
    def unmatched_(self) -> int:
        return self._read()[4]

    @property
    def pivot_(self) -> np.ndarray:
        return self._read()[5]

    def pivoted(self):
        """-> (count [G], S1 [G, D], S2 [G, D]) about pivot_."""
        return self._read()[:3]

    def sum(self) -> np.ndarray:
        n, s1, _, _, _, p = self._read()
        return s1 + n[:, None] * p[None, :]

    def sumsq(self) -> np.ndarray:
        n, s1, s2, _, _, p = self._read()
        return s2 + 2.0 * p[None, :] * s1 + n[:, None] * (p * p)[None, :]

    def mean(self) -> np.ndarray:
        """[G, D]; zeros for an empty group."""
        n, s1, _, _, _, p = self._read()
        nn = np.maximum(n, 1)[:, None]
        return np.where(n[:, None] > 0, p[None, :] + s1 / nn, 0.0)

    def var(self) -> np.ndarray:
        """[G, D]: the population variance, clamped at 0; zeros for an empty group."""
        n, s1, s2, _, _, _ = self._read()
        nn = np.maximum(n, 1)[:, None]
        return np.where(n[:, None] > 0, np.maximum(s2 / nn - (s1 / nn) ** 2, 0.0), 0.0)


# ---- the reference's accumulators -----------------------------------------------------------------------------------------------------
class EvtAccumulators:
    """phase_evt_diagnostics.EvtAccumulators with its method names and return conventions, over device tensors.

    `codes` is the EVT vocabulary (the reference discovers it; here a class outside it is counted in `unmatched_` and left out).  Gamma
    is a plain GroupedMoments, z_phase a temporal one, the probe an observations-mode one over [pred - target | target]."""

    def __init__(self, d_phase: int, n_target_ch: Optional[int] = None, codes: Sequence[int] = (), workgroups: int = 0):
        self.d_phase, self.n_target_ch = int(d_phase), None if n_target_ch is None else int(n_target_ch)
        self.gamma = GroupedMoments(codes, self.d_phase, workgroups=workgroups)
        self.phase = GroupedMoments(codes, self.d_phase, temporal=True, workgroups=workgroups)
        self.probe = None if n_target_ch is None else GroupedMoments(codes, 2 * self.n_target_ch, workgroups=workgroups)
        self._index = {c: i for i, c in enumerate(self.gamma.codes)}

    def add_pixels(self, evt_codes: torch.Tensor, gamma: torch.Tensor, z_phase: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """gamma [B, H, W, d] or [N, d]; z_phase channels-last [B, T, H, W, d] as forward_phase_nhwc returns it (used in place), or the
        reference's [N, d, T] (one permute copy); evt_codes and mask [B, H, W] or [N]."""
        if z_phase.dim() == 3:
            n, d, t = z_phase.shape
            z_phase = z_phase.permute(2, 0, 1).contiguous().view(1, t, n, 1, d)    # the documented copy
            self.phase.partial_fit(z_phase, evt_codes.reshape(1, -1, 1), None if mask is None else mask.reshape(1, -1, 1))
        else:
            self.phase.partial_fit(z_phase, evt_codes, mask)
        self.gamma.partial_fit(gamma, evt_codes, mask)

    def add_probe(self, evt_codes: torch.Tensor, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """pred and target [B, T, H, W, C], [B, H, W, C] or [N, C]; mask per pixel or per timestep."""
        if self.probe is None:
            return
        self.probe.partial_fit(torch.cat([pred - target, target], dim=-1), evt_codes, mask)

    @property
    def unmatched_(self) -> int:
        return self.gamma.unmatched_

    def all_evt_codes(self) -> List[int]:
        n = self.gamma.count_
        return [c for c, i in sorted(self._index.items()) if n[i] > 0]

    def n_pixels(self, e: int) -> int:
        i = self._index.get(int(e))
        return 0 if i is None else int(self.gamma.count_[i])

    def gamma_stats(self, e: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean_gamma [d_phase], std_gamma [d_phase]) float64; zeros for an empty class."""
        i = self._index.get(int(e))
        if i is None or self.gamma.count_[i] == 0:
            z = torch.zeros(self.d_phase, dtype=torch.float64)
            return z, z
        return torch.from_numpy(self.gamma.mean()[i].copy()), torch.from_numpy(np.sqrt(self.gamma.var()[i]))

    def temporal_frac(self, e: int) -> torch.Tensor:
        """E[Var(z | pixel)] / (E[Var(z | pixel)] + Var(E[z | pixel])) per channel; zeros for an empty class."""
        i = self._index.get(int(e))
        if i is None or self.phase.count_[i] == 0:
            return torch.zeros(self.d_phase, dtype=torch.float64)
        within = self.phase.within_[i] / self.phase.count_[i]
        total = np.maximum(within + self.phase.var()[i], 1e-12)
        return torch.from_numpy(within / total)

    def probe_r2(self, e: int) -> Optional[torch.Tensor]:
        """Per-channel R^2, or None without a probe or for a class with no probe observation."""
        i = None if self.probe is None else self._index.get(int(e))
        if i is None or self.probe.count_[i] == 0:
            return None
        c = self.n_target_ch
        n, s1, s2 = self.probe.pivoted()
        ssres = self.probe.sumsq()[i, :c]
        sstot = np.maximum(s2[i, c:] - s1[i, c:] ** 2 / n[i], 1e-12)
        return torch.from_numpy(1.0 - ssres / sstot)


# ---- recovery curves ------------------------------------------------------------------------------------------------------------------
class RecoveryCurves:
    """phase_recovery_curves.py's `EvtReservoir` and the rows of its `save_csv`, over every observation instead of a reservoir of
    10 000 per class: per (EVT class, ysfc bin) the quartiles of predicted NBR and the median of observed NBR, exact
    (quantiles.GroupedQuantiles over the columns [pred_nbr, obs_nbr], one row label per bin).

    An observation counts where its mask is set and 0 <= ysfc <= max_ysfc; one at or beyond the last bin edge (or below the first, with
    bins that do not start at 0) falls into no bin but still counts in `n_seen`, as in the reference.  `n_seen`, `pixel_counts` and
    `top_codes` run the select of `table` and keep it, so `top_codes` followed by `table` selects once.  `capacity` is the number of observations the device buffer holds (12 bytes each); `table`
    raises if more arrived.  Plots, the CSV file and data loading are the caller's."""

    def __init__(self, codes: Sequence[int], bins: Sequence[Tuple[int, int]] = RECOVERY_YSFC_BINS, max_ysfc: float = 30.0, capacity: int = 1 << 22,
                 labels: Optional[Sequence[str]] = None, workgroups: int = 0):
        from .quantiles import GroupedQuantiles
        self.bins = [(float(a), float(b)) for a, b in bins]
        self._edges = [a for a, _ in self.bins] + [self.bins[-1][1]]
        if any(self.bins[i][1] != self._edges[i + 1] for i in range(len(self.bins))) or any(a >= b for a, b in zip(self._edges, self._edges[1:])):
            raise ValueError("RecoveryCurves: bins must be contiguous and increasing")
        if labels is None:
            labels = RECOVERY_YSFC_BIN_LABELS if list(bins) == RECOVERY_YSFC_BINS else [f"{a:g}-{b:g}" for a, b in self.bins]
        if len(labels) != len(self.bins):
            raise ValueError(f"RecoveryCurves: {len(labels)} labels for {len(self.bins)} bins")
        self.labels, self.max_ysfc = list(labels), float(max_ysfc)
        # the last row: outside the bins; counts asked for before table() run table()'s select
        self._q = GroupedQuantiles(codes, 2, n_rows=len(self.bins) + 1, capacity=capacity, workgroups=workgroups, default_probs=(0.25, 0.5, 0.75))
        self._index = {c: i for i, c in enumerate(self._q.codes)}

    def add(self, evt_grid: torch.Tensor, ysfc: torch.Tensor, pred_nbr: torch.Tensor, obs_nbr: torch.Tensor, mask: Optional[torch.Tensor] = None) -> None:
        """evt_grid [B, ...] (int32 or float32 codes); ysfc, pred_nbr and obs_nbr [B, T, ...]; mask per pixel [B, ...] or per timestep."""
        name = "RecoveryCurves.add"
        _need_gpu(name, evt_grid, ysfc, pred_nbr, obs_nbr, mask)
        _, b, shape = _codes_rows(evt_grid, name)
        for what, v in (("ysfc", ysfc), ("pred_nbr", pred_nbr), ("obs_nbr", obs_nbr)):
            if v.dim() != len(shape) + 2 or v.shape[0] != b or tuple(v.shape[2:]) != tuple(shape) or v.shape[1] != ysfc.shape[1]:
                raise ValueError(f"{name}: {what} must be [B, T, ...] = {(b, 'T') + tuple(shape)}, got {tuple(v.shape)}")
        t = ysfc.shape[1]
        y = ysfc.float()
        keep = (y >= 0) & (y <= self.max_ysfc)
        if mask is not None:
            m = mask if mask.dtype == torch.bool else mask != 0
            keep = keep & (m.unsqueeze(1) if m.dim() == ysfc.dim() - 1 else m)
        idx = torch.bucketize(y, torch.tensor(self._edges, dtype=torch.float32, device=y.device), right=True) - 1
        rows = torch.where(keep & (idx >= 0), idx, torch.full_like(idx, len(self.bins))).to(torch.int32)   # below the first edge: no bin either
        values = torch.stack([pred_nbr.float(), obs_nbr.float()], dim=-1).view(b, t, -1, 1, 2)
        self._q.partial_fit(values, evt_grid.reshape(b, -1, 1), rows.view(b, t, -1, 1), keep.view(b, t, -1, 1))

    def reset(self) -> None:
        """Forgets every observation; the device buffer is kept."""
        self._q.reset()

    @property
    def unmatched_(self) -> int:
        return self._q.unmatched_

    @property
    def nonfinite_(self) -> int:
        """Counted observations left out because pred_nbr or obs_nbr was not finite."""
        return self._q.nonfinite_

    @property
    def dropped_(self) -> int:
        return self._q.dropped_

    def pixel_counts(self) -> Dict[int, int]:
        """n_seen per EVT class with an observation (pixel x timestep observations, those beyond the last bin included)."""
        n = self._q.count_.sum(axis=0)
        return {c: int(n[i]) for c, i in sorted(self._index.items()) if n[i] > 0}

    def n_seen(self, code: int) -> int:
        i = self._index.get(int(code))
        return 0 if i is None else int(self._q.count_[:, i].sum())

    def top_codes(self, k: int) -> List[int]:
        """The k classes of most observations, descending (the reference's top-K; ties by the lower code)."""
        return [c for c, _ in sorted(self.pixel_counts().items(), key=lambda cv: (-cv[1], cv[0]))[:int(k)]]

    def table(self, top_codes: Sequence[int]) -> List[dict]:
        """The rows of the reference's save_csv without evt_name: evt_code, ysfc_bin, n_samples, pred_nbr_q25, pred_nbr_median,
        pred_nbr_q75, obs_nbr_median per class of top_codes and bin with an observation."""
        qv = self._q.quantiles([0.25, 0.5, 0.75])                                  # [bins + 1, G, 2, 3]
        n = self._q.count_
        rows = []
        for code in top_codes:
            i = self._index.get(int(code))
            if i is None:
                continue
            for r, label in enumerate(self.labels):
                if n[r, i] == 0:
                    continue
                rows.append({"evt_code": int(code), "ysfc_bin": label, "n_samples": int(n[r, i]), "pred_nbr_q25": float(qv[r, i, 0, 0]),
                             "pred_nbr_median": float(qv[r, i, 0, 1]), "pred_nbr_q75": float(qv[r, i, 0, 2]), "obs_nbr_median": float(qv[r, i, 1, 1])})
        return rows
