"""Exact quantiles on the GPU, plain and grouped: what the reference computes from a sample wherever it needs a quantile
(frl/training/phase_recovery_curves.py and ysfc_evt_histograms.py from per-class reservoirs, representation/step.py `compute_stats` from a
randperm subsample of 2^23 values because torch.quantile refuses more than 2^24, data/stats from at most 100 000 stored samples), here
over every observation.

csrc/quantile.hip finds the two order statistics that bracket a quantile by radix select on a monotone key: no sort, no per-pixel host
copy, no sampling, and no host read between its passes.  For a cell of n values and a probability q, with v = (n - 1) q in float64,
k = floor(v) and t = v - k, it returns lo = x_(k), hi = x_(min(k + 1, n - 1)) and t; the quantile is lo + (hi - lo) t for t < 0.5, else
hi - (hi - lo) (1 - t), in float64: numpy's method="linear" applied to the float64 cast of the data.  The order statistics are exact,
bit-identical from run to run and under any permutation of the input.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .strata import _codes_rows, _mask_rows, _need_gpu, _per_pixel_or_step, _vocab

__all__ = ["masked_quantiles", "summary_stats", "GroupedQuantiles", "interpolate"]


def interpolate(lo, hi, frac):
    """lo + (hi - lo) t for t < 0.5, else hi - (hi - lo) (1 - t), in float64 (numpy's linear method); lo, hi [..., D, Q], frac [..., Q];
    torch tensors or numpy arrays."""
    if isinstance(lo, torch.Tensor):
        lo, hi, t = lo.double(), hi.double(), frac.double().unsqueeze(-2)
        return torch.where(t < 0.5, lo + (hi - lo) * t, hi - (hi - lo) * (1.0 - t))
    lo, hi, t = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(frac, np.float64)[..., None, :]
    with np.errstate(invalid="ignore"):
        return np.where(t < 0.5, lo + (hi - lo) * t, hi - (hi - lo) * (1.0 - t))


def masked_quantiles(x: torch.Tensor, q, mask: Optional[torch.Tensor] = None, workgroups: int = 0) -> torch.Tensor:
    """The quantiles q (a probability or up to 8) of the rows of x [N] or [N, D] (float32, on the GPU) that mask [N] keeps -> float64
    [Q] or [D, Q] on the device: NaN where the mask keeps nothing.  A contiguous x is read in place (no copy, no sort), any N < 2^31; a
    non-contiguous x is copied once, and a mask that is not bool costs an N-byte temporary (mask != 0).  No host read.  A NaN in x ranks
    above every number."""
    name = "masked_quantiles"
    probs = ops.chk_quantile_probs(q, name)
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2) or x.dtype != torch.float32:
        raise ValueError(f"{name}: x must be a float32 tensor [N] or [N, D], got {getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    rows = x.contiguous().view(x.shape[0], -1)
    ops.chk_quantile_dims(1, rows.shape[1], len(probs), workgroups, name)
    if rows.shape[0] < 1:
        raise ValueError(f"{name}: x is empty")
    m = None
    if mask is not None:
        if tuple(mask.shape) != (x.shape[0],):
            raise ValueError(f"{name}: mask must be [{x.shape[0]}], got {tuple(mask.shape)}")
        m = (mask if mask.dtype == torch.bool else mask != 0).contiguous().view(torch.uint8)
    _need_gpu(name, rows, m)
    _, lo, hi, frac = ops.quantile_select(probs, 1, rows.shape[1], x=rows, mask=m, workgroups=workgroups)
    out = interpolate(lo[0], hi[0], frac[0])
    return out[0] if x.dim() == 1 else out


def summary_stats(tensors: Sequence[torch.Tensor]) -> Dict[str, float]:
    """compute_stats of the reference's representation/step.py over every element of the tensors (no randperm subsample): mean, std
    (unbiased), min, max from stock torch ops, q25, q50, q75 exact; one host read."""
    keys = ["mean", "std", "min", "max", "q25", "q50", "q75"]
    tensors = list(tensors)
    if not tensors:
        return {k: 0.0 for k in keys}
    _need_gpu("summary_stats", *tensors)
    flat = [t.reshape(-1).float() for t in tensors]
    combined = flat[0] if len(flat) == 1 else torch.cat(flat)
    qs = masked_quantiles(combined, [0.25, 0.5, 0.75])
    head = torch.stack([combined.mean(), combined.std(), combined.min(), combined.max()]).double()
    vals = torch.cat([head, qs]).cpu().tolist()                                   # the one host read
    return dict(zip(keys, vals))


class GroupedQuantiles:
    """Exact quantiles per (row label, EVT code, column) over a stream of batches.

    `partial_fit` keys every observation as `ContingencyTable` and `GroupedMoments` do and appends one record (its cell and the keys of its
    n_columns values) to a device buffer of `capacity` records (4 (n_columns + 1) bytes each); nothing is read back.  An observation with a
    value that is not finite is skipped and counted in `nonfinite_`; past the capacity records are counted in `dropped_` and `quantiles`
    raises: it never returns an approximation silently.  Results are numpy arrays on the host; the last select (its probabilities, counts,
    order statistics and counters, one host read) is kept until the next `partial_fit`."""

    def __init__(self, codes: Sequence[int], n_columns: int, n_rows: int = 1, capacity: int = 1 << 22, workgroups: int = 0,
                 default_probs: Sequence[float] = (0.5,)):
        self._codes = _vocab(codes, "GroupedQuantiles")
        self._default_probs = ops.chk_quantile_probs(default_probs, "GroupedQuantiles")
        self.n_columns, self.n_rows, self.capacity, self.workgroups = int(n_columns), int(n_rows), int(capacity), int(workgroups)
        if self.n_rows < 1:
            raise ValueError(f"GroupedQuantiles: n_rows must be >= 1, got {n_rows}")
        ops.chk_quantile_dims(self.n_rows * self._codes.size, self.n_columns, 1, self.workgroups, "GroupedQuantiles")
        if not 1 <= self.capacity < 2 ** 31:
            raise ValueError(f"GroupedQuantiles: supports 1 <= capacity < 2^31 records, got {capacity}")
        self._vocab_dev = self._cells = self._keys = self._state = self._host = None

    @property
    def codes(self) -> List[int]:
        return [int(c) for c in self._codes]

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

    def partial_fit(self, values: torch.Tensor, codes: torch.Tensor, rows: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                    channels_last: bool = True) -> "GroupedQuantiles":
        """values float32 [N, D], [B, H, W, D] or [B, T, H, W, D]; codes int32 or float32 [N] / [B, H, W]; rows (integer labels in
        [0, n_rows)) and mask per pixel or per timestep."""
        name = "GroupedQuantiles.partial_fit"
        x, shape, b = self._rows(values, channels_last, name)
        c, bc, cshape = _codes_rows(codes, name)
        if (bc, tuple(cshape)) != (b, tuple(shape)) and not (b == 1 and c.numel() == x.shape[2]):
            raise ValueError(f"{name}: codes {tuple(codes.shape)} do not match values {tuple(values.shape)}")
        c = c.view(b, -1)
        m = _mask_rows(mask, b, shape, name)
        if m is not None and m.shape[1] not in (1, x.shape[1]):
            raise ValueError(f"{name}: mask {tuple(mask.shape)} does not match T = {x.shape[1]}")
        r = None
        if rows is not None:
            if not isinstance(rows, torch.Tensor) or rows.dtype.is_floating_point:
                raise ValueError(f"{name}: rows must be an integer tensor")
            r = _per_pixel_or_step(rows if rows.dtype == torch.int32 else rows.to(torch.int32), b, shape, "rows", name)
            if r.shape[1] not in (1, x.shape[1]):
                raise ValueError(f"{name}: rows {tuple(rows.shape)} do not match T = {x.shape[1]}")
        elif self.n_rows != 1:
            raise ValueError(f"{name}: this accumulator has {self.n_rows} rows: rows must be given")
        _need_gpu(name, x, c, r, m)
        if self._cells is None:
            dev = x.device
            self._vocab_dev = torch.from_numpy(self._codes).to(dev)
            self._cells = torch.empty(self.capacity, dtype=torch.int32, device=dev)
            self._keys = torch.empty(self.n_columns, self.capacity, dtype=torch.int32, device=dev)
            self._state = torch.zeros(5, dtype=torch.int64, device=dev)          # cursor, unmatched, rejected, nonfinite, dropped
        ops.quantile_append(x, c, r, m, self._vocab_dev, self.n_rows, self._cells, self._keys, self._state, self.workgroups)
        self._host = None
        return self

    def reset(self) -> "GroupedQuantiles":
        """Forgets every record and counter; the device buffer is kept."""
        if self._state is not None:
            self._state.zero_()
        self._host = None
        return self

    # ---- results ----------------------------------------------------------------------------------------------------------------
    def _select(self, q):
        """-> (probs, count [C], lo, hi [C, D, Q], frac [C, Q], state [5]) on the host, from one read."""
        probs = ops.chk_quantile_probs(q, "GroupedQuantiles")
        cells = self.n_rows * self._codes.size
        ops.chk_quantile_dims(cells, self.n_columns, len(probs), self.workgroups, "GroupedQuantiles")
        if self._host is not None and self._host[0] == probs:
            return self._host
        d, nq = self.n_columns, len(probs)
        if self._cells is None:
            nan = np.full((cells, d, nq), np.nan, np.float32)
            self._host = (probs, np.zeros(cells, np.int64), nan, nan.copy(), np.zeros((cells, nq)), np.zeros(5, np.int64))
            return self._host
        count, lo, hi, frac = ops.quantile_select(probs, cells, d, cells=self._cells, keys=self._keys, cursor=self._state, workgroups=self.workgroups)
        n1, n2 = cells * d * nq, cells * nq
        flat = torch.cat([lo.reshape(-1).double(), hi.reshape(-1).double(), frac.reshape(-1), count.double(), self._state.double()]).cpu().numpy()
        lo_h, hi_h = flat[:n1].astype(np.float32).reshape(cells, d, nq), flat[n1:2 * n1].astype(np.float32).reshape(cells, d, nq)
        o = 2 * n1 + n2
        self._host = (probs, flat[o:o + cells].astype(np.int64), lo_h, hi_h, flat[2 * n1:o].reshape(cells, nq).copy(), flat[o + cells:].astype(np.int64))
        return self._host

    def _counter(self, i: int) -> int:
        if self._cells is None:
            return 0
        if self._host is not None:
            return int(self._host[5][i])
        return int(self._state[i].item())

    @property
    def count_(self) -> np.ndarray:
        """int64 [n_rows, G]: the records of every cell.  The counts come with a select: read after `quantiles(q)` they cost nothing,
        read first they run one at `default_probs`, which a following `quantiles(default_probs)` then finds done."""
        return self._select(self._default_probs if self._host is None else self._host[0])[1].reshape(self.n_rows, -1)

    @property
    def unmatched_(self) -> int:
        """Observations with a valid code that the vocabulary does not hold."""
        return self._counter(1)

    @property
    def rejected_(self) -> int:
        """Observations whose row label lies outside [0, n_rows)."""
        return self._counter(2)

    @property
    def nonfinite_(self) -> int:
        """Observations skipped for a value that is not finite."""
        return self._counter(3)

    @property
    def dropped_(self) -> int:
        """Records that found the buffer full."""
        return self._counter(4)

    def order_statistics(self, q) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (lo float32 [R, G, D, Q], hi float32 [R, G, D, Q], frac float64 [R, G, Q]); lo and hi NaN for an empty cell."""
        _, _, lo, hi, frac, state = self._select(q)
        if state[4] > 0:
            raise RuntimeError(f"GroupedQuantiles: {int(state[4])} records did not fit the capacity of {self.capacity}: the quantiles would be approximate")
        shape = (self.n_rows, self._codes.size)
        return lo.reshape(shape + lo.shape[1:]), hi.reshape(shape + hi.shape[1:]), frac.reshape(shape + frac.shape[1:])

    def quantiles(self, q) -> np.ndarray:
        """-> float64 [R, G, D, Q]; NaN for an empty cell.  Raises when records were dropped."""
        return interpolate(*self.order_statistics(q))
