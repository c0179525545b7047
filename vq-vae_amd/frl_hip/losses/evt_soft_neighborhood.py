"""EVT-guided soft-neighbourhood loss on the HIP path: `EvtDiffusionMetric` and `evt_soft_neighborhood_loss` with the reference's
signatures and results (frl/losses/evt_soft_neighborhood.py; caller frl/training/representation/step.py:540), and the batched form that
takes every sample of a batch in one forward launch pair and one backward launch.

The metric is built on the host with numpy exactly as the reference builds it (the confusion table is read with the `csv` module: no
pandas) and looks codes up with integer tensor ops on the device: no `.item()`, no Python loop over anchors, no host synchronisation.

Per segment (one sample's anchors), with idx = metric.code_index(evt_codes):

    anchor i valid       iff idx[i] >= 0;   pair (i, j) in the mask iff both valid and idx[i] != idx[j];   row i active iff >= 2 pairs
    a_ij = -(1 - S[idx_i, idx_j]) / tau_ref,  b_ij = -|e_i - e_j|_2 / tau_learned,  p = softmax_j a,  q = softmax_j b   over the mask
    loss = sum_i w[idx_i] active_i KL(p_i || q_i) / sum_i w[idx_i] active_i

and 0 (with a zero gradient) with fewer than min_valid_anchors valid anchors, no active row or a zero weight sum.  No [M, M] array is
written in either direction (csrc/evt_soft_neighborhood.hip); a pair at distance 0 has zero gradient (torch.cdist's convention).  Loss and
gradients are bit-reproducible, float32 whatever the dtype of the embeddings; the gradient has their dtype.

Diagnostics: the reference's keys except `median_d_learned` and `mean_rank_confused`, which need sorts of the distance matrix and are not
produced."""
from __future__ import annotations

import csv
import math
from pathlib import Path
from typing import Optional

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops

_SUMMARY_COLS = ("Row Totals", "Percent Row Agreement")
_SUMMARY_ROWS = ("Column Totals", "Percent Column Agreement")


def _int_label(text: str) -> int:
    try:
        return int(text)
    except ValueError:
        return int(float(text))


def _read_confusion(path) -> tuple[list[int], list[int], np.ndarray]:
    """The contingency table without its summary rows and columns -> (row codes, column codes, float64 counts [rows, columns])."""
    with open(path, newline="") as fh:
        table = [row for row in csv.reader(fh) if row]
    header = [c.strip() for c in table[0][1:]]
    cols = [k for k, name in enumerate(header) if name not in _SUMMARY_COLS]
    rows = [r for r in table[1:] if r[0].strip() and r[0].strip() not in _SUMMARY_ROWS]
    cell = lambda r, k: float(r[k + 1]) if k + 1 < len(r) and r[k + 1].strip() else float("nan")  # noqa: E731
    values = np.array([[cell(r, k) for k in cols] for r in rows], dtype=np.float64).reshape(len(rows), len(cols))
    return [_int_label(r[0].strip()) for r in rows], [_int_label(header[k]) for k in cols], values


class EvtDiffusionMetric:
    """Diffusion-distance metric derived from the EVT confusion table: the reference's constructor, filters and arithmetic.

    confusion_csv: the combined EVT contingency table (row and column labels are integer LANDFIRE codes, with or without the summary
    rows and columns); code_counts: code -> regional pixel count (keys may be strings).  Codes below `min_count`, absent from either
    source, or with fewer than `min_confusion_samples` samples among the kept codes are dropped.  S = P^diffusion_steps of the
    symmetrised, optionally Laplace-smoothed, row-normalised table (rows without any count: uniform), optionally dichotomised at
    `binary_threshold` with a zeroed diagonal and renormalised; the weights are median_freq / freq capped at `max_weight`."""

    def __init__(self, confusion_csv: str | Path, code_counts: dict, min_count: int = 100, min_confusion_samples: int = 30,
                 diffusion_steps: int = 2, laplace_smoothing: float = 0.0, binary_threshold: float = 0.0, max_weight: float = 10.0) -> None:
        self.max_weight = max_weight
        self._device = torch.device("cpu")
        row_codes, col_codes, values = _read_confusion(confusion_csv)
        row_of = {c: k for k, c in enumerate(row_codes)}
        col_of = {c: k for k, c in enumerate(col_codes)}

        def reindex(codes):                                             # rows and columns `codes`, zeros where the table has neither
            out = np.zeros((len(codes), len(codes)), dtype=np.float64)
            for a, ca in enumerate(codes):
                for b, cb in enumerate(codes):
                    if cb in col_of:
                        out[a, b] = values[row_of[ca], col_of[cb]]
            return out

        int_counts = {int(k): float(v) for k, v in code_counts.items()}
        valid_codes = {code for code, cnt in int_counts.items() if cnt >= min_count}
        keep = sorted(c for c in row_codes if c in valid_codes)
        if min_confusion_samples > 0:
            sums = np.nansum(reindex(keep), axis=1)
            keep = sorted(c for c, s in zip(keep, sums) if s >= min_confusion_samples)
        if len(keep) < 2:
            raise ValueError(f"Fewer than 2 EVT codes survive the filters (min_count={min_count}, "
                             f"min_confusion_samples={min_confusion_samples}). Lower the thresholds or check that the stats file covers "
                             f"your region.")
        C = reindex(keep)
        C_sym = (C + C.T) / 2.0
        if laplace_smoothing > 0.0:
            C_sym = C_sym + laplace_smoothing
        row_sums = C_sym.sum(axis=1, keepdims=True)
        uniform = np.full(C_sym.shape, 1.0 / C_sym.shape[0])
        P = np.where(row_sums > 0, C_sym / np.where(row_sums > 0, row_sums, 1.0), uniform)
        Pk = np.linalg.matrix_power(P, diffusion_steps)
        if binary_threshold > 0.0:
            Pk_bin = (Pk > binary_threshold).astype(float)
            np.fill_diagonal(Pk_bin, 0.0)
            row_sums_bin = Pk_bin.sum(axis=1, keepdims=True)
            uniform_bin = np.full(Pk_bin.shape, 1.0 / Pk_bin.shape[0])
            Pk = np.where(row_sums_bin > 0, Pk_bin / np.where(row_sums_bin > 0, row_sums_bin, 1.0), uniform_bin)
        self._S = torch.tensor(Pk, dtype=torch.float32)
        self._code_to_idx: dict[int, int] = {code: i for i, code in enumerate(keep)}
        self._codes = torch.tensor(keep, dtype=torch.int64)             # ascending: code_index searches it

        counts = np.array([int_counts.get(c, 0.0) for c in keep], dtype=np.float64)
        total = counts.sum()
        freqs = counts / total if total > 0 else np.ones_like(counts) / len(counts)
        median_freq = float(np.median(freqs[freqs > 0])) if (freqs > 0).any() else 1.0
        raw_weights = np.where(freqs > 0, median_freq / np.where(freqs > 0, freqs, 1.0), 0.0)
        raw_weights = np.clip(raw_weights, 0.0, max_weight)
        self._freq_weights = torch.tensor(raw_weights, dtype=torch.float32)

    def to(self, device) -> "EvtDiffusionMetric":
        """Move internal tensors to *device*; returns self."""
        self._device = torch.device(device)
        self._S = self._S.to(self._device)
        self._freq_weights = self._freq_weights.to(self._device)
        self._codes = self._codes.to(self._device)
        return self

    def code_index(self, codes: torch.Tensor) -> torch.Tensor:
        """codes: int tensor of LANDFIRE codes (any shape, on the metric's device) -> int32 indices into the metric, -1 for a code it does
        not hold (negative codes and codes above the largest known one included).  Integer tensor ops only: no host synchronisation."""
        c = codes.to(self._device, torch.int64)
        pos = torch.searchsorted(self._codes, c.contiguous()).clamp_(max=self._codes.numel() - 1)
        return torch.where(self._codes[pos] == c, pos, torch.full_like(pos, -1)).to(torch.int32)

    def reference_distances(self, codes: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """codes [N] -> (d_ref [N, N] = 1 - diffused similarity, 1.0 where either code is unknown; valid [N] bool)."""
        idx = self.code_index(codes)
        valid = idx >= 0
        safe = idx.clamp(min=0).to(torch.int64)
        sim = self._S[safe[:, None], safe[None, :]]
        sim = torch.where(valid[:, None] & valid[None, :], sim, torch.zeros_like(sim))
        return 1.0 - sim, valid

    def anchor_weights(self, codes: torch.Tensor) -> torch.Tensor:
        """codes [N] -> inverse-frequency weight per anchor, 0.0 for unknown codes."""
        idx = self.code_index(codes)
        w = self._freq_weights[idx.clamp(min=0).to(torch.int64)]
        return torch.where(idx >= 0, w, torch.zeros_like(w))

    @property
    def n_codes(self) -> int:
        return len(self._code_to_idx)

    @property
    def valid_codes(self) -> set:
        return set(self._code_to_idx.keys())


class _EvtFn(Function):
    @staticmethod
    def forward(ctx, emb, idx, table, code_weights, seg, seg_host, seg_weights, tau_ref, tau_learned, min_valid):
        segout, segstat, rowstat = ops.evt_soft_nbr_fwd(emb, idx, table, code_weights, seg, seg_host, tau_ref, tau_learned, min_valid)
        ctx.save_for_backward(emb, idx, table, code_weights, seg, seg_weights, rowstat, segout)
        ctx.seg_host, ctx.hp = seg_host, (tau_ref, tau_learned)
        raw = segout[:, 0]
        ctx.mark_non_differentiable(segstat, raw)
        return (raw.clone() if seg_weights is None else raw * seg_weights), segstat, raw                # the backward kernel applies the weights

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _, __):
        emb, idx, table, code_weights, seg, seg_weights, rowstat, segout = ctx.saved_tensors
        grad = ops.evt_soft_nbr_bwd(emb, idx, table, code_weights, seg, ctx.seg_host, *ctx.hp, rowstat, segout, g.float().contiguous(),
                                    seg_weights)
        return grad, None, None, None, None, None, None, None, None, None


_MEAN_KEYS = ("mean_kl", "mean_entropy_ref", "mean_entropy_learned", "d_lrn_confused", "d_lrn_noncf", "n_confused_pairs", "eff_n_ref")


def _segment_stats(row, n_in: int, min_valid: int) -> dict:
    """row: the twelve doubles of one segment (include/frl_hip.h), already on the host."""
    loss, live, n_valid, n_active, ent_p, ent_q, ncf_active, ncf, dcf, dnc, nnc, _ = (float(v) for v in row)
    out = {"n_anchors_in": n_in, "n_anchors_valid": int(n_valid), "n_rows_active": int(n_active) if n_valid >= min_valid else 0}
    out.update({k: 0.0 for k in _MEAN_KEYS})
    if live > 0:
        ent_ref = ent_p / n_active
        out.update(mean_kl=loss, mean_entropy_ref=ent_ref, mean_entropy_learned=ent_q / n_active, d_lrn_confused=dcf / ncf if ncf > 0 else 0.0,
                   d_lrn_noncf=dnc / nnc if nnc > 0 else 0.0, n_confused_pairs=ncf_active / n_active, eff_n_ref=math.exp(ent_ref))
    return out


def _segments(segment_offsets, n: int, device):
    """-> (offsets int32 on the host, the same on the device).  Offsets given on the host cost no synchronisation."""
    host = torch.as_tensor(segment_offsets).detach().to("cpu", torch.int64).reshape(-1)
    if host.numel() < 2 or int(host[0]) != 0 or int(host[-1]) != n or bool((host[1:] < host[:-1]).any()):
        raise ValueError(f"segment_offsets must rise from 0 to N = {n} without decreasing, got {host.tolist()}")
    host = host.to(torch.int32).contiguous()
    return host, host.to(device)


def _run(embeddings, evt_codes, segment_offsets, metric, tau_ref, tau_learned, min_valid_anchors, segment_weights):
    """-> (per-segment losses [S] float32 times segment_weights, carrying the gradient; the unweighted losses, detached; per-segment
    statistics as a list of dicts)."""
    if embeddings.dim() != 2 or evt_codes.shape != (embeddings.shape[0],):
        raise ValueError(f"expected embeddings [N, D] and evt_codes [N], got {tuple(embeddings.shape)} and {tuple(evt_codes.shape)}")
    n, dev = embeddings.shape[0], embeddings.device
    seg_host, seg = _segments(segment_offsets, n, dev)
    s = seg_host.numel() - 1
    lengths = (seg_host[1:] - seg_host[:-1]).tolist()
    w = None
    if segment_weights is not None:
        if segment_weights.shape != (s,):
            raise ValueError(f"segment_weights must have shape [{s}], got {tuple(segment_weights.shape)}")
        w = segment_weights.detach().to(dev, torch.float32).contiguous()
    if n == 0:
        zeros = torch.zeros(s, dtype=torch.float32, device=dev) + 0.0 * embeddings.sum()
        return zeros, zeros.detach(), [_segment_stats([0.0] * 12, 0, min_valid_anchors) for _ in range(s)]
    e = embeddings if embeddings.dtype in (torch.float32, torch.bfloat16) else embeddings.float()
    idx = metric.code_index(evt_codes.to(dev))
    per_seg, segstat, raw = _EvtFn.apply(e.contiguous(), idx.contiguous(), metric._S, metric._freq_weights, seg, seg_host, w, float(tau_ref),
                                    float(tau_learned), int(min_valid_anchors))
    host = segstat.cpu().tolist()                                       # the one device-to-host copy of the diagnostics
    return per_seg, raw, [_segment_stats(row, ln, min_valid_anchors) for row, ln in zip(host, lengths)]


def evt_soft_neighborhood_loss(embeddings: torch.Tensor, evt_codes: torch.Tensor, metric: EvtDiffusionMetric, tau_ref: float = 0.5,
                               tau_learned: float = 0.5, min_valid_anchors: int = 4) -> tuple[torch.Tensor, dict]:
    """embeddings [N, D] (float32 | bfloat16, D <= 256), evt_codes [N] integer LANDFIRE codes -> (loss 0-dim float32, stats).  The
    reference's function; `metric` must live on the device of the embeddings.  stats: n_anchors_in, n_anchors_valid, n_rows_active,
    mean_kl, mean_entropy_ref, mean_entropy_learned, d_lrn_confused, d_lrn_noncf, n_confused_pairs, eff_n_ref (zeros where the reference
    returns early); `median_d_learned` and `mean_rank_confused` need sorts of the distance matrix and are not produced."""
    per_seg, _, stats = _run(embeddings, evt_codes, [0, embeddings.shape[0]], metric, tau_ref, tau_learned, min_valid_anchors, None)
    return per_seg[0], stats[0]


def evt_soft_neighborhood_loss_batched(embeddings: torch.Tensor, evt_codes: torch.Tensor, segment_offsets, metric: EvtDiffusionMetric,
                                       tau_ref: float = 0.5, tau_learned: float = 0.5, min_valid_anchors: int = 4,
                                       segment_weights: Optional[torch.Tensor] = None, reduction: str = "mean") -> tuple[torch.Tensor, dict]:
    """The loss of every segment (sample) of a batch at once: embeddings [N, D], evt_codes [N], segment_offsets [S + 1] rising from 0 to N
    (a list or a CPU tensor costs no synchronisation; segments may be empty) -> (loss, stats).  Segment s's loss is what
    evt_soft_neighborhood_loss returns for its rows, bit for bit, times segment_weights[s] when given.  reduction: "mean" averages over
    all S segments, the zero ones included (the reference trainer's accumulation), "sum" adds them, "none" returns the [S] vector.
    stats: the counts summed over the segments, each mean statistic averaged over the segments that produced one, "per_segment_loss"
    (an [S] device tensor, unweighted, detached) and "per_segment" (a list of the single-call stats dicts)."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction must be 'mean', 'sum' or 'none', got {reduction!r}")
    weighted, raw, seg_stats = _run(embeddings, evt_codes, segment_offsets, metric, tau_ref, tau_learned, min_valid_anchors, segment_weights)
    loss = weighted if reduction == "none" else weighted.sum() if reduction == "sum" else weighted.sum() / max(len(seg_stats), 1)
    stats = {k: sum(s[k] for s in seg_stats) for k in ("n_anchors_in", "n_anchors_valid", "n_rows_active")}
    produced = [s for s in seg_stats if s["eff_n_ref"] > 0.0]
    stats.update({k: (sum(s[k] for s in produced) / len(produced) if produced else 0.0) for k in _MEAN_KEYS})
    stats["per_segment_loss"] = raw
    stats["per_segment"] = seg_stats
    return loss, stats
