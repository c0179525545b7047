"""Phase pair mining on the GPU: the `pair_indices` / `pair_weights` that the phase soft-neighbourhood chain starts from.

`build_phase_pairs` keeps the reference's signature and result layout (frl/losses/phase_pairs.py:74-253; called per sample from
frl/training/representation/step.py, process_batch): per anchor the k nearest anchors in spectral space, kept when the two pixels share at
least `min_overlap` distinct ysfc values, anchors dropped when fewer than `min_pairs` of their neighbours are kept, weights
exp(-|spec_i - spec_j|_2 / sigma); cross pairs first, ordered by anchor and neighbour rank, then the self pairs (i, i) of the surviving
anchors.  `build_phase_pairs_batched` does this for every sample (segment of the rows) of a batch in one launch and returns the
per-segment results shifted and concatenated: what step.py pools with `cross_phase_pairs.append(phase_pairs + cross_phase_n_offset)`.

Everything up to the fixed-shape [N, k] outputs runs in `frl_phase_pairs` (csrc/phase_pairs.hip): no [N, N] distance or overlap matrix,
no [N, classes] presence matrix.  One host read (the per-segment counters and the invalid-ysfc flag, 4 S + 1 integers) sizes the outputs;
the compaction is one `nonzero_static` over `keep`.  Neighbour order on exactly tied distances is (distance, index) here; torch.topk
leaves it unspecified.  ysfc values are truncated as `.long()` does and must lie in 0..255: a NaN, an infinity, a negative value or a
value of 256 or more raises ValueError (the reference fails in scatter_ or returns garbage for these).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from .evt_soft_neighborhood import _segments

_COUNT_KEYS = ("n_anchors", "n_anchors_surviving", "n_candidates", "n_after_overlap", "n_self_pairs", "n_total_pairs")
_DIST_KEYS = ("dist_mean", "dist_std", "dist_q25", "dist_q50", "dist_q75", "dist_min", "dist_max")


def _empty_stats(n: int, n_candidates: int = 0) -> dict:
    """The reference's ten-key dict of an empty result (it fills in n_candidates only, even when pairs passed the overlap filter)."""
    return {"n_anchors": n, "n_anchors_surviving": 0, "n_candidates": n_candidates, "n_after_overlap": 0, "n_self_pairs": 0,
            "n_total_pairs": 0, "overlap_mean": 0.0, "overlap_min": 0, "weight_mean": 0.0, "weight_std": 0.0}


def _float_stats(ov: torch.Tensor, w: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """The kept cross pairs of one segment (at least one) -> eleven float64 values on the device."""
    w, d = w.double(), d.double()
    zero = torch.zeros((), dtype=torch.float64, device=w.device)
    many = w.numel() > 1
    q = torch.quantile(d, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64, device=d.device))
    return torch.stack([ov.sum().double(), ov.min().double(), w.mean(), w.std() if many else zero, d.mean(), d.std() if many else zero,
                        q[0], q[1], q[2], d.min(), d.max()])


def _mine(spec_features, ysfc, segment_offsets, k, min_overlap, min_pairs, include_self, sigma, self_pair_weight, stats):
    """-> (pair_indices, pair_weights, list of per-segment stats dicts or None)."""
    if spec_features.dim() != 2 or ysfc.dim() != 2 or ysfc.shape[0] != spec_features.shape[0]:
        raise ValueError(f"expected spec_features [N, C] and ysfc [N, T], got {tuple(spec_features.shape)} and {tuple(ysfc.shape)}")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"k must be in 1..64 (one lane per neighbour), got {k}")
    if not float(sigma) > 0.0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    n, dev, k = spec_features.shape[0], spec_features.device, int(k)
    seg_host, seg = _segments(segment_offsets, n, dev)
    lengths = (seg_host[1:] - seg_host[:-1]).tolist()
    s = len(lengths)
    empty = (torch.zeros((0, 2), dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.float32, device=dev))
    if max(lengths) < 2:                                                 # no anchor has a neighbour: the reference's first early return
        return (*empty, [_empty_stats(ln) for ln in lengths] if stats else None)
    out = ops.phase_pairs(spec_features.float().contiguous(), ysfc.float().contiguous(), seg, seg_host, k, math.ceil(min_overlap),
                          math.ceil(min_pairs), float(sigma))
    meta = out["meta"].cpu().tolist()                                    # the one host read: sizes the outputs, carries the flag
    if meta[-1]:
        raise ValueError("ysfc must hold finite values in 0..255 (a NaN, an infinity, a negative value or a value >= 256 was found)")
    counters = [meta[4 * j:4 * j + 4] for j in range(s)]
    cross = [c[2] for c in counters]
    # with min_pairs <= 0 every anchor passes, but a sample without one cross pair still returns empty
    surviving = [c[3] if c[2] > 0 else 0 for c in counters]
    n_self = surviving if include_self else [0] * s
    p_cross, p_self = sum(cross), sum(n_self)
    if p_cross == 0:
        return (*empty, [_empty_stats(ln, c[0]) for ln, c in zip(lengths, counters)] if stats else None)
    e = torch.nonzero_static(out["keep"].reshape(-1), size=p_cross).reshape(-1)      # ascending: by anchor, then by neighbour rank
    anchor = torch.div(e, k, rounding_mode="floor")
    cross_pairs = torch.stack([anchor, out["knn_idx"].reshape(-1)[e].long()], dim=1)
    cross_w = out["weight"].reshape(-1)[e]
    if p_self == 0:
        pairs, weights = cross_pairs, cross_w
    else:
        ok = out["anchor_ok"]
        seg_id = None
        if s > 1:
            seg_id = torch.repeat_interleave(torch.arange(s, device=dev), torch.tensor(lengths, device=dev), output_size=n)
            if any(c[3] != sv for c, sv in zip(counters, surviving)):
                ok = ok * torch.tensor([1 if c > 0 else 0 for c in cross], dtype=torch.uint8, device=dev)[seg_id]
        self_anchor = torch.nonzero_static(ok, size=p_self).reshape(-1)
        self_pairs = self_anchor.unsqueeze(1).expand(-1, 2)
        self_w = torch.full((p_self,), float(self_pair_weight), dtype=torch.float32, device=dev)
        if s == 1:
            pairs, weights = torch.cat([cross_pairs, self_pairs], dim=0), torch.cat([cross_w, self_w], dim=0)
        else:                                                            # [cross_s; self_s] segment by segment
            cross_end = np.cumsum(cross)
            self_start = np.cumsum(n_self) - np.asarray(n_self)
            pos_c = torch.arange(p_cross, device=dev) + torch.tensor(self_start, device=dev)[seg_id[anchor]]
            pos_s = torch.arange(p_self, device=dev) + torch.tensor(cross_end, device=dev)[seg_id[self_anchor]]
            pairs = torch.empty((p_cross + p_self, 2), dtype=torch.long, device=dev)
            weights = torch.empty(p_cross + p_self, dtype=torch.float32, device=dev)
            pairs[pos_c], pairs[pos_s] = cross_pairs, self_pairs
            weights[pos_c], weights[pos_s] = cross_w, self_w
    if not stats:
        return pairs, weights, None
    ov, dist = out["overlap"].reshape(-1)[e], out["dist"].reshape(-1)[e]
    bounds = np.concatenate([[0], np.cumsum(cross)]).tolist()
    live = [j for j in range(s) if cross[j] > 0]
    floats = torch.stack([_float_stats(ov[bounds[j]:bounds[j + 1]], cross_w[bounds[j]:bounds[j + 1]], dist[bounds[j]:bounds[j + 1]])
                          for j in live]).cpu().tolist()
    per_segment = [_empty_stats(ln, c[0]) for ln, c in zip(lengths, counters)]
    for j, f in zip(live, floats):
        c = counters[j]
        # the reference takes the mean of the float32 overlaps: an exact integer sum, one correctly rounded float32 division
        per_segment[j] = {"n_anchors": lengths[j], "n_anchors_surviving": surviving[j], "n_candidates": c[0], "n_after_overlap": c[1],
                          "n_self_pairs": n_self[j], "n_total_pairs": cross[j] + n_self[j],
                          "overlap_mean": float(np.float32(f[0]) / np.float32(cross[j])), "overlap_min": int(f[1]), "weight_mean": f[2],
                          "weight_std": f[3], **dict(zip(_DIST_KEYS, f[4:]))}
    return pairs, weights, per_segment


def build_phase_pairs(spec_features: torch.Tensor, ysfc: torch.Tensor, k: int = 16, min_overlap: int = 3, min_pairs: int = 5,
                      include_self: bool = True, sigma: float = 5.0, self_pair_weight: float = 1.0, *,
                      stats: bool = True) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """spec_features [N, C] (C <= 256), ysfc [N, T] integer-valued in 0..255, both on the GPU -> (pair_indices [P, 2] int64,
    pair_weights [P] float32, stats).  The reference's function: cross pairs by anchor and neighbour rank, then the self pairs of the
    surviving anchors with weight self_pair_weight; [0, 2] / [0] when N < 2 or nothing survives.  1 <= k <= 64.  stats: the reference's
    keys (the ten it documents and dist_mean / std / q25 / q50 / q75 / min / max; its ten-key dict with only n_candidates filled in when no
    cross pair is left), float64 reductions of the float32 kernel outputs; stats=False returns {} and costs no host read beyond the one
    that sizes the outputs."""
    pairs, weights, per_segment = _mine(spec_features, ysfc, [0, spec_features.shape[0]], k, min_overlap, min_pairs, include_self, sigma,
                                        self_pair_weight, stats)
    return pairs, weights, per_segment[0] if stats else {}


def build_phase_pairs_batched(spec_features: torch.Tensor, ysfc: torch.Tensor, segment_offsets, k: int = 16, min_overlap: int = 3,
                              min_pairs: int = 5, include_self: bool = True, sigma: float = 5.0, self_pair_weight: float = 1.0, *,
                              stats: bool = True) -> tuple[torch.Tensor, torch.Tensor, dict]:
    """Every sample of a batch in one launch: spec_features [N, C], ysfc [N, T], segment_offsets [S + 1] rising from 0 to N (a list or a
    CPU tensor costs no synchronisation; segments may be empty; anchors only ever see anchors of their own segment).  The result is the
    concatenation over the segments of what build_phase_pairs returns for the segment's rows, indices shifted by the segment's offset,
    bit for bit: it indexes the pooled rows, ready for phase_neighborhood_loss.  stats: the integer counts summed over the segments and
    "per_segment", the list of the single-call dicts (the float statistics appear only there); stats=False returns {}."""
    pairs, weights, per_segment = _mine(spec_features, ysfc, segment_offsets, k, min_overlap, min_pairs, include_self, sigma,
                                        self_pair_weight, stats)
    if not stats:
        return pairs, weights, {}
    out = {key: sum(st[key] for st in per_segment) for key in _COUNT_KEYS}
    out["per_segment"] = per_segment
    return pairs, weights, out
