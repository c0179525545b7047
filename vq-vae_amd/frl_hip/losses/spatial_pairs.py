"""Spatial InfoNCE pair mining on the GPU: the pair block of the reference's step (frl/training/representation/step.py:325-401).

Per sample the reference calls `spatial_knn_pairs` and `spatial_negative_pairs` (frl/utils/spatial.py:176-332), maps the anchors, the
neighbours and the negatives onto their sorted unique coordinates with `torch.unique(dim=0, return_inverse=True)`, gathers the spectral
map there and weights each pair by its spectral distance d: exp(-d / tau) for a positive, 1 - exp(-d / tau) for a negative, both clamped
to [min_w, 1].  `build_spatial_pairs` returns all of that for one sample, `build_spatial_pairs_batched` for every sample (segment of the
anchors) of a batch with the same launches; a segment's slice of the batched result is what the per-sample call gives for that sample
and its slice of `draws`, with the indices shifted by the segment's offset in `unique_coords`.

Everything up to the padded [N, k] / [N, n] outputs runs in csrc/spatial_pairs.hip (include/frl_hip.h has the definitions): a packed bit
mask, popcounts under column intervals, a bitmap rank in place of torch.unique, the weights read straight from the map.  One host read
per call (3 S + 2 integers: pairs and unique coordinates per segment, the out-of-range flags) sizes the ragged outputs; everything
before it is a fixed sequence of launches, and the compaction after it is two `nonzero_static`.  Nothing here is differentiable.
Deviation from the reference: its `torch.randperm` stream is not reproduced.  The negatives are a function of `draws` (uniform without
replacement over the same candidate set, the same sampling law); neighbours at one distance come in (dr, dc) order, which the
reference's unstable argsort leaves open.
"""
from __future__ import annotations

import torch

from .. import ops
from ..utils import spatial as sp
from .evt_soft_neighborhood import _segments

MAX_CHANNELS = 256


def _mine(anchors, masks, feats, segment_offsets, k, max_radius, min_distance, max_distance, n_per_anchor, tau, min_w, generator, draws):
    sp.check_knn_args(k, max_radius)
    sp.check_negative_args(min_distance, max_distance, n_per_anchor)
    if not float(tau) > 0.0:
        raise ValueError(f"tau must be positive, got {tau}")
    sp.check_anchors_and_masks(anchors, masks, 3)
    s, h, w = masks.shape
    if feats.dim() != 4 or feats.shape[0] != s or tuple(feats.shape[2:]) != (h, w) or feats.dtype != torch.float32:
        raise ValueError(f"the feature maps must be a float32 [{s}, C, {h}, {w}] tensor, got {tuple(feats.shape)} {feats.dtype}")
    if not 1 <= feats.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"at most {MAX_CHANNELS} feature channels, got {feats.shape[1]}")
    n, dev, n_per = anchors.shape[0], anchors.device, int(n_per_anchor)
    sp.check_draws(draws, n, n_per)
    seg_host, _ = _segments(segment_offsets, n, "cpu")
    if seg_host.numel() != s + 1:
        raise ValueError(f"segment_offsets must have {s + 1} entries for {s} masks, got {seg_host.numel()}")
    sp.require_gpu(anchors, masks, feats)
    lengths = (seg_host[1:] - seg_host[:-1]).tolist()
    i64 = dict(dtype=torch.long, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    if n == 0:
        zeros = [0] * (s + 1)
        return {"unique_coords": torch.zeros((0, 2), **i64), "unique_offsets": zeros, "anchor_to_unique": torch.zeros(0, **i64),
                "pos_pairs": torch.zeros((0, 2), **i64), "neg_pairs": torch.zeros((0, 2), **i64), "pos_offsets": zeros, "neg_offsets": zeros,
                "pos_weights": torch.zeros(0, **f32), "neg_weights": torch.zeros(0, **f32), "pos_dist": torch.zeros(0, **f32),
                "neg_dist": torch.zeros(0, **f32), "stats": {"n_anchors": lengths, "n_pos": zeros[1:], "n_neg": zeros[1:], "n_unique": zeros[1:]}}
    seg = seg_host.to(dev)
    offs = torch.tensor(sp.neighbor_offsets(k, max_radius), dtype=torch.int32).to(dev)
    k_act = offs.shape[0]
    lo, hi = sp.distance_thresholds(min_distance, max_distance, h, w)
    a32 = sp.anchors_int32(anchors)
    meta = torch.zeros(3 * s + 2, dtype=torch.int32, device=dev)          # positives [S] | negatives [S] | unique offsets [S + 1] | flags
    bits = ops.spatial_pack_mask(masks)
    pos_rc, pos_valid = ops.spatial_knn(bits, w, a32, seg, seg_host, offs, meta, 0, 3 * s + 1)
    neg_rc, neg_count = ops.spatial_negatives(bits, w, a32, seg, seg_host, lo, hi, sp.draws_int32(draws, n, n_per, dev, generator), meta, s,
                                              3 * s + 1)
    out = ops.spatial_pair_index(h, w, a32, seg, seg_host, pos_rc, pos_valid, neg_rc, neg_count, feats.contiguous(), tau, min_w, meta, 2 * s)
    m = meta.cpu().tolist()                                               # the one host read: sizes the outputs, carries the flags
    sp.raise_flag(m[-1])
    n_pos, n_neg, useg = m[:s], m[s:2 * s], m[2 * s:3 * s + 1]
    anchor_idx = out["anchor_idx"].long()
    e = torch.nonzero_static(pos_valid.reshape(-1), size=sum(n_pos)).reshape(-1)     # ascending: by anchor, then by offset rank
    pos_pairs = torch.stack([anchor_idx[torch.div(e, k_act, rounding_mode="floor")], out["pos_idx"].reshape(-1)[e].long()], dim=1)
    live = torch.arange(n_per, device=dev).unsqueeze(0) < neg_count.unsqueeze(1)
    f = torch.nonzero_static(live.reshape(-1), size=sum(n_neg)).reshape(-1)          # by anchor, then in draw order
    neg_pairs = torch.stack([anchor_idx[torch.div(f, n_per, rounding_mode="floor")], out["neg_idx"].reshape(-1)[f].long()], dim=1)

    def ends(counts):
        acc = [0]
        for c in counts:
            acc.append(acc[-1] + c)
        return acc

    return {"unique_coords": out["unique_rc"][:useg[-1]].long(), "unique_offsets": useg, "anchor_to_unique": anchor_idx,
            "pos_pairs": pos_pairs, "neg_pairs": neg_pairs, "pos_offsets": ends(n_pos), "neg_offsets": ends(n_neg),
            "pos_weights": out["pos_w"].reshape(-1)[e], "neg_weights": out["neg_w"].reshape(-1)[f], "pos_dist": out["pos_d"].reshape(-1)[e],
            "neg_dist": out["neg_d"].reshape(-1)[f],
            "stats": {"n_anchors": lengths, "n_pos": n_pos, "n_neg": n_neg, "n_unique": [b - a for a, b in zip(useg[:-1], useg[1:])]}}


def build_spatial_pairs(anchors: torch.Tensor, mask: torch.Tensor, feat: torch.Tensor, *, k: int = 4, max_radius: int = 8,
                        min_distance: float = 16.0, max_distance: float | None = None, n_per_anchor: int = 4, tau: float = 1.0,
                        min_w: float = 0.05, generator=None, draws=None) -> dict:
    """One sample: anchors [N, 2] int64 / int32 (row, col), mask [H, W] bool, feat [C, H, W] float32 (the spectral map the weights are
    taken from, C <= 256), all on the GPU; H, W <= 1024, at most 64 neighbours and 1 <= n_per_anchor <= 64 negatives per anchor.  -> dict:
    unique_coords [U, 2] int64 (what torch.unique(dim=0) gives for anchors, neighbours and negatives), anchor_to_unique [N],
    pos_pairs [P, 2] / neg_pairs [Q, 2] int64 (anchor, other) indexing unique_coords, pairs anchor-major and in offset / draw order,
    pos_weights / neg_weights / pos_dist / neg_dist float32, unique_offsets / pos_offsets / neg_offsets ([0, U], [0, P], [0, Q]) and
    stats (n_anchors, n_pos, n_neg, n_unique as integers).  draws [N, n_per_anchor] in [0, 2^31) fix the negatives (None: torch.randint
    with `generator`).  One host read per call (five integers); an anchor outside the mask or a draw out of range raises ValueError there.
    Argument errors are raised before anything is launched."""
    if mask.dim() != 2 or feat.dim() != 3:
        raise ValueError(f"expected mask [H, W] and feat [C, H, W], got {tuple(mask.shape)} and {tuple(feat.shape)}")
    out = _mine(anchors, mask.unsqueeze(0), feat.unsqueeze(0), [0, anchors.shape[0]] if anchors.dim() == 2 else [0, 0], k, max_radius,
                min_distance, max_distance, n_per_anchor, tau, min_w, generator, draws)
    out["stats"] = {key: value[0] for key, value in out["stats"].items()}
    return out


def build_spatial_pairs_batched(anchors_all: torch.Tensor, masks: torch.Tensor, feats: torch.Tensor, offsets, *, k: int = 4,
                                max_radius: int = 8, min_distance: float = 16.0, max_distance: float | None = None, n_per_anchor: int = 4,
                                tau: float = 1.0, min_w: float = 0.05, generator=None, draws=None) -> dict:
    """Every sample of a batch in the same launches: anchors_all [N, 2] concatenated over the samples, masks [S, H, W] bool, feats
    [S, C, H, W] float32, offsets [S + 1] rising from 0 to N (a list or a CPU tensor costs no synchronisation; segments may be empty).
    The dict of build_spatial_pairs with every tensor concatenated over the segments: unique_coords [U, 2] with unique_offsets [S + 1],
    pos_pairs / neg_pairs (and anchor_to_unique) shifted by the segment's unique offset so that they index the pooled unique_coords,
    pos_offsets / neg_offsets [S + 1], stats with one integer per segment.  One host read per call (3 S + 2 integers)."""
    return _mine(anchors_all, masks, feats, offsets, k, max_radius, min_distance, max_distance, n_per_anchor, tau, min_w, generator, draws)
