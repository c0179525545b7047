"""Sparse-location gathers and spatial pair mining of the live trainer (frl/utils/spatial.py:132-332) on the HIP path.

`extract_at_locations(feature [C, H, W], coords [N, 2]) -> [N, C]` and `extract_temporal_at_locations(feature [C, T, H, W], coords)
-> [N, T, C]` keep the reference's signatures (callers: frl/training/representation/step.py:526,562,602).  The kernel takes element
strides, so the reference's channels-first view of one of this library's NHWC tensors (`z[b].permute(2, 0, 1)`) is gathered in place,
row by row -- which is the coalesced direction for NHWC.  Backward: rows of the incoming gradient that address the same pixel are
summed in list order over a key-sorted list (`frl_segment_sum_rows`): bit-reproducible, no float atomics.

`spatial_knn_pairs` and `spatial_negative_pairs` keep the reference's signatures and return values (frl/utils/spatial.py:176-332; callers:
step.py:325-338) on the kernels of csrc/spatial_pairs.hip: the mask packed to one bit per pixel, neighbours by a fixed offset list,
negatives drawn uniformly without replacement from the valid pixels whose distance lies in [min_distance, max_distance].  The distance
test is the reference's float32 one, restated on the host as two integer bounds on the squared distance.  Deviation: the reference draws
with `torch.randperm`, whose stream is not reproduced; the sampling law (uniform without replacement over the same candidate set) is the
same, and the picks are a documented function of `draws` (include/frl_hip.h, frl_spatial_negatives).  Offsets at one distance are ordered
by (dr, dc); the reference's `argsort` leaves that order unspecified.  `losses.build_spatial_pairs` does the whole block of step.py:325-401.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _lib, ops

MAX_K = MAX_RADIUS = MAX_PER_ANCHOR = 64


class _GatherFn(Function):
    @staticmethod
    def forward(ctx, feature, coords):
        c, h, w = feature.shape
        ctx.shape = (c, h, w)
        ctx.save_for_backward(coords)
        ctx.strides, ctx.dtype = feature.stride(), feature.dtype
        return ops.gather_locations(feature, coords)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (coords,) = ctx.saved_tensors
        c, h, w = ctx.shape
        r = torch.where(coords[:, 0] < 0, coords[:, 0] + h, coords[:, 0])
        q = torch.where(coords[:, 1] < 0, coords[:, 1] + w, coords[:, 1])
        keys, order = torch.sort(r * w + q, stable=True)
        rows = torch.zeros(h * w, c, dtype=torch.float32, device=g.device)              # NHWC rows of the gradient raster
        ops.segment_sum_rows(g.float().contiguous(), order, keys, rows)
        return rows.reshape(h, w, c).permute(2, 0, 1).to(ctx.dtype), None              # a [C, H, W] view, like the input


def extract_at_locations(feature: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """feature [C, H, W] (any strides), coords [N, 2] as (row, col) -> [N, C]."""
    if feature.dim() != 3 or coords.dim() != 2 or coords.shape[1] != 2:
        raise ValueError("extract_at_locations: feature must be [C, H, W] and coords [N, 2]")
    coords = coords.to(device=feature.device, dtype=torch.int64)
    _, h, w = feature.shape
    coords = torch.stack([ops.sanitize_indices(coords[:, 0], h, "extract_at_locations: row"),
                          ops.sanitize_indices(coords[:, 1], w, "extract_at_locations: col")], dim=1).contiguous()
    if feature.requires_grad:
        return _GatherFn.apply(feature, coords)
    return ops.gather_locations(feature, coords)


def extract_temporal_at_locations(feature: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """feature [C, T, H, W], coords [N, 2] -> [N, T, C] (one gather per time step; T <= 15 in this model)."""
    if feature.dim() != 4:
        raise ValueError("extract_temporal_at_locations: feature must be [C, T, H, W]")
    return torch.stack([extract_at_locations(feature[:, t], coords) for t in range(feature.shape[1])], dim=1)


# ---- spatial pair mining: host logic shared with losses/spatial_pairs.py -------------------------------------------------------------

def neighbor_offsets(k: int, max_radius: int) -> list:
    """The first min(k, count) of the (dr, dc) in [-R, R]^2 with 0 < dr^2 + dc^2 <= R^2, ordered by (dr^2 + dc^2, (dr + R) (2R + 1) + dc + R)."""
    r = int(max_radius)
    offs = [(dr * dr + dc * dc, (dr + r) * (2 * r + 1) + dc + r, dr, dc) for dr in range(-r, r + 1) for dc in range(-r, r + 1)
            if 0 < dr * dr + dc * dc <= r * r]
    return [(dr, dc) for _, _, dr, dc in sorted(offs)[:int(k)]]


def distance_thresholds(min_distance: float, max_distance, h: int, w: int) -> tuple:
    """-> (lo, hi): lo <= d2 <= hi for an integer squared distance d2 on an h x w grid iff float32 sqrt(float32(d2)) >= float32(min_distance)
    and <= float32(max_distance) (None: no upper bound), the reference's float32 predicate (its squared distances are exact integers below
    2^24).  lo is the smallest such integer >= 0, hi the largest <= (h - 1)^2 + (w - 1)^2; lo > hi when no distance qualifies."""
    top = (h - 1) ** 2 + (w - 1) ** 2
    with np.errstate(over="ignore"):
        dmin = np.float32(min_distance)
        dmax = None if max_distance is None else np.float32(max_distance)
    a, b = 0, top + 1                                                    # float32 sqrt is monotone: bisect
    while a < b:
        mid = (a + b) // 2
        if np.sqrt(np.float32(mid)) >= dmin:
            b = mid
        else:
            a = mid + 1
    lo = a
    if dmax is None:
        return lo, top
    a, b = -1, top
    while a < b:
        mid = (a + b + 1) // 2
        if np.sqrt(np.float32(mid)) <= dmax:
            a = mid
        else:
            b = mid - 1
    return lo, a


def check_knn_args(k, max_radius) -> None:
    if int(k) < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if not 1 <= int(max_radius) <= MAX_RADIUS:
        raise ValueError(f"max_radius must be in 1..{MAX_RADIUS}, got {max_radius}")
    if min(int(k), len(neighbor_offsets(MAX_K + 1, max_radius))) > MAX_K:
        raise ValueError(f"at most {MAX_K} neighbours per anchor (k = {k} at max_radius = {max_radius})")


def check_negative_args(min_distance, max_distance, n_per_anchor) -> None:
    if int(n_per_anchor) < 1 or int(n_per_anchor) > MAX_PER_ANCHOR:
        raise ValueError(f"n_per_anchor must be in 1..{MAX_PER_ANCHOR}, got {n_per_anchor}")
    if not float(min_distance) >= 0.0:
        raise ValueError(f"min_distance must not be negative, got {min_distance}")
    if max_distance is not None and not float(max_distance) >= float(min_distance):
        raise ValueError(f"max_distance must not be below min_distance, got {max_distance} < {min_distance}")


def check_anchors_and_masks(anchor_coords: torch.Tensor, masks: torch.Tensor, mask_dims: int) -> None:
    if anchor_coords.dim() != 2 or anchor_coords.shape[1] != 2 or anchor_coords.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"anchors must be an int64 or int32 [N, 2] tensor of (row, col), got {tuple(anchor_coords.shape)} {anchor_coords.dtype}")
    shape = "[H, W]" if mask_dims == 2 else "[S, H, W]"
    if masks.dim() != mask_dims or masks.dtype != torch.bool or 0 in masks.shape:
        raise ValueError(f"the mask must be a bool {shape} tensor, got {tuple(masks.shape)} {masks.dtype}")
    limit = _lib.load().frl_spatial_pairs_max_hw()
    if max(masks.shape[-2:]) > limit:
        raise ValueError(f"mask height and width must not exceed {limit}, got {tuple(masks.shape[-2:])}")


def check_draws(draws, n: int, n_per_anchor: int) -> None:
    if draws is None:
        return
    if draws.dtype not in (torch.int64, torch.int32) or tuple(draws.shape) != (n, int(n_per_anchor)):
        raise ValueError(f"draws must be an int64 or int32 [{n}, {int(n_per_anchor)}] tensor, got {tuple(draws.shape)} {draws.dtype}")
    if not draws.is_cuda and draws.numel() and (int(draws.min()) < 0 or int(draws.max()) >= 2 ** 31):
        raise ValueError("draws must lie in [0, 2^31)")


def require_gpu(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.FrlHipError("spatial pairs: tensors must live on the GPU (no CPU fallback)")


def anchors_int32(anchor_coords: torch.Tensor) -> torch.Tensor:
    """int64 coordinates beyond int32 stay outside every grid (the kernels flag them)."""
    if anchor_coords.dtype == torch.int64:
        anchor_coords = anchor_coords.clamp(-1, 1 << 20)
    return anchor_coords.to(torch.int32).contiguous()


def draws_int32(draws, n: int, n_per_anchor: int, device, generator) -> torch.Tensor:
    """None: torch.randint(0, 2^31, (n, n_per_anchor)).  A value outside [0, 2^31) becomes -1, which the kernel flags."""
    if draws is None:
        draws = torch.randint(0, 2 ** 31, (n, int(n_per_anchor)), device=device, generator=generator)
    draws = draws.to(device)
    if draws.dtype == torch.int64:
        draws = torch.where((draws >= 0) & (draws < 2 ** 31), draws, torch.full_like(draws, -1))
    return draws.to(torch.int32).contiguous()


def raise_flag(flag: int) -> None:
    if flag & 1:
        raise ValueError("an anchor lies outside the mask (row in [0, H) and col in [0, W) are required)")
    if flag & 2:
        raise ValueError("draws must lie in [0, 2^31)")


def _empty_pairs(device):
    return torch.zeros(0, dtype=torch.long, device=device), torch.zeros((0, 2), dtype=torch.long, device=device)


def _one_segment(n: int, device):
    seg_host = torch.tensor([0, n], dtype=torch.int32)
    return seg_host, seg_host.to(device)


def spatial_knn_pairs(anchor_coords: torch.Tensor, mask: torch.Tensor, k: int = 4, max_radius: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """anchor_coords [N, 2] int64 / int32 (row, col), mask [H, W] bool, both on the GPU -> (anchor_indices [M] int64 into anchor_coords,
    neighbor_coords [M, 2] int64): per anchor the first min(k, count) offsets of `neighbor_offsets` whose pixel is inside the mask and
    valid, anchor-major and in offset order.  k >= 1, the neighbour count at most 64, 1 <= max_radius <= 64.  One host read (the number of
    valid slots and the out-of-range flag); an anchor outside the mask raises ValueError."""
    check_knn_args(k, max_radius)
    check_anchors_and_masks(anchor_coords, mask, 2)
    require_gpu(anchor_coords, mask)
    n, dev = anchor_coords.shape[0], anchor_coords.device
    if n == 0:
        return _empty_pairs(dev)
    offs = torch.tensor(neighbor_offsets(k, max_radius), dtype=torch.int32).to(dev)
    seg_host, seg = _one_segment(n, dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)
    pos_rc, pos_valid = ops.spatial_knn(ops.spatial_pack_mask(mask.unsqueeze(0)), mask.shape[1], anchors_int32(anchor_coords), seg, seg_host,
                                        offs, meta, 0, 1)
    count, flag = meta.cpu().tolist()                                    # the one host read
    raise_flag(flag)
    e = torch.nonzero_static(pos_valid.reshape(-1), size=count).reshape(-1)
    return torch.div(e, offs.shape[0], rounding_mode="floor"), pos_rc.reshape(-1, 2)[e].long()


def spatial_negative_pairs(anchor_coords: torch.Tensor, mask: torch.Tensor, min_distance: float = 16.0, max_distance: float | None = None,
                           n_per_anchor: int = 4, *, generator=None, draws=None) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (anchor_indices [M] int64, neighbor_coords [M, 2] int64): per anchor min(n_per_anchor, cnt) of its cnt candidates (valid pixels
    at a float32 distance in [min_distance, max_distance]), uniformly without replacement, anchor-major and in draw order; anchors without
    a candidate contribute nothing.  draws [N, n_per_anchor] int64 / int32 in [0, 2^31) fix the picks (None: torch.randint with
    `generator`).  1 <= n_per_anchor <= 64.  One host read (the number of negatives and the flags); an anchor outside the mask or a draw
    out of range raises ValueError."""
    check_negative_args(min_distance, max_distance, n_per_anchor)
    check_anchors_and_masks(anchor_coords, mask, 2)
    n, dev = anchor_coords.shape[0], anchor_coords.device
    check_draws(draws, n, n_per_anchor)
    require_gpu(anchor_coords, mask)
    if n == 0:
        return _empty_pairs(dev)
    h, w = mask.shape
    lo, hi = distance_thresholds(min_distance, max_distance, h, w)
    seg_host, seg = _one_segment(n, dev)
    meta = torch.zeros(2, dtype=torch.int32, device=dev)
    neg_rc, neg_count = ops.spatial_negatives(ops.spatial_pack_mask(mask.unsqueeze(0)), w, anchors_int32(anchor_coords), seg, seg_host, lo, hi,
                                              draws_int32(draws, n, n_per_anchor, dev, generator), meta, 0, 1)
    count, flag = meta.cpu().tolist()                                    # the one host read
    raise_flag(flag)
    live = torch.arange(int(n_per_anchor), device=dev).unsqueeze(0) < neg_count.unsqueeze(1)
    e = torch.nonzero_static(live.reshape(-1), size=count).reshape(-1)
    return torch.div(e, int(n_per_anchor), rounding_mode="floor"), neg_rc.reshape(-1, 2)[e].long()
