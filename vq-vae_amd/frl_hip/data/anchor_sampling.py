"""Anchor sampling on the GPU: the reference's frl/data/sampling/anchor_sampling.py on the kernels of csrc/anchors.hip.

Anchors are the pixels a contrastive step builds its pairs around: a regular grid whose origin is jittered during training, kept where
the mask is valid, plus a supplement of `supplement_n` valid pixels drawn without replacement, uniformly or in proportion to a weight map.
The reference draws them per sample with a dozen small torch ops and two host reads; `sample_anchors_batched` draws them for every sample
of a batch with three launches (pack the masks, grid, supplement) and ONE host read of 3 S + 1 integers (grid points, supplement picks and
valid pixels per sample, the error flags).  Its `anchors` / `offsets` are what `losses.build_spatial_pairs_batched` takes.  The
reference's surface sits on top of it: `sample_anchors_grid`, `sample_anchors_grid_plus_supplement`, `resolve_supplement_weights`,
`AnchorSampler` (with `.batched`) and `build_anchor_sampler`; `inverse_frequency_weights` is its `_apply_inverse_frequency` for a batch.

The supplement is an exponential race.  Every pixel gets an Exp(1) variate (`noise`); the key of an eligible pixel is noise / weight
(noise alone without weights) and the picks are the `supplement_n` eligible pixels of smallest (key, row * W + col), in ascending order.
The minimum of independent exponentials with rates w_i falls on pixel i with probability w_i / sum(w), and by memorylessness the rest
of the race is the same race without the winner: the picks are a sequential draw without replacement proportional to the weights, the
law of `torch.multinomial(replacement=False)`; with equal weights a uniformly random ordered subset, `randperm[:n]`.

Deviations from the reference:
  * torch's `randperm` / `multinomial` / `randint` streams are not reproduced: the result is a documented function of `jitter` and `noise`.
  * With weights of which some are positive the supplement has m = min(supplement_n, pixels of positive weight) picks.  The reference asks
    `multinomial` for min(supplement_n, valid pixels); asked for more than there are positive entries, torch's CPU multinomial hands out
    zero-weight pixels without a word (observed with the torch this package is tested with).
  * A non-finite weight at a valid pixel raises ValueError.  In the reference a NaN turns `total > 0` false and the draw silently uniform.
    So does a negative or NaN `noise` at a valid pixel (the default noise never is).
  * `border - jitter_radius < 0`, `stride < 1` and `border > 1024` are refused.  With a negative grid origin the reference indexes the mask
    with negative rows, which wrap around.
  * A grid whose first row or column already lies at or beyond H - border or W - border has no point and the result is the supplement
    alone; the reference's `torch.arange` raises when the start lies beyond the end (border 16 on a 24 x 20 mask).
  * `inverse_frequency_weights`: a value that rounds beyond int32 is in no whitelist; more than 4096 distinct values in a sample raise.
Limits: at most 4096 samples of at most 1024 x 1024, supplement_n <= 1024, at most 16384 grid points per sample.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .. import _lib, ops

MAX_SAMPLES, MAX_HW, MAX_SUPPLEMENT, MAX_GRID, MAX_VALUES = 4096, 1024, 1024, 16384, 4096
FLAG_JITTER, FLAG_WEIGHT, FLAG_NOISE, FLAG_DISTINCT = 1, 2, 4, 8


@dataclass
class WeightSpec:
    """One source of supplement weights: `channel` is 'group.channel' in the sample dict; without `transform` it is a plain mask that
    multiplies in, with 'inverse-frequency' it is a discrete channel weighted by 1 / count; `valid_values`: only pixels whose rounded
    value is in this set take part."""
    channel: str
    transform: Optional[str] = None
    valid_values: Optional[set] = None


def _steps(start: int, end: int, stride: int) -> int:
    return (end - start + stride - 1) // stride if start < end else 0


def grid_capacity(h: int, w: int, stride: int, border: int, jitter_radius: int) -> int:
    """The most grid points any jitter in [-jitter_radius, jitter_radius]^2 gives on an h x w mask (the origin at border - jitter_radius)."""
    return _steps(border - jitter_radius, h - border, stride) * _steps(border - jitter_radius, w - border, stride)


def _require_gpu(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.FrlHipError("anchor sampling: tensors must live on the GPU (no CPU fallback)")


def _check(masks, stride, border, jitter_radius, supplement_n, weights, jitter, noise):
    if not isinstance(masks, torch.Tensor) or masks.dim() != 3 or masks.dtype != torch.bool or 0 in masks.shape:
        raise ValueError(f"masks must be a bool [S, H, W] tensor, got {tuple(masks.shape)} {masks.dtype}" if isinstance(masks, torch.Tensor)
                         else "masks must be a bool [S, H, W] tensor")
    s, h, w = masks.shape
    if s > MAX_SAMPLES:
        raise ValueError(f"at most {MAX_SAMPLES} samples per call, got {s}")
    if max(h, w) > MAX_HW:
        raise ValueError(f"mask height and width must not exceed {MAX_HW}, got {(h, w)}")
    if int(stride) < 1:
        raise ValueError(f"stride must be at least 1, got {stride}")
    if int(jitter_radius) < 0:
        raise ValueError(f"jitter_radius must not be negative, got {jitter_radius}")
    if int(border) - int(jitter_radius) < 0:
        raise ValueError(f"border - jitter_radius must not be negative (the grid origin would leave the mask), got {border} - {jitter_radius}")
    if int(border) > MAX_HW:
        raise ValueError(f"border must not exceed {MAX_HW}, got {border}")
    if not 0 <= int(supplement_n) <= MAX_SUPPLEMENT:
        raise ValueError(f"supplement_n must be in 0..{MAX_SUPPLEMENT}, got {supplement_n}")
    cap = grid_capacity(h, w, int(stride), int(border), int(jitter_radius))
    if cap > MAX_GRID:
        raise ValueError(f"at most {MAX_GRID} grid points per sample, stride {stride} and border {border} give {cap} on {h} x {w}")
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (s, h, w) or weights.dtype == torch.bool
                                or weights.is_complex()):
        raise ValueError(f"weights must be a real [{s}, {h}, {w}] tensor")
    if jitter is not None:
        if not isinstance(jitter, torch.Tensor) or tuple(jitter.shape) != (s, 2) or jitter.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"jitter must be an int64 or int32 [{s}, 2] tensor of (row, col) shifts")
        if not jitter.is_cuda and jitter.numel() and int(jitter.abs().max()) > int(jitter_radius):
            raise ValueError(f"jitter must lie in [-{jitter_radius}, {jitter_radius}]")
    if noise is not None and (not isinstance(noise, torch.Tensor) or tuple(noise.shape) != (s, h, w) or noise.dtype != torch.float32):
        raise ValueError(f"noise must be a float32 [{s}, {h}, {w}] tensor")
    return cap


def _raise_flag(flag: int, jitter_radius) -> None:
    if flag & FLAG_JITTER:
        raise ValueError(f"jitter must lie in [-{jitter_radius}, {jitter_radius}]")
    if flag & FLAG_WEIGHT:
        raise ValueError("a weight at a valid pixel is not finite")
    if flag & FLAG_NOISE:
        raise ValueError("noise at a valid pixel is negative or NaN")
    if flag & FLAG_DISTINCT:
        raise ValueError(f"more than {MAX_VALUES} distinct values in a sample")


def sample_anchors_batched(masks: torch.Tensor, *, stride: int = 16, border: int = 16, jitter_radius: int = 0, supplement_n: int = 104,
                           weights: Optional[torch.Tensor] = None, jitter: Optional[torch.Tensor] = None,
                           noise: Optional[torch.Tensor] = None, generator=None) -> dict:
    """masks [S, H, W] bool on the GPU -> dict: `anchors` [N, 2] int64 (row, col), per sample the grid anchors in row-major order and then
    the supplement in key order (not deduplicated, as the reference concatenates them); `offsets`, a list of S + 1 ints (sample s owns
    anchors[offsets[s]:offsets[s + 1]]); `stats` with n_grid, n_supplement, n_valid, one integer per sample.

    weights [S, H, W] (any real dtype; only values at valid pixels matter), jitter [S, 2] integers in [-jitter_radius, jitter_radius]
    (None: torch.randint on the device with `generator`, zeros when jitter_radius == 0), noise [S, H, W] float32 >= 0 (None:
    exponential_ with `generator`).  supplement_n = 0 gives the grid only.  One host read; a non-finite weight, a bad noise or a jitter
    out of range raises ValueError there, argument errors before anything is launched."""
    cap = _check(masks, stride, border, jitter_radius, supplement_n, weights, jitter, noise)
    _require_gpu(masks, weights, noise)
    s, h, w = masks.shape
    dev, n_sup, radius = masks.device, int(supplement_n), int(jitter_radius)
    if jitter is None:
        jitter = torch.randint(-radius, radius + 1, (s, 2), device=dev, generator=generator) if radius > 0 else \
            torch.zeros((s, 2), dtype=torch.int32, device=dev)
    jitter = jitter.to(dev)
    if jitter.dtype == torch.int64:
        jitter = jitter.clamp(-(1 << 20), 1 << 20)                          # still out of range for the kernel, which flags it
    jitter = jitter.to(torch.int32).contiguous()
    if noise is None and n_sup > 0:
        noise = torch.empty((s, h, w), dtype=torch.float32, device=dev).exponential_(generator=generator)
    if weights is not None:
        weights = weights.to(dev, torch.float32).contiguous()
    meta = torch.zeros(3 * s + 1, dtype=torch.int32, device=dev)           # grid points [S] | picks [S] | valid pixels [S] | flags
    bits = ops.spatial_pack_mask(masks)
    grid_rc = ops.anchor_grid(bits, w, stride, border, radius, jitter, cap, meta, 0, 3 * s)
    sup_rc = ops.anchor_supplement(bits, w, weights, None if noise is None else noise.contiguous(), n_sup, meta, s, 2 * s, 3 * s)
    m = meta.cpu().tolist()                                                # the one host read: sizes the output, carries the flags
    _raise_flag(m[-1], radius)
    n_grid, n_pick, n_valid = m[:s], m[s:2 * s], m[2 * s:3 * s]
    offsets = [0]
    for g, p in zip(n_grid, n_pick):
        offsets.append(offsets[-1] + g + p)
    counts = meta[:2 * s].reshape(2, s)
    live = torch.cat([torch.arange(cap, device=dev).unsqueeze(0) < counts[0].unsqueeze(1),
                      torch.arange(n_sup, device=dev).unsqueeze(0) < counts[1].unsqueeze(1)], dim=1)
    e = torch.nonzero_static(live.reshape(-1), size=offsets[-1]).reshape(-1)      # ascending: by sample, grid before supplement
    anchors = torch.cat([grid_rc, sup_rc], dim=1).reshape(-1, 2)[e].long()
    return {"anchors": anchors, "offsets": offsets, "stats": {"n_grid": n_grid, "n_supplement": n_pick, "n_valid": n_valid}}


def _single(mask, weights, jitter, noise):
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2:
        raise ValueError("mask must be a bool [H, W] tensor")
    if weights is not None and isinstance(weights, torch.Tensor) and weights.dim() == 2:
        weights = weights.unsqueeze(0)
    if jitter is not None and isinstance(jitter, torch.Tensor) and jitter.dim() == 1:
        jitter = jitter.unsqueeze(0)
    if noise is not None and isinstance(noise, torch.Tensor) and noise.dim() == 2:
        noise = noise.unsqueeze(0)
    return mask.unsqueeze(0), weights, jitter, noise


def sample_anchors_grid(mask: torch.Tensor, stride: int = 16, border: int = 16, jitter_radius: int = 0, *, jitter=None,
                        generator=None) -> torch.Tensor:
    """mask [H, W] bool -> [N, 2] int64: the grid points (border + jr + i stride, border + jc + j stride) with row < H - border and
    col < W - border on valid pixels, row-major.  jitter [2] (or [1, 2]) fixes (jr, jc)."""
    masks, _, jitter, _ = _single(mask, None, jitter, None)
    return sample_anchors_batched(masks, stride=stride, border=border, jitter_radius=jitter_radius, supplement_n=0, jitter=jitter,
                                  generator=generator)["anchors"]


def sample_anchors_grid_plus_supplement(mask: torch.Tensor, stride: int = 16, border: int = 16, jitter_radius: int = 0,
                                        supplement_n: int = 104, weights: Optional[torch.Tensor] = None, *, jitter=None, noise=None,
                                        generator=None) -> torch.Tensor:
    """mask [H, W] bool, weights [H, W] or None -> [N, 2] int64: the grid anchors, then the supplement."""
    masks, weights, jitter, noise = _single(mask, weights, jitter, noise)
    return sample_anchors_batched(masks, stride=stride, border=border, jitter_radius=jitter_radius, supplement_n=supplement_n,
                                  weights=weights, jitter=jitter, noise=noise, generator=generator)["anchors"]


def inverse_frequency_weights(data: torch.Tensor, valid_mask: torch.Tensor, valid_values=None) -> torch.Tensor:
    """data [S, H, W] or [H, W] float32, valid_mask bool of the same shape, both on the GPU -> float32 weights of that shape: 1 / count
    at a pixel that is valid, finite and (with `valid_values`, an iterable of integers) whose value rounded half to even is listed, count
    being the number of such pixels of the sample with an equal value; 0 elsewhere.  A sample without such a pixel gets 1 at its valid
    pixels.  One host read (the flag): more than 4096 distinct values in a sample raise ValueError."""
    if not isinstance(data, torch.Tensor) or data.dim() not in (2, 3) or data.dtype != torch.float32 or 0 in data.shape:
        raise ValueError("data must be a float32 [S, H, W] or [H, W] tensor")
    if not isinstance(valid_mask, torch.Tensor) or valid_mask.shape != data.shape or valid_mask.dtype != torch.bool:
        raise ValueError(f"valid_mask must be a bool tensor of shape {tuple(data.shape)}")
    if max(data.shape[-2:]) > MAX_HW or (data.dim() == 3 and data.shape[0] > MAX_SAMPLES):
        raise ValueError(f"at most {MAX_SAMPLES} samples of at most {MAX_HW} x {MAX_HW}, got {tuple(data.shape)}")
    listed = None
    if valid_values is not None:
        listed = sorted({int(v) for v in valid_values})
        if len(listed) > MAX_VALUES or any(not -2 ** 31 <= v < 2 ** 31 for v in listed):
            raise ValueError(f"valid_values must be at most {MAX_VALUES} int32 values")
    _require_gpu(data, valid_mask)
    d3 = data.reshape((-1,) + tuple(data.shape[-2:])).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=data.device)
    if listed is not None:
        listed = torch.tensor(listed, dtype=torch.int32).to(data.device)
    out = ops.anchor_inverse_frequency(d3, ops.spatial_pack_mask(valid_mask.reshape(d3.shape)), listed, flag)
    _raise_flag(int(flag.item()), 0)
    return out.reshape(data.shape)


def _channel(sample: Dict[str, Any], ref: str) -> torch.Tensor:
    """'group.channel' -> that channel of sample[group] as a float32 [H, W] tensor ([T, H, W] data: its first slice)."""
    pieces = ref.split(".")
    if len(pieces) != 2:
        raise ValueError(f"a weight channel is named 'group.channel', got '{ref}'")
    group, name = pieces
    names = list(sample["metadata"]["channel_names"][group])
    if name not in names:
        raise ValueError(f"group '{group}' has no channel '{name}' (it has {names})")
    plane = sample[group][names.index(name)]
    if isinstance(plane, np.ndarray):
        plane = torch.from_numpy(np.ascontiguousarray(plane))
    if plane.dim() == 3:
        plane = plane[0]
    return plane.float()


def resolve_supplement_weights(sample: Dict[str, Any], weight_specs: List[WeightSpec], device=None) -> Optional[torch.Tensor]:
    """The [H, W] float32 weight map of a sample, in the reference's order: the plain masks (specs without a transform) are multiplied
    together; each transform is then evaluated on the pixels where that product is positive (on the finite pixels when there is no plain
    mask) and multiplied in.  numpy planes are accepted.  Everything is moved to `device` when given; a transform runs on the GPU, so its
    operands are uploaded to the current device when they are not there yet.  An unknown transform raises ValueError before any work."""
    for spec in weight_specs:
        if spec.transform not in (None, "inverse-frequency"):
            raise ValueError(f"unknown weight transform '{spec.transform}'")
    product = None
    for spec in weight_specs:
        if spec.transform is None:
            plane = _channel(sample, spec.channel)
            plane = plane if device is None else plane.to(device)
            product = plane if product is None else product * plane.to(product.device)
    for spec in weight_specs:
        if spec.transform is None:
            continue
        plane = _channel(sample, spec.channel)
        target = device if device is not None else (product.device if product is not None and product.is_cuda else None)
        plane = plane.to(target) if target is not None else (plane if plane.is_cuda else plane.cuda())
        if product is not None:
            product = product.to(plane.device)
        valid = product > 0 if product is not None else torch.isfinite(plane)
        w = inverse_frequency_weights(plane.contiguous(), valid, spec.valid_values)
        product = w if product is None else product * w
    return product


def _known(strategy: str) -> bool:
    return strategy == "grid" or strategy.startswith("grid-plus-supplement")


class AnchorSampler:
    """The reference's configured sampler: `sampler(mask, training=True, sample=None)` -> [N, 2] anchors of one mask, and
    `sampler.batched(masks, ...)` -> the dict of `sample_anchors_batched` for a batch.  strategy 'grid' or 'grid-plus-supplement*'; the
    jitter applies only when training.  With `weight_specs` and a sample dict the supplement is weighted by `resolve_supplement_weights`."""

    def __init__(self, strategy: str, stride: int = 16, border: int = 16, jitter_radius: int = 4, supplement_n: int = 104,
                 weight_specs: Optional[List[WeightSpec]] = None):
        self.strategy = strategy
        self.stride = stride
        self.border = border
        self.jitter_radius = jitter_radius
        self.supplement_n = supplement_n
        self.weight_specs = list(weight_specs) if weight_specs else []

    def _plan(self, training: bool) -> dict:
        if not _known(self.strategy):
            raise ValueError(f"unknown sampling strategy '{self.strategy}'")
        return dict(stride=self.stride, border=self.border, jitter_radius=self.jitter_radius if training else 0,
                    supplement_n=0 if self.strategy == "grid" else self.supplement_n)

    def __call__(self, mask: torch.Tensor, training: bool = True, sample: Optional[Dict[str, Any]] = None, *, jitter=None, noise=None,
                 generator=None) -> torch.Tensor:
        plan = self._plan(training)
        weights = None
        if plan["supplement_n"] and self.weight_specs and sample is not None:
            weights = resolve_supplement_weights(sample, self.weight_specs, device=mask.device)
        masks, weights, jitter, noise = _single(mask, weights, jitter, noise)
        return sample_anchors_batched(masks, weights=weights, jitter=jitter, noise=noise, generator=generator, **plan)["anchors"]

    def batched(self, masks: torch.Tensor, training: bool = True, samples: Optional[List[Dict[str, Any]]] = None,
                weights: Optional[torch.Tensor] = None, *, jitter=None, noise=None, generator=None) -> dict:
        """masks [S, H, W]; weights [S, H, W] given, or resolved per sample from `samples` (a list of S sample dicts) when the sampler has
        weight specs."""
        plan = self._plan(training)
        if weights is None and plan["supplement_n"] and self.weight_specs and samples is not None:
            if len(samples) != masks.shape[0]:
                raise ValueError(f"{masks.shape[0]} masks but {len(samples)} samples")
            weights = torch.stack([resolve_supplement_weights(smp, self.weight_specs, device=masks.device) for smp in samples])
        if plan["supplement_n"] == 0:
            weights = None
        return sample_anchors_batched(masks, weights=weights, jitter=jitter, noise=noise, generator=generator, **plan)


def _get(obj, name, default=None):
    """obj.name or obj[name], whichever obj offers; `default` when it is absent or None."""
    if obj is None:
        return default
    value = obj.get(name) if isinstance(obj, dict) else getattr(obj, name, None)
    return default if value is None else value


def _specs_from_entries(entries) -> List[WeightSpec]:
    """weight_by entries: a 'group.channel' string, a dict or an object with mask_ref, or with channel (and transform)."""
    specs = []
    for entry in entries or []:
        if isinstance(entry, str):
            specs.append(WeightSpec(channel=entry))
            continue
        if not isinstance(entry, dict) and not hasattr(entry, "channel") and not hasattr(entry, "mask_ref"):
            raise ValueError(f"a weight_by entry is a string, a dict or a config object, got {type(entry)}")
        mask_ref = _get(entry, "mask_ref")
        if mask_ref:
            specs.append(WeightSpec(channel=mask_ref))
            continue
        channel = _get(entry, "channel")
        if not channel:
            if isinstance(entry, dict):
                raise ValueError(f"a weight_by dict needs a 'channel', got {entry}")
            continue
        specs.append(WeightSpec(channel=channel, transform=_get(entry, "transform")))
    return specs


def build_anchor_sampler(bindings_config, strategy_name: str) -> AnchorSampler:
    """An AnchorSampler from a bindings configuration, duck-typed on its two shapes: `sampling_strategies[name]` with `.grid` (stride,
    exclude_border, jitter.radius) and `.supplement` (n, weight_by entries carrying mask_ref or channel / transform), or the legacy
    `sampling_strategy` dict of dicts ('grid' -> {stride, exclude_border, jitter: {radius}}, name -> {grid, supplement: {n, sampling:
    {weight_by}}}).  Missing values default to stride 16, border 16, jitter radius 4, 104 supplement points; without either table those
    defaults are used."""
    parsed = _get(bindings_config, "sampling_strategies")
    entry = parsed.get(strategy_name) if parsed else None
    if entry is not None:
        grid, supplement = _get(entry, "grid"), _get(entry, "supplement")
        common = dict(stride=_get(grid, "stride", 16), border=_get(grid, "exclude_border", 16),
                      jitter_radius=_get(_get(grid, "jitter"), "radius", 4))
        if strategy_name == "grid":
            return AnchorSampler("grid", supplement_n=0, **common)
        return AnchorSampler(strategy_name, supplement_n=_get(supplement, "n", 104),
                             weight_specs=_specs_from_entries(_get(supplement, "weight_by")), **common)
    legacy = _get(bindings_config, "sampling_strategy")
    if legacy:
        if strategy_name == "grid":
            grid, supplement = legacy.get("grid", {}), {}
        elif strategy_name.startswith("grid-plus-supplement"):
            block = legacy.get(strategy_name, {})
            grid, supplement = block.get("grid", {}), block.get("supplement", {})
        else:
            raise ValueError(f"unknown sampling strategy '{strategy_name}'")
        common = dict(stride=grid.get("stride", 16), border=grid.get("exclude_border", 16),
                      jitter_radius=grid.get("jitter", {}).get("radius", 4))
        if strategy_name == "grid":
            return AnchorSampler("grid", supplement_n=0, **common)
        return AnchorSampler(strategy_name, supplement_n=supplement.get("n", 104),
                             weight_specs=_specs_from_entries(supplement.get("sampling", {}).get("weight_by", [])), **common)
    return AnchorSampler(strategy_name)
