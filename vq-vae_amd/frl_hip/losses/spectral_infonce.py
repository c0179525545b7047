"""The global spectral InfoNCE with cross-batch kNN of the reference's step (frl/training/representation/step.py:707-812) on the HIP path.

The anchors of every patch of a batch are pooled; positives are mutual k-nearest neighbours in spectral space over the pool
(`pairs_mutual_knn_chunked`), negatives are random cross-patch pairs weighted by 1 - exp(-d / tau) of their spectral distance d, and
`contrastive_loss` runs on the pooled embeddings.  `global_spectral_infonce` is the whole block; its parts are public too:

  cross_patch_negatives   step.py:743-773.  The reference loops over the ordered patch pairs (pi, pj), pi != pj, with two torch.randint
                          calls per pair; here the pairs, their distances and their weights come from one launch (csrc/spectral_negatives.hip),
                          as a function of `draws [Q, 2]`: negative q belongs to block b = q // n_per of that loop order (pi = b // (S - 1),
                          r = b % (S - 1), pj = r + (r >= pi)) and picks anchor offsets[p] + ((draw * count_p) >> 31) of either patch.
  pair_similarity         the -|a - b|^2 / D per pair of step.py:573-574 and :801-802.
  pair_similarity_stats   the kernel-sizing diagnostic of step.py:798-807, one host read for both lists.
  spectral_neg_tau_sweep  the epoch-0 diagnostic of step.py:774-783 (stock torch ops: it runs once per run).

Deviations from the reference: torch.randint's stream is not reproduced -- the sampling law is the same (each anchor of a patch with
probability 1 / count to within count / 2^31) and the picks are a documented function of `draws`.  With one patch the reference fails in
torch.cat([]); here the negatives are empty and the loss is what `contrastive_loss` gives without negatives.  Positives on exactly tied
distances rank by (distance, index), the deviation of `pairs_mutual_knn_chunked`.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from .. import _lib, ops
from .contrastive import contrastive_loss
from .pairs import pairs_mutual_knn_chunked

MAX_CHANNELS = ops.SPECTRAL_NEG_MAX_WIDTH
_OFFSETS = {}                                                             # (device, offsets) -> int32 tensor on the device; a few entries


def _offsets_list(offsets, n: int) -> list:
    if isinstance(offsets, torch.Tensor):
        if offsets.is_cuda:
            raise ValueError("offsets must be a host list or a CPU tensor (reading them back would synchronise)")
        offsets = offsets.reshape(-1).tolist()
    offs = [int(o) for o in offsets]
    if not offs or offs[0] != 0 or offs[-1] != n:
        raise ValueError(f"offsets must start at 0 and end at the number of anchors ({n}), got {offs[:1]} .. {offs[-1:]}")
    if any(b < a for a, b in zip(offs[:-1], offs[1:])):
        raise ValueError("offsets must not decrease")
    return offs


def _offsets_on(device, offs: list) -> torch.Tensor:
    key = (str(device), tuple(offs))
    t = _OFFSETS.get(key)
    if t is None:
        if len(_OFFSETS) >= 16:
            _OFFSETS.clear()
        t = _OFFSETS[key] = torch.tensor(offs, dtype=torch.int32).to(device)
    return t


def negatives_per_patch_pair(neg_per_anchor: int, n: int, n_patches: int) -> int:
    """n_per of step.py:751-755: max(1, neg_per_anchor * N // (S (S - 1))), 0 when there is no ordered patch pair."""
    pairs = n_patches * (n_patches - 1)
    return max(1, (int(neg_per_anchor) * n) // pairs) if pairs > 0 else 0


def cross_patch_negatives(spec_all: torch.Tensor, offsets, neg_per_anchor: int = 20, tau: float = 1.0, min_w: float = 0.05, generator=None,
                          draws: Optional[torch.Tensor] = None) -> dict:
    """spec_all [N, C] (C <= 256) on the GPU, offsets [S + 1] patch bounds (a list or a CPU tensor) -> dict: neg_pairs [Q, 2] int64 (i in
    patch pi, j in patch pj != pi), neg_weights [Q] = clamp(1 - exp(-neg_dist / tau), min_w, 1), neg_dist [Q] = |spec[i] - spec[j]|, all
    on the GPU, and n_per = max(1, neg_per_anchor * N // (S (S - 1))) with Q = n_per * S * (S - 1) (one patch: Q = 0).  draws [Q, 2] int64
    / int32 in [0, 2^31) fix the picks (None: torch.randint on the device with `generator`).  An empty patch, offsets that do not run
    from 0 to N without decreasing, and draws of the wrong shape or dtype raise ValueError, as do CPU draws out of range; draws on the
    device that are out of range are clamped and flagged for ops.index_errors().  One launch, no host read: with the same offsets as an
    earlier call (their device copy is kept) the call can be captured in a graph."""
    if spec_all.dim() != 2:
        raise ValueError(f"spec_all must be [N, C], got {tuple(spec_all.shape)}")
    n, c = spec_all.shape
    if not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"1 to {MAX_CHANNELS} spectral channels, got {c}")
    if not float(tau) > 0.0:
        raise ValueError(f"tau must be positive, got {tau}")
    if int(neg_per_anchor) < 0:
        raise ValueError(f"neg_per_anchor must not be negative, got {neg_per_anchor}")
    offs = _offsets_list(offsets, n)
    s = len(offs) - 1
    if any(b == a for a, b in zip(offs[:-1], offs[1:])):
        raise ValueError("every patch needs at least one anchor (torch.randint(low, low) of the reference raises too)")
    n_per = negatives_per_patch_pair(neg_per_anchor, n, s)
    q = n_per * s * (s - 1)
    if q >= 2 ** 31:
        raise ValueError(f"{q} negatives: at most 2^31 - 1")
    if draws is not None:
        if draws.dtype not in (torch.int64, torch.int32) or tuple(draws.shape) != (q, 2):
            raise ValueError(f"draws must be an int64 or int32 [{q}, 2] tensor, got {tuple(draws.shape)} {draws.dtype}")
        if not draws.is_cuda and q and (int(draws.min()) < 0 or int(draws.max()) >= 2 ** 31):
            raise ValueError("draws must lie in [0, 2^31)")
    if not spec_all.is_cuda:
        raise _lib.FrlHipError("cross_patch_negatives: spec_all must live on the GPU (no CPU fallback)")
    dev = spec_all.device
    if q == 0:
        return {"neg_pairs": torch.zeros((0, 2), dtype=torch.long, device=dev), "neg_weights": torch.zeros(0, device=dev),
                "neg_dist": torch.zeros(0, device=dev), "n_per": n_per}
    if draws is None:
        draws = torch.randint(0, 2 ** 31, (q, 2), device=dev, generator=generator)
    draws = draws.to(dev)
    if draws.dtype == torch.int64:                                        # beyond int32: -1, which the kernel clamps and flags
        draws = torch.where((draws >= 0) & (draws < 2 ** 31), draws, torch.full_like(draws, -1))
    pairs, dist, weights = ops.spectral_negatives(spec_all.detach().float().contiguous(), _offsets_on(dev, offs), s, n_per,
                                                  draws.to(torch.int32).contiguous(), float(tau), float(min_w))
    return {"neg_pairs": pairs, "neg_weights": weights, "neg_dist": dist, "n_per": n_per}


def _rows_and_pairs(z: torch.Tensor, pairs: torch.Tensor):
    if z.dim() != 2 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"expected z [N, D] and pairs [P, 2], got {tuple(z.shape)} and {tuple(pairs.shape)}")
    if z.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"z must be float32 or bfloat16, got {z.dtype}")
    if not z.is_cuda:
        raise _lib.FrlHipError("pair_similarity: z must live on the GPU (no CPU fallback)")
    return z.detach().float().contiguous(), pairs.to(z.device, torch.int64).contiguous()


def pair_similarity(z: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
    """z [N, D] float32 | bfloat16 (D <= 256; bfloat16 is converted, as contrastive_loss does), pairs [P, 2] -> sims [P] float32 =
    -|z[a] - z[b]|^2 / D, the unit the l2 InfoNCE feeds its softmax (step.py:573-574, :801-802).  Not differentiable."""
    rows, pairs = _rows_and_pairs(z, pairs)
    return ops.pair_sims(rows, pairs)


def pair_similarity_stats(z: torch.Tensor, pos_pairs: torch.Tensor, neg_pairs: torch.Tensor, temperature: float) -> Optional[dict]:
    """The kernel-sizing diagnostic of step.py:798-807: {pos_mean, pos_std, neg_mean, neg_std, temperature} of the pair similarities
    (std unbiased, NaN for a single pair, as torch.std), None when either list is empty.  Sums in double in a fixed order; one host read
    for both lists."""
    if pos_pairs.shape[0] == 0 or neg_pairs.shape[0] == 0:
        return None
    rows, pos = _rows_and_pairs(z, pos_pairs)
    _, neg = _rows_and_pairs(z, neg_pairs)
    stats = torch.empty((2, 4), dtype=torch.float64, device=rows.device)
    ops.pair_sims(rows, pos, stats[0])
    ops.pair_sims(rows, neg, stats[1])
    (_, pm, ps, _), (_, nm, ns, _) = stats.cpu().tolist()                 # the one host read
    return {"pos_mean": pm, "pos_std": ps, "neg_mean": nm, "neg_std": ns, "temperature": float(temperature)}


def spectral_neg_tau_sweep(neg_dist: torch.Tensor, min_w: float = 0.05, taus: Sequence[float] = (0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0)) -> dict:
    """The epoch-0 diagnostic of step.py:774-783: tau -> {neg_mean, neg_q25, neg_q50} of clamp(1 - exp(-neg_dist / tau), min_w, 1).  Stock
    torch ops on the tensor's own device and one host read; {} for no negatives."""
    taus = [float(t) for t in taus]
    if neg_dist.numel() == 0 or not taus:
        return {}
    d = neg_dist.detach().reshape(1, -1).float()
    t = torch.tensor(taus, dtype=torch.float32).to(d.device).reshape(-1, 1)
    w = (1.0 - torch.exp(-d / t)).clamp(min=min_w, max=1.0)
    qs = torch.quantile(w, torch.tensor([0.25, 0.50], dtype=torch.float32).to(d.device), dim=1)
    rows = torch.stack([w.mean(dim=1), qs[0], qs[1]], dim=1).cpu().tolist()
    return {tau: {"neg_mean": r[0], "neg_q25": r[1], "neg_q50": r[2]} for tau, r in zip(taus, rows)}


def global_spectral_infonce(z_all: torch.Tensor, spec_all: torch.Tensor, coord_list: Sequence[torch.Tensor], offsets, *, positive_k: int = 16,
                            positive_min_spatial: float = 4.0, neg_per_anchor: int = 20, neg_tau: float = 1.0, neg_min_weight: float = 0.05,
                            temperature: float = 0.07, generator=None, draws: Optional[torch.Tensor] = None, stats: bool = True):
    """step.py:721-809 in one call.  z_all [N, D] (the pooled, projected anchor embeddings; receives the gradient), spec_all [N, C] (data:
    no gradient), coord_list: the [n_p, 2] anchor coordinates of every patch, offsets [S + 1] (a list or a CPU tensor) -> (loss, info).
    loss is 0-dim: contrastive_loss(z_all, pos, neg, neg_weights=..., similarity="l2") over the mutual-kNN positives and the cross-patch
    negatives.  info: pos_pairs, neg_pairs, neg_weights, neg_dist, n_pos, n_neg and sim_stats (pair_similarity_stats; None when `stats`
    is false or a list is empty).  One patch: no negatives.  No patch: a zero loss, nothing launched."""
    dev = z_all.device
    if len(coord_list) == 0 or z_all.shape[0] == 0:
        empty = torch.zeros((0, 2), dtype=torch.long, device=dev)
        return z_all.new_zeros(()), {"pos_pairs": empty, "neg_pairs": empty, "neg_weights": z_all.new_zeros(0, dtype=torch.float32),
                                     "neg_dist": z_all.new_zeros(0, dtype=torch.float32), "n_pos": 0, "n_neg": 0, "sim_stats": None}
    if z_all.dim() != 2 or spec_all.dim() != 2 or spec_all.shape[0] != z_all.shape[0]:
        raise ValueError(f"expected z_all [N, D] and spec_all [N, C], got {tuple(z_all.shape)} and {tuple(spec_all.shape)}")
    offs = _offsets_list(offsets, z_all.shape[0])
    if len(offs) != len(coord_list) + 1:
        raise ValueError(f"offsets must have {len(coord_list) + 1} entries for {len(coord_list)} patches, got {len(offs)}")
    spec = spec_all.detach()
    neg = cross_patch_negatives(spec, offs, neg_per_anchor, neg_tau, neg_min_weight, generator, draws)   # validates before any launch
    pos = pairs_mutual_knn_chunked(spec, coord_list, offs, k=int(positive_k), pos_min_spatial=float(positive_min_spatial))
    loss = contrastive_loss(z_all, pos, neg["neg_pairs"], neg_weights=neg["neg_weights"], temperature=temperature, similarity="l2")
    sim_stats = pair_similarity_stats(z_all, pos, neg["neg_pairs"], temperature) if stats else None
    return loss.reshape(()), {"pos_pairs": pos, "neg_pairs": neg["neg_pairs"], "neg_weights": neg["neg_weights"], "neg_dist": neg["neg_dist"],
                              "n_pos": pos.shape[0], "n_neg": neg["neg_pairs"].shape[0], "sim_stats": sim_stats}
