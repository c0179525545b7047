"""The phase margin losses of the reference's cross-batch phase block on the HIP path (csrc/phase_margin.hip; caller
frl/training/representation/step.py:969-1006): `phase_recovery_discrimination_loss` (frl/losses/triplet_phase.py:352-426) and
`compute_phase_spread_ranking` (frl/losses/phase_neighborhood.py:637-740) with the reference's signatures and semantics, plus the gathered
form of the spread ranking, which runs on the rows `phase_alignment` produces and never holds a distance block in memory.

Recovery discrimination, per pixel of z_phase [N, T, D] with ysfc [N, T] (NaN / negative = invalid):

    low[t] = valid and ysfc <= low_ysfc_max,  high[t] = valid and ysfc >= high_ysfc_min,  pairs = {(tl, th): low[tl] and high[th]}
    d = sqrt(max(|z_tl - z_th|^2, 1e-12)),    loss = sum over all pixels and pairs of softplus(margin - d) / n_pairs   (0 without pairs)

Spread ranking, per valid pair b = (i, j) with the self-distance blocks of the two pixels at the ysfc values they share:

    n_b = max(1, unmasked off-diagonal entries),  spread_i = sum mask d_i / n_b,  spread_j likewise,  r_b = dynamism_ref[i] - dynamism_ref[j]
    term_b = softplus(spread_j - spread_i + margin) [r_b > delta] + softplus(spread_i - spread_j + margin) [r_b < -delta]
    loss = sum_b term_b / B_valid    (the mean runs over all valid pairs, constrained or not)

Losses are 0-dim float32 whatever the dtype of the embeddings, gradients have the dtype of the input they belong to, and both are
bit-reproducible.  A zero distance has zero gradient.  `stats=False` returns an empty dict and makes no host read (same loss bits);
`stats=True` costs one device-to-host copy.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops
from .soft_neighborhood import _fold_gradient_rows, _zero, phase_alignment


def _gup(g: torch.Tensor) -> torch.Tensor:
    return g.reshape(1).float().contiguous()


class _RecoveryFn(Function):
    @staticmethod
    def forward(ctx, z, ysfc, margin, low_ysfc_max, high_ysfc_min):
        out2, stats = ops.recovery_disc_fwd(z, ysfc, margin, low_ysfc_max, high_ysfc_min)
        ctx.save_for_backward(z, ysfc, out2)
        ctx.hp = (margin, low_ysfc_max, high_ysfc_min)
        ctx.mark_non_differentiable(stats)
        return out2[0], stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        z, ysfc, out2 = ctx.saved_tensors
        return ops.recovery_disc_bwd(z, ysfc, *ctx.hp, out2, _gup(g)), None, None, None, None


class _SpreadMatrixFn(Function):
    @staticmethod
    def forward(ctx, d_i, d_j, mask, ref_diff, margin, delta):
        out2, stats, pairstat = ops.spread_rank_fwd(d_i, d_j, mask, ref_diff, margin, delta)
        ctx.save_for_backward(mask, pairstat, ref_diff)
        ctx.hp = (margin, delta)
        ctx.mark_non_differentiable(stats)
        return out2[0], stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        mask, pairstat, ref_diff = ctx.saved_tensors
        gi, gj = ops.spread_rank_bwd(mask, pairstat, ref_diff, *ctx.hp, _gup(g))
        return gi if ctx.needs_input_grad[0] else None, gj if ctx.needs_input_grad[1] else None, None, None, None, None


class _SpreadGatheredFn(Function):
    @staticmethod
    def forward(ctx, emb, rows, lengths, ref_diff, margin, delta):
        out2, stats, pairstat, rows = ops.spread_rank_gathered_fwd(emb, rows, lengths, ref_diff, margin, delta)
        ctx.save_for_backward(emb, rows, lengths, ref_diff, pairstat)
        ctx.hp = (margin, delta)
        ctx.mark_non_differentiable(stats)
        return out2[0], stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        emb, rows, lengths, ref_diff, pairstat = ctx.saved_tensors
        grows = ops.spread_rank_gathered_bwd(emb, rows, lengths, ref_diff, *ctx.hp, pairstat, _gup(g), checked=True)
        return _fold_gradient_rows(grows, rows, lengths, emb), None, None, None, None, None


def _embeddings(x: torch.Tensor) -> torch.Tensor:
    return (x if x.dtype in (torch.float32, torch.bfloat16) else x.float()).contiguous()


def phase_recovery_discrimination_loss(z_phase: torch.Tensor, ysfc: torch.Tensor, margin: float = 0.5, low_ysfc_max: float = 1.0,
                                       high_ysfc_min: float = 5.0, *, stats: bool = True) -> tuple[torch.Tensor, dict]:
    """z_phase [N, T, D] float32 | bfloat16, ysfc [N, T] floating (NaN = invalid) -> (loss, {"n_pairs", "n_active_pixels"}); the gradient
    flows to z_phase, in its dtype.  T <= 32, D <= 256."""
    if z_phase.dim() != 3 or ysfc.dim() != 2 or tuple(ysfc.shape) != tuple(z_phase.shape[:2]):
        raise ValueError(f"expected z_phase [N, T, D] and ysfc [N, T], got {tuple(z_phase.shape)} and {tuple(ysfc.shape)}")
    n, t, d = z_phase.shape
    if t > ops.PHASE_MARGIN_MAX_T or d > ops.PHASE_MARGIN_MAX_WIDTH:
        raise ValueError(f"supports T <= {ops.PHASE_MARGIN_MAX_T} and D <= {ops.PHASE_MARGIN_MAX_WIDTH}, got T = {t}, D = {d}")
    if n == 0 or t == 0 or d == 0:
        return _zero(z_phase.device), ({"n_pairs": 0, "n_active_pixels": 0} if stats else {})
    loss, vec = _RecoveryFn.apply(_embeddings(z_phase), ysfc.detach().to(z_phase.device, torch.float32).contiguous(), float(margin),
                                  float(low_ysfc_max), float(high_ysfc_min))
    if not stats:
        return loss, {}
    host = vec.cpu().tolist()
    return loss, {"n_pairs": int(host[1]), "n_active_pixels": int(host[2])}


_EMPTY_SPREAD_STATS = {"n_pairs": 0, "n_constrained_i": 0, "n_constrained_j": 0, "frac_satisfied": 1.0, "mean_spread_i": 0.0,
                       "mean_spread_j": 0.0, "mean_ref_diff": 0.0}


def _spread_stats(vec, b: int) -> dict:
    """vec: the eight doubles of the reduction kernel, already on the host."""
    n_ci, n_cj = int(vec[1]), int(vec[2])
    return {"n_pairs": b, "n_constrained_i": n_ci, "n_constrained_j": n_cj,
            "frac_satisfied": float(vec[3]) / (n_ci + n_cj) if n_ci + n_cj > 0 else 1.0, "mean_spread_i": float(vec[4]) / b,
            "mean_spread_j": float(vec[5]) / b, "mean_ref_diff": float(vec[6]) / b}


def _finish_spread(loss, vec, b: int, stats: bool):
    if not stats:
        return loss, {}
    return loss, (dict(_EMPTY_SPREAD_STATS) if vec is None else _spread_stats(vec.cpu().tolist(), b))


def compute_phase_spread_ranking(batch_result: dict, idx_i_valid: torch.Tensor, idx_j_valid: torch.Tensor, dynamism_ref: torch.Tensor,
                                 margin: float = 0.1, delta: float = 0.5, *, stats: bool = True) -> tuple[torch.Tensor, dict]:
    """The matrix form on a dict in the layout of the reference's build_phase_neighborhood_batch: d_learned_self, d_learned_self_j and
    mask_self [B_valid, M, M] (any M); idx_*_valid [B_valid] index dynamism_ref [N].  The gradient flows to both distance tensors."""
    d_i, d_j, mask = batch_result["d_learned_self"], batch_result["d_learned_self_j"], batch_result["mask_self"]
    if d_i.dim() != 3 or d_i.shape[1] != d_i.shape[2] or d_j.shape != d_i.shape or mask.shape != d_i.shape:
        raise ValueError(f"expected d_learned_self, d_learned_self_j and mask_self of one shape [B, M, M], got {tuple(d_i.shape)}, "
                         f"{tuple(d_j.shape)}, {tuple(mask.shape)}")
    b, m, _ = d_i.shape
    if tuple(idx_i_valid.shape) != (b,) or tuple(idx_j_valid.shape) != (b,) or dynamism_ref.dim() != 1:
        raise ValueError(f"expected idx_i_valid and idx_j_valid of shape [{b}] and dynamism_ref [N], got {tuple(idx_i_valid.shape)}, "
                         f"{tuple(idx_j_valid.shape)}, {tuple(dynamism_ref.shape)}")
    dev = d_i.device
    if b == 0 or m == 0:
        return _finish_spread(_zero(dev), None, 0, stats)
    dyn = dynamism_ref.detach().to(dev, torch.float32)
    ref_diff = (dyn[idx_i_valid.to(dev)] - dyn[idx_j_valid.to(dev)]).contiguous()
    loss, vec = _SpreadMatrixFn.apply(d_i.float().contiguous(), d_j.float().contiguous(), mask.to(torch.bool).contiguous(), ref_diff,
                                      float(margin), float(delta))
    return _finish_spread(loss, vec, b, stats)


def phase_spread_ranking_gathered(emb: torch.Tensor, rows_i: torch.Tensor, rows_j: torch.Tensor, lengths: torch.Tensor,
                                  ref_diff: torch.Tensor, margin: float = 0.1, delta: float = 0.5, *,
                                  stats: bool = True) -> tuple[torch.Tensor, dict]:
    """The same loss with d_i[b, t, t'] = |emb[rows_i[b, t]] - emb[rows_i[b, t']]|_2, d_j likewise from rows_j, and the mask t, t' <
    lengths[b], t != t'.  emb [R, D] float32 | bfloat16, rows_* [B, M] int64, lengths [B], ref_diff [B] = r_b; M <= 32, D <= 256.  The
    gradient flows to emb, in its dtype."""
    if emb.dim() != 2:
        raise ValueError(f"expected emb [R, D], got {tuple(emb.shape)}")
    if rows_i.dim() != 2 or rows_j.shape != rows_i.shape:
        raise ValueError(f"rows_i and rows_j must share one shape [B, M], got {tuple(rows_i.shape)} and {tuple(rows_j.shape)}")
    b, m = rows_i.shape
    if tuple(lengths.shape) != (b,) or tuple(ref_diff.shape) != (b,):
        raise ValueError(f"lengths and ref_diff must have shape [{b}], got {tuple(lengths.shape)} and {tuple(ref_diff.shape)}")
    if m > ops.PHASE_MARGIN_MAX_T or emb.shape[1] > ops.PHASE_MARGIN_MAX_WIDTH:
        raise ValueError(f"the gathered form supports M <= {ops.PHASE_MARGIN_MAX_T} positions per pair and D <= "
                         f"{ops.PHASE_MARGIN_MAX_WIDTH}, got M = {m}, D = {emb.shape[1]}")
    dev = emb.device
    if b == 0 or m == 0:
        return _finish_spread(_zero(dev), None, 0, stats)
    rows = torch.stack([rows_i.to(dev, torch.int64), rows_j.to(dev, torch.int64)])
    loss, vec = _SpreadGatheredFn.apply(_embeddings(emb), rows, lengths.to(dev, torch.int64).contiguous(),
                                        ref_diff.detach().to(dev, torch.float32).contiguous(), float(margin), float(delta))
    return _finish_spread(loss, vec, b, stats)


def phase_spread_ranking_loss(phase_embeddings: torch.Tensor, ysfc: torch.Tensor, pair_indices: torch.Tensor, dynamism_ref: torch.Tensor,
                              min_overlap: int = 3, margin: float = 0.1, delta: float = 0.5, *, alignment: Optional[tuple] = None,
                              stats: bool = True) -> tuple[torch.Tensor, dict]:
    """phase_embeddings [N, T, D], ysfc [N, T], pair_indices [B, 2], dynamism_ref [N] -> (loss, stats): the spread ranking over the pairs
    with at least min_overlap shared ysfc values, at the timesteps phase_alignment picks.  `alignment` takes the 4-tuple of a
    phase_alignment call already made (a trainer that also calls phase_neighborhood_loss aligns once)."""
    if phase_embeddings.dim() != 3 or tuple(ysfc.shape) != tuple(phase_embeddings.shape[:2]):
        raise ValueError(f"expected phase_embeddings [N, T, D] and ysfc [N, T], got {tuple(phase_embeddings.shape)} and {tuple(ysfc.shape)}")
    n, t, d = phase_embeddings.shape
    if tuple(dynamism_ref.shape) != (n,):
        raise ValueError(f"dynamism_ref must have shape [{n}], got {tuple(dynamism_ref.shape)}")
    if d > ops.PHASE_MARGIN_MAX_WIDTH:
        raise ValueError(f"supports D <= {ops.PHASE_MARGIN_MAX_WIDTH}, got D = {d}")
    dev = phase_embeddings.device
    valid, rows_i, rows_j, lengths = phase_alignment(ysfc, pair_indices, min_overlap) if alignment is None else alignment
    if int(lengths.numel()) == 0:
        return _finish_spread(_zero(dev), None, 0, stats)
    pairs = pair_indices.to(dev, torch.int64).reshape(-1, 2)[valid.to(dev)]
    dyn = dynamism_ref.detach().to(dev, torch.float32)
    return phase_spread_ranking_gathered(phase_embeddings.reshape(n * t, d), rows_i, rows_j, lengths, dyn[pairs[:, 0]] - dyn[pairs[:, 1]],
                                         margin, delta, stats=stats)
