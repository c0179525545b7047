"""Soft-neighbourhood matching (phase KL) loss on the HIP path: `soft_neighborhood_matching_loss` and `phase_neighborhood_loss` with the
reference's signatures and semantics (frl/losses/soft_neighborhood.py:46-208, frl/losses/phase_neighborhood.py:458-630; caller
frl/training/representation/step.py:948), plus the gathered form the phase loss runs on and the index plumbing that feeds it.

Per pair b and row t, over the unmasked entries t' of that row only:

    lp = log_softmax(-d_ref / tau_ref),  lq = log_softmax(-d_learned / tau_learned),  p = exp(lp),  q = exp(lq)
    kl[b,t] = sum_t' p (lp - lq)             rows with fewer than min_valid_per_row unmasked entries are skipped
    L_b     = sum_t kl[b,t] / rows_b         rows_b = contributing rows; a pair with none is inactive
    loss    = sum_b w_b L_b / sum_b w_b      over the active pairs; 0 when there is none or the weights sum to 0

(the reference fills masked logits with -1e9, where p = q = 0 exactly: skipping them is the same function).  The matrix form reads the
[B, M, M] blocks from memory; the gathered form builds them on chip from rows of two matrices, d[t, t'] = |a_t - b_t'|_2, so no distance
matrix is written, and its backward folds per-position gradient rows into d(emb) with the sorted-segment sum InfoNCE uses.  A zero
distance has zero gradient (torch.cdist's convention: the diagonal of an (i, i) self-pair).  Loss and gradients are bit-reproducible,
float32 whatever the dtype of `emb`; the gradient has the dtype of `d_learned` / `emb`.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops

class _MatrixFn(Function):
    @staticmethod
    def forward(ctx, d_learned, d_reference, mask, weights, tau_ref, tau_learned, min_valid):
        out2, stats, pairstat, coef = ops.soft_nbr_fwd(d_reference, d_learned, mask, weights, tau_ref, tau_learned, min_valid,
                                                       want_coef=ctx.needs_input_grad[0])
        ctx.save_for_backward(coef, pairstat, weights, out2)
        ctx.mark_non_differentiable(stats)
        return out2[0], stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        coef, pairstat, weights, out2 = ctx.saved_tensors
        return ops.soft_nbr_bwd(coef, pairstat, weights, out2, g.reshape(1).float().contiguous()), None, None, None, None, None, None


class _GatheredFn(Function):
    @staticmethod
    def forward(ctx, emb, ref, rows, lengths, exclude_diagonal, weights, tau_ref, tau_learned, min_valid):
        out2, stats, pairstat, rows = ops.soft_nbr_gathered_fwd(ref, emb, rows, lengths, exclude_diagonal, weights, tau_ref, tau_learned, min_valid)
        ctx.save_for_backward(emb, ref, rows, lengths, weights, pairstat, out2)
        ctx.hp = (exclude_diagonal, tau_ref, tau_learned, min_valid)
        ctx.mark_non_differentiable(stats)
        return out2[0], stats

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        emb, ref, rows, lengths, weights, pairstat, out2 = ctx.saved_tensors
        exclude_diagonal, tau_ref, tau_learned, min_valid = ctx.hp
        grows = ops.soft_nbr_gathered_bwd(ref, emb, rows, lengths, exclude_diagonal, weights, tau_ref, tau_learned, min_valid, pairstat, out2,
                                          g.reshape(1).float().contiguous(), checked=True)
        return _fold_gradient_rows(grows, rows[2:], lengths, emb), None, None, None, None, None, None, None, None


def _fold_gradient_rows(grows, keys, lengths, emb):
    """grows [2, B, M, D] float32 gradient rows of the positions keys [2, B, M] (rows of emb) -> d emb in emb's dtype."""
    # role a's rows ahead of role b's, each in pair order, grouped by embedding row (stable sort: index plumbing) and summed in that order.
    # Positions beyond lengths carry zero rows and whatever index the caller padded with (phase_alignment: 0); keyed by that they would
    # form one long run that a single thread walks, so they are dealt round the embedding rows instead (adding zeros, no host read).
    inside = torch.arange(keys.shape[2], device=keys.device) < lengths.unsqueeze(1)
    dealt = torch.arange(keys.numel(), device=keys.device).reshape(keys.shape) % emb.shape[0]
    keys, order = torch.sort(torch.where(inside, keys, dealt).reshape(-1), stable=True)
    de = torch.zeros(emb.shape, dtype=torch.float32, device=emb.device)
    ops.segment_sum_rows(grows.reshape(-1, emb.shape[1]), order, keys, de)
    return de.to(emb.dtype)


def _weights(pair_weights: Optional[torch.Tensor], b: int, device) -> Optional[torch.Tensor]:
    if pair_weights is None:
        return None
    if pair_weights.shape != (b,):
        raise ValueError(f"pair_weights must have shape [{b}], got {tuple(pair_weights.shape)}")
    return pair_weights.detach().to(device, torch.float32).contiguous()


def _zero(device) -> torch.Tensor:
    return torch.zeros((), dtype=torch.float32, device=device, requires_grad=True)


def _stats_dict(vec, n_pairs: int, m: int) -> dict:
    """vec: the eight doubles of the reduction kernel, already on the host."""
    _, _, active, rows, overlap, ent_p, ent_q, _ = (float(v) for v in vec)
    loss = float(vec[0])
    per_row = (lambda s: s / rows) if rows > 0 else (lambda s: 0.0)
    return {"n_pairs": n_pairs, "n_pairs_active": int(active), "n_rows_total": n_pairs * m, "n_rows_valid": int(rows), "mean_kl": loss,
            "mean_overlap": per_row(overlap), "mean_entropy_p": per_row(ent_p), "mean_entropy_q": per_row(ent_q)}


def _empty_stats(n_pairs: int, m: int) -> dict:
    return _stats_dict([0.0] * 8, n_pairs, m)


def _matrix_term(d_reference, d_learned, mask, tau_ref, tau_learned, pair_weights, min_valid_per_row):
    """-> (loss 0-dim float32, stats f64 [8] on the device or None when nothing was launched, B, M)"""
    if int(min_valid_per_row) < 2:
        raise ValueError(f"min_valid_per_row must be >= 2, got {min_valid_per_row}")
    if d_reference.dim() != 3 or d_reference.shape[1] != d_reference.shape[2] or d_learned.shape != d_reference.shape or mask.shape != d_reference.shape:
        raise ValueError(f"expected d_reference, d_learned and mask of one shape [B, M, M], got {tuple(d_reference.shape)}, "
                         f"{tuple(d_learned.shape)}, {tuple(mask.shape)}")
    b, m, _ = d_reference.shape
    w = _weights(pair_weights, b, d_learned.device)
    if b == 0 or m == 0:
        return _zero(d_learned.device), None, b, m
    dl = d_learned if d_learned.dtype == torch.float32 else d_learned.float()
    loss, stats = _MatrixFn.apply(dl.contiguous(), d_reference.detach().float().contiguous(), mask.to(torch.bool).contiguous(), w,
                                  float(tau_ref), float(tau_learned), int(min_valid_per_row))
    return loss, stats, b, m


def soft_neighborhood_matching_loss(d_reference: torch.Tensor, d_learned: torch.Tensor, mask: torch.Tensor, tau_ref: float = 1.0,
                                    tau_learned: float = 1.0, pair_weights: Optional[torch.Tensor] = None, min_valid_per_row: int = 2,
                                    *, stats: bool = True) -> tuple[torch.Tensor, dict]:
    """d_reference, d_learned [B, M, M], mask [B, M, M] bool -> (loss, stats); the gradient flows to d_learned.  stats=False returns an
    empty dict and makes no host synchronisation (the loss bits are the same)."""
    loss, vec, b, m = _matrix_term(d_reference, d_learned, mask, tau_ref, tau_learned, pair_weights, min_valid_per_row)
    if not stats:
        return loss, {}
    return loss, (_empty_stats(b, m) if vec is None else _stats_dict(vec.cpu().tolist(), b, m))


def _gathered_term(ref, emb, ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b, lengths, exclude_diagonal, tau_ref, tau_learned, pair_weights,
                   min_valid_per_row):
    if int(min_valid_per_row) < 2:
        raise ValueError(f"min_valid_per_row must be >= 2, got {min_valid_per_row}")
    if ref_rows_a.dim() != 2 or any(r.shape != ref_rows_a.shape for r in (ref_rows_b, emb_rows_a, emb_rows_b)):
        raise ValueError("the four row-index arrays must share one shape [B, M]")
    b, m = ref_rows_a.shape
    if lengths.shape != (b,):
        raise ValueError(f"lengths must have shape [{b}], got {tuple(lengths.shape)}")
    if m > ops.SOFT_NBR_MAX_M:
        raise ValueError(f"the gathered form supports M <= {ops.SOFT_NBR_MAX_M} positions per pair, got M = {m}")
    dev = emb.device
    w = _weights(pair_weights, b, dev)
    rows = torch.stack([r.to(dev, torch.int64) for r in (ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b)])
    if b == 0 or m == 0:
        return _zero(dev), None, b, m
    e = emb if emb.dtype in (torch.float32, torch.bfloat16) else emb.float()
    loss, stats = _GatheredFn.apply(e.contiguous(), ref.detach().float().contiguous(), rows, lengths.to(dev, torch.int64).contiguous(),
                                    bool(exclude_diagonal), w, float(tau_ref), float(tau_learned), int(min_valid_per_row))
    return loss, stats, b, m


def soft_neighborhood_loss_gathered(ref: torch.Tensor, emb: torch.Tensor, ref_rows_a: torch.Tensor, ref_rows_b: torch.Tensor,
                                    emb_rows_a: torch.Tensor, emb_rows_b: torch.Tensor, lengths: torch.Tensor, exclude_diagonal: bool,
                                    tau_ref: float = 1.0, tau_learned: float = 1.0, pair_weights: Optional[torch.Tensor] = None,
                                    min_valid_per_row: int = 2, *, stats: bool = True) -> tuple[torch.Tensor, dict]:
    """The same loss with d_ref[b, t, t'] = |ref[ref_rows_a[b, t]] - ref[ref_rows_b[b, t']]|_2 and d_learned likewise from emb, the mask
    t < lengths[b] and t' < lengths[b] (minus the diagonal when exclude_diagonal).  ref [R, C] float32, emb [R, D] float32 | bfloat16,
    M <= 32, C <= 256, D <= 256.  The gradient flows to emb, in its dtype."""
    loss, vec, b, m = _gathered_term(ref, emb, ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b, lengths, exclude_diagonal, tau_ref, tau_learned,
                                     pair_weights, min_valid_per_row)
    if not stats:
        return loss, {}
    return loss, (_empty_stats(b, m) if vec is None else _stats_dict(vec.cpu().tolist(), b, m))


def phase_alignment(ysfc: torch.Tensor, pair_indices: torch.Tensor, min_overlap: int = 3):
    """ysfc [N, T] (integer-valued), pair_indices [B, 2] -> (valid_pair_mask [B] bool, rows_i [Bv, M], rows_j [Bv, M], lengths [Bv]).

    A recovery sequence starts at t = 0 and wherever ysfc falls below its previous value; a timestep scores len(its sequence) * (T + 1) + t,
    and the representative timestep of a (pixel, ysfc value) is the highest-scoring one with that value.  A pair's shared values are those
    present at both pixels, in ascending order: K of them, the pair is valid when K >= min_overlap, M = the largest K among valid pairs.
    rows_i[b, m] = i * T + best_t[i, v_m] (a row of the [N * T, .] view of per-timestep features), likewise rows_j; positions beyond
    lengths hold 0.  Integer torch ops on the device of the inputs; three host reads size its tensors (the distinct ysfc values, the
    valid pairs, M)."""
    n, t = ysfc.shape
    dev = ysfc.device
    pair_indices = pair_indices.to(dev, torch.int64).reshape(-1, 2)
    y = ysfc.to(torch.int64)
    start = torch.ones_like(y, dtype=torch.bool)
    start[:, 1:] = y[:, 1:] < y[:, :-1]
    seq = torch.cumsum(start.to(torch.int64), dim=1)
    seq_len = (seq.unsqueeze(2) == seq.unsqueeze(1)).sum(dim=2)                     # [N, T]: length of the sequence each timestep is in
    score = seq_len * (t + 1) + torch.arange(t, device=dev, dtype=torch.int64).unsqueeze(0)
    values, code = torch.unique(y, return_inverse=True)                             # ascending values; code [N, T] in [0, V)
    best = torch.full((n, values.numel()), -1, dtype=torch.int64, device=dev)
    best.scatter_reduce_(1, code.reshape(n, t), score, "amax", include_self=True)   # the largest score per (pixel, value); -1 = absent
    has_value = best >= 0
    best_t = torch.where(has_value, best % (t + 1), torch.zeros_like(best))
    first, second = pair_indices[:, 0], pair_indices[:, 1]
    common = has_value[first] & has_value[second]                                   # [B, V]
    overlap = common.sum(dim=1)
    valid = overlap >= min_overlap
    keep = valid.nonzero().squeeze(1)
    first, second, common, lengths = first[keep], second[keep], common[keep], overlap[keep]
    m = int(lengths.max()) if keep.numel() > 0 else 0
    # per pair the value indices with the common ones first, each group ascending (a stable sort on "not common"); the first K are the pair's
    ranked = torch.sort((~common).to(torch.int32), dim=1, stable=True).indices[:, :m]
    inside = torch.arange(m, device=dev).unsqueeze(0) < lengths.unsqueeze(1)
    rows_i = torch.where(inside, first.unsqueeze(1) * t + best_t[first].gather(1, ranked), 0)
    rows_j = torch.where(inside, second.unsqueeze(1) * t + best_t[second].gather(1, ranked), 0)
    return valid, rows_i, rows_j, lengths


def phase_neighborhood_loss(spectral_features: torch.Tensor, phase_embeddings: torch.Tensor, ysfc: torch.Tensor, pair_indices: torch.Tensor,
                            pair_weights: Optional[torch.Tensor] = None, tau_ref: float = 0.1, tau_learned: float = 0.1, min_overlap: int = 3,
                            min_valid_per_row: int = 2, self_similarity_weight: float = 1.0, cross_pixel_weight: float = 1.0,
                            _batch: Optional[dict] = None) -> tuple[torch.Tensor, dict]:
    """spectral_features [N, T, C], phase_embeddings [N, T, D], ysfc [N, T], pair_indices [B, 2] -> (loss, stats):
    self_similarity_weight * KL(self-distances of j's spectra || self-distances of i's embeddings, diagonal excluded)
    + cross_pixel_weight * KL(i-to-j spectral distances || i-to-j embedding distances, diagonal included), at the ysfc values the two
    pixels share (phase_alignment).  With a `_batch` dict in the layout of the reference's build_phase_neighborhood_batch the two matrix-form
    calls run on its matrices instead.  The reference's d_ref_* calibration statistics need the matrices in memory and are not produced."""
    if int(min_valid_per_row) < 2:
        raise ValueError(f"min_valid_per_row must be >= 2, got {min_valid_per_row}")
    dev = phase_embeddings.device
    n_input = int(pair_indices.shape[0])
    zero_stats = {"n_pairs_input": n_input, "n_pairs_sufficient_overlap": 0, "loss_self": 0.0, "loss_cross": 0.0}
    if _batch is not None:
        valid = _batch["valid_pair_mask"]
        n_valid = int(_batch["d_ref_self"].shape[0])
    else:
        valid, rows_i, rows_j, lengths = phase_alignment(ysfc, pair_indices, min_overlap)
        n_valid = int(lengths.numel())
    if n_valid == 0:
        return _zero(dev), zero_stats
    w = None if pair_weights is None else pair_weights.to(valid.device)[valid]
    if _batch is not None:
        loss_self, vec_self, b, m = _matrix_term(_batch["d_ref_self"], _batch["d_learned_self"], _batch["mask_self"], tau_ref, tau_learned, w,
                                                 min_valid_per_row)
        loss_cross, vec_cross, _, _ = _matrix_term(_batch["d_ref_cross"], _batch["d_learned_cross"], _batch["mask_cross"], tau_ref, tau_learned, w,
                                                   min_valid_per_row)
    else:
        nt = spectral_features.shape[0] * spectral_features.shape[1]
        ref = spectral_features.detach().reshape(nt, spectral_features.shape[2])
        emb = phase_embeddings.reshape(nt, phase_embeddings.shape[2])
        loss_self, vec_self, b, m = _gathered_term(ref, emb, rows_j, rows_j, rows_i, rows_i, lengths, True, tau_ref, tau_learned, w,
                                                   min_valid_per_row)
        loss_cross, vec_cross, _, _ = _gathered_term(ref, emb, rows_i, rows_j, rows_i, rows_j, lengths, False, tau_ref, tau_learned, w,
                                                     min_valid_per_row)
    loss = self_similarity_weight * loss_self + cross_pixel_weight * loss_cross
    host = torch.stack([vec_self, vec_cross]).cpu().tolist()                        # the one device-to-host copy of the diagnostics
    stats = {"n_pairs_input": n_input, "n_pairs_sufficient_overlap": n_valid, "loss_self": host[0][0], "loss_cross": host[1][0]}
    for prefix, vec in (("self_", host[0]), ("cross_", host[1])):
        for key, val in _stats_dict(vec, b, m).items():
            stats[prefix + key] = val
    return loss, stats
