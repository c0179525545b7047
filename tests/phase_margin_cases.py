"""Plain-torch float64 restatement of the two phase margin losses (the recovery discrimination loss and the phase spread ranking) and of
their closed-form gradients, checked against the reference-written fixtures (tests/test_cpu_phase_margin.py) and used where a fixture
holds only part of a gradient or no fixture is committed (tests/test_gpu_phase_margin.py); and the seeded input makers the fixtures were
drawn with, on top of those of tests/soft_neighborhood_cases.py.

    recovery discrimination, per pixel:  low = valid & (ysfc <= low_max), high = valid & (ysfc >= high_min), valid = isfinite & (ysfc >= 0)
        d = sqrt(max(|z_tl - z_th|^2, 1e-12)) over the pairs (tl, th) with low[tl] and high[th];  loss = sum softplus(margin - d) / n_pairs
        d z_tl += -g sigmoid(margin - d) / n_pairs (z_tl - z_th) / d,  z_th the negative;  0 where the sum of squares is under the clamp
    spread ranking, per pair b:  n_b = max(1, unmasked), spread_i = sum mask d_i / n_b, spread_j likewise, r_b = ref_diff[b]
        term_b = softplus(spread_j - spread_i + margin) [r_b > delta] + softplus(spread_i - spread_j + margin) [r_b < -delta]
        loss = sum term_b / B;  d loss / d d_i = g c_b / (B n_b) mask,  d loss / d d_j its negative,  c_b = d term_b / d spread_i
"""
import torch

import soft_neighborhood_cases as SC

SPREAD_COUNTS = ("n_pairs", "n_constrained_i", "n_constrained_j")
SPREAD_MEANS = ("frac_satisfied", "mean_spread_i", "mean_spread_j", "mean_ref_diff")


def softplus64(x):
    """torch's softplus (beta 1, threshold 20)."""
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def recovery_classes(ysfc, low_ysfc_max=1.0, high_ysfc_min=5.0):
    y = ysfc.detach().to("cpu", torch.float64)
    valid = torch.isfinite(y) & (y >= 0)
    return valid & (y <= low_ysfc_max), valid & (y >= high_ysfc_min)


def recovery_f64(z, ysfc, margin=0.5, low_ysfc_max=1.0, high_ysfc_min=5.0, upstream=1.0):
    """-> (loss python float, {"n_pairs", "n_active_pixels"}, gradient float64 [N, T, D] of upstream * loss with respect to z)."""
    z = z.detach().to("cpu", torch.float64)
    low, high = recovery_classes(ysfc, low_ysfc_max, high_ysfc_min)
    pair = low.unsqueeze(2) & high.unsqueeze(1)                                     # [N, tl, th]
    n_pairs = int(pair.sum())
    stats = {"n_pairs": n_pairs, "n_active_pixels": int((low.any(dim=1) & high.any(dim=1)).sum())}
    grad = torch.zeros_like(z)
    if n_pairs == 0:
        return 0.0, stats, grad
    loss = 0.0
    for n in pair.flatten(1).any(dim=1).nonzero().flatten().tolist():              # pixel by pixel: [T, T, D] differences at a time
        diff = z[n].unsqueeze(1) - z[n].unsqueeze(0)                                # [tl, th, D]
        ss = (diff ** 2).sum(dim=2)
        d = torch.sqrt(torch.clamp(ss, min=1e-12))
        loss = loss + float(softplus64(margin - d)[pair[n]].sum())
        h = torch.where(pair[n] & (ss > 1e-12), -upstream * torch.sigmoid(margin - d) / (n_pairs * d), torch.zeros_like(d))
        hd = h.unsqueeze(2) * diff
        grad[n] = hd.sum(dim=1) - hd.sum(dim=0)
    return loss / n_pairs, stats, grad


def spread_matrix_f64(d_i, d_j, mask, ref_diff, margin=0.1, delta=0.5, upstream=1.0):
    """-> (loss, stats dict, (gradient float64 [B, M, M] with respect to d_i, likewise d_j), per-pair (spread_i, spread_j))."""
    d_i, d_j = d_i.detach().to("cpu", torch.float64), d_j.detach().to("cpu", torch.float64)
    mask = mask.detach().to("cpu", torch.bool)
    r = ref_diff.detach().to("cpu", torch.float64)
    b = d_i.shape[0]
    nb = mask.sum(dim=(1, 2)).clamp(min=1).to(torch.float64)
    si, sj = (d_i * mask).sum(dim=(1, 2)) / nb, (d_j * mask).sum(dim=(1, 2)) / nb
    ci, cj = r > delta, r < -delta
    xi, xj = sj - si + margin, si - sj + margin
    zero = torch.zeros_like(si)
    loss = float((torch.where(ci, softplus64(xi), zero) + torch.where(cj, softplus64(xj), zero)).sum() / b)
    coef = torch.where(ci, -torch.sigmoid(xi), zero) + torch.where(cj, torch.sigmoid(xj), zero)
    gi = (upstream * coef / (b * nb)).reshape(b, 1, 1) * mask
    n_con = int(ci.sum() + cj.sum())
    sat = int((ci & ((si - sj) > margin)).sum() + (cj & ((sj - si) > margin)).sum())
    stats = {"n_pairs": b, "n_constrained_i": int(ci.sum()), "n_constrained_j": int(cj.sum()), "frac_satisfied": sat / n_con if n_con else 1.0,
             "mean_spread_i": float(si.mean()), "mean_spread_j": float(sj.mean()), "mean_ref_diff": float(r.abs().mean())}
    return loss, stats, (gi, -gi), (si, sj)


def spread_gathered_f64(emb, rows_i, rows_j, lengths, ref_diff, margin=0.1, delta=0.5, upstream=1.0):
    """The gathered form: -> (loss, stats, gradient float64 [R, D] with respect to emb)."""
    emb = emb.detach().to("cpu", torch.float64)
    ri, rj = rows_i.to("cpu", torch.int64), rows_j.to("cpu", torch.int64)
    mask = SC.length_mask(lengths, ri.shape[1], True)
    a, b = emb[ri], emb[rj]
    loss, stats, (gi, gj), _ = spread_matrix_f64(SC.pair_distances_f64(a, a), SC.pair_distances_f64(b, b), mask, ref_diff, margin, delta, upstream)
    de = torch.zeros_like(emb)
    for rows, pts, g in ((ri, a, gi), (rj, b, gj)):
        g1, g2 = SC.distance_grads_f64(pts, pts, g)
        de.index_add_(0, rows.reshape(-1), (g1 + g2).reshape(-1, emb.shape[1]))
    return loss, stats, de


def self_distance_blocks(emb, rows, lengths):
    """float64 self-distances [B, M, M] of the gathered rows, zero where masked, and the mask."""
    pts = emb.detach().to("cpu", torch.float64)[rows.to("cpu", torch.int64)]
    mask = SC.length_mask(lengths, rows.shape[1], True)
    d = SC.pair_distances_f64(pts, pts)
    return torch.where(mask, d, torch.zeros_like(d)), mask


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def plant_invalid(ysfc, seed, nan_frac=0.0, neg_frac=0.0):
    """A copy of ysfc with a seeded fraction of entries replaced by NaN and by -1 (both invalid)."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(ysfc.shape, generator=g)
    y = ysfc.clone().float()
    y[u < nan_frac] = float("nan")
    y[(u >= nan_frac) & (u < nan_frac + neg_frac)] = -1.0
    return y


def make_dynamism(n, seed, scale=1.0):
    """Per-pixel dynamism scores on the 2^-8 grid: differences and their comparison with delta are exact in float32."""
    g = torch.Generator().manual_seed(seed)
    return SC.grid(torch.randn(n, generator=g, dtype=torch.float64) * scale)


def make_pairs(n, b, seed, self_pairs=0):
    g = torch.Generator().manual_seed(seed)
    pairs = torch.randint(0, n, (b, 2), generator=g, dtype=torch.int64)
    pairs[:self_pairs, 1] = pairs[:self_pairs, 0]
    return pairs
