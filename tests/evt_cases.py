"""Plain-torch float64 restatement of the EVT soft-neighbourhood loss and of its closed-form gradient, checked against the
reference-written fixtures (tests/test_cpu_evt_soft_neighborhood.py) and used for the shapes without a fixture
(tests/test_gpu_evt_soft_neighborhood.py); and the seeded input makers the fixtures were drawn with.

    per segment, idx = the anchors' code indices (-1 = unknown):
    valid_i = idx_i >= 0;  mask_ij = valid_i and valid_j and idx_i != idx_j;  active_i = (sum_j mask_ij) >= 2
    a_ij = -(1 - S[idx_i, idx_j]) / tau_ref (1 - S in float32, as the reference's d_ref),  b_ij = -|e_i - e_j|_2 / tau_learned
    p = softmax_j a, q = softmax_j b over the mask;  KL_i = sum_j p (log p - log q)
    loss = sum_i w[idx_i] active_i KL_i / W,  W = sum_i w[idx_i] active_i;  0 with fewer than min_valid_anchors valid anchors or W <= 0
    c_i = upstream w[idx_i] active_i / W,  G_ij = -c_i (q_ij - p_ij) / tau_learned,  d e_i = sum_j (G_ij + G_ji) (e_i - e_j) / d_ij, 0 where d_ij = 0

To reproduce the reference's "float64" results to 1e-12, what its code leaves in float32 whatever the dtype of the embeddings is formed in
float32 here too, by the same torch ops on the valid anchors: d_ref and the reference logits (its 0-dim -1e9 fill does not promote the
float32 d_ref), hence p, log p and H(p); and the sum W of the float32 weights.  All are float32 roundings of the definition (1e-7
relative); since sum_j p_ij is then 1 only to float32, the gradient the reference's autograd returns is -c_i (q_ij sum_j p_ij - p_ij).
"""
import math

import torch

COUNT_KEYS = ("n_anchors_in", "n_anchors_valid", "n_rows_active")
MEAN_KEYS = ("mean_kl", "mean_entropy_ref", "mean_entropy_learned", "d_lrn_confused", "d_lrn_noncf", "n_confused_pairs", "eff_n_ref")
CASES = ("a", "b", "c", "d", "e", "f")
METRIC_SETTINGS = {"a": {}, "b": {"laplace_smoothing": 0.1, "diffusion_steps": 3}, "c": {"binary_threshold": 0.05}}
CASE_METRIC = {"a": "a", "b": "b", "c": "c", "d": "a", "e": "a", "f": "a"}


def _masked_log_softmax(logits, mask):
    neg = torch.where(mask, logits, torch.full_like(logits, float("-inf")))
    top = neg.amax(dim=1, keepdim=True)
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    e = torch.where(mask, torch.exp(logits - top), torch.zeros_like(logits))
    s = e.sum(dim=1, keepdim=True)
    s1 = torch.where(s > 0, s, torch.ones_like(s))
    return torch.where(mask, logits - top - torch.log(s1), torch.zeros_like(logits)), e / s1


def segment_f64(emb, idx, S, w, tau_ref=0.5, tau_learned=0.5, min_valid_anchors=4, upstream=1.0):
    """One segment: emb [M, D], idx [M] (-1 = unknown), S [K, K] float32, w [K] float32 -> (loss python float, stats dict,
    gradient float64 [M, D] of upstream * loss with respect to emb)."""
    e_all = emb.detach().to("cpu", torch.float64)
    ix_all = idx.detach().to("cpu", torch.int64)
    S32, w32 = S.detach().to("cpu", torch.float32), w.detach().to("cpu", torch.float32)
    stats = {"n_anchors_in": e_all.shape[0], "n_anchors_valid": 0, "n_rows_active": 0, **{k: 0.0 for k in MEAN_KEYS}}
    grad = torch.zeros_like(e_all)
    rows = (ix_all >= 0).nonzero().squeeze(1)
    stats["n_anchors_valid"] = m = int(rows.numel())
    if m == 0 or m < min_valid_anchors:
        return 0.0, stats, grad
    e, ix = e_all[rows], ix_all[rows]                                   # the valid anchors
    d_ref32 = 1.0 - S32[ix[:, None], ix[None, :]]
    mask = ix[:, None] != ix[None, :]                                   # (off the diagonal: an anchor shares its own code)
    d = torch.sqrt(((e[:, None, :] - e[None, :, :]) ** 2).sum(dim=2))
    logits32 = torch.where(mask, -d_ref32 / tau_ref, torch.tensor(-1e9, dtype=torch.float32))
    lp32, p32 = logits32.log_softmax(dim=1), logits32.softmax(dim=1)    # float32: p = 0 exactly off the mask
    lp, p = torch.where(mask, lp32.double(), torch.zeros_like(d)), p32.double()
    lq, q = _masked_log_softmax(-d / tau_learned, mask)
    active = mask.sum(dim=1) >= 2
    stats["n_rows_active"] = int(active.sum())
    if not active.any():
        return 0.0, stats, grad
    kl = torch.where(active, (p * (lp - lq)).sum(dim=1), torch.zeros(m, dtype=torch.float64))
    wi = w32[ix] * active.float()
    total = float(wi.sum())                                             # float32, in the reference's order
    if not total > 0:
        return 0.0, stats, grad
    loss = float((wi.double() * kl).sum() / total)
    c = upstream * wi.double() / total
    g = torch.where(mask & active[:, None], -c[:, None] * (q * p.sum(dim=1, keepdim=True) - p) / tau_learned, torch.zeros_like(d))
    g = g + g.T
    h = torch.where(d > 0, g / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
    grad[rows] = e * h.sum(dim=1, keepdim=True) - h @ e
    confused = (d_ref32 < (1.0 - 1e-6)) & mask
    other = (d_ref32 >= (1.0 - 1e-6)) & mask
    ent_ref = float((-(p32 * lp32).sum(dim=1))[active].mean())
    stats.update(mean_kl=loss, mean_entropy_ref=ent_ref, mean_entropy_learned=float((-(q * lq).sum(dim=1))[active].mean()),
                 d_lrn_confused=float(d[confused].mean()) if confused.any() else 0.0,
                 d_lrn_noncf=float(d[other].mean()) if other.any() else 0.0,
                 n_confused_pairs=float(confused.sum(dim=1).float()[active].mean()), eff_n_ref=math.exp(ent_ref))
    return loss, stats, grad


def evt_f64(emb, idx, S, w, seg, tau_ref=0.5, tau_learned=0.5, min_valid_anchors=4, seg_weights=None, upstream=None):
    """Every segment of emb [N, D]: seg = offsets [S + 1]; upstream = the gradient of each segment's (weighted) loss, default ones ->
    (losses list [S], unweighted; stats list [S]; gradient float64 [N, D])."""
    seg = [int(v) for v in seg]
    losses, stats, grads = [], [], []
    for s in range(len(seg) - 1):
        up = (1.0 if upstream is None else float(upstream[s])) * (1.0 if seg_weights is None else float(seg_weights[s]))
        lo, st, g = segment_f64(emb[seg[s]:seg[s + 1]], idx[seg[s]:seg[s + 1]], S, w, tau_ref, tau_learned, min_valid_anchors, up)
        losses.append(lo)
        stats.append(st)
        grads.append(g)
    return losses, stats, torch.cat(grads) if grads else torch.zeros(0, emb.shape[1], dtype=torch.float64)


def code_index(codes, kept):
    """The dict lookup: codes (any ints) -> index into the ascending list `kept`, -1 when absent."""
    table = {int(c): k for k, c in enumerate(kept)}
    return torch.tensor([table.get(int(c), -1) for c in codes], dtype=torch.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def grid(x):
    """Values on a 2^-8 grid: exactly representable in float32 and bfloat16-safe differences; the stored arrays compress well."""
    return (torch.round(x.double() * 256.0) / 256.0).float()


def make_embeddings(n, d, seed, scale=0.25):
    g = torch.Generator().manual_seed(seed)
    return grid(torch.randn(n, d, generator=g, dtype=torch.float64) * scale)


def make_codes(n, seed, known, unknown=(), unknown_share=0.0):
    """n codes drawn from `known` (a list of ints), a share of them from `unknown`."""
    g = torch.Generator().manual_seed(seed)
    pick = torch.tensor(known, dtype=torch.int64)[torch.randint(0, len(known), (n,), generator=g)]
    if len(unknown) and unknown_share > 0:
        bad = torch.tensor(unknown, dtype=torch.int64)[torch.randint(0, len(unknown), (n,), generator=g)]
        pick = torch.where(torch.rand(n, generator=g) < unknown_share, bad, pick)
    return pick


def make_case(name, kept, dropped):
    """The inputs of fixture case `name`: kept = the metric's codes (ascending), dropped = codes the metric does not hold ->
    dict(emb [N, D] float32, codes [N] int64, seg [S + 1], tau_ref, tau_learned, min_valid_anchors)."""
    kept, dropped = [int(c) for c in kept], [int(c) for c in dropped]
    kw = dict(tau_ref=0.5, tau_learned=0.5, min_valid_anchors=4)
    if name == "a":
        emb, codes = make_embeddings(48, 64, 401), make_codes(48, 411, kept)
    elif name == "b":
        emb, codes = make_embeddings(200, 64, 402), make_codes(200, 412, kept, dropped, 0.15)
        kw.update(tau_ref=0.25, tau_learned=0.5)
    elif name == "c":                                                   # one dominant code and a single anchor of another: one active row
        emb = make_embeddings(37, 12, 403, scale=0.5)
        codes = torch.full((37,), kept[0], dtype=torch.int64)
        codes[20] = kept[3]
    elif name == "d":                                                   # three valid anchors among nine
        emb = make_embeddings(9, 64, 404)
        codes = torch.tensor([dropped[k % len(dropped)] for k in range(9)], dtype=torch.int64)
        codes[1], codes[4], codes[7] = kept[0], kept[1], kept[2]
    elif name == "e":                                                   # two pairs of identical embeddings with different codes
        emb, codes = make_embeddings(16, 64, 405, scale=1.0), make_codes(16, 415, kept)
        emb[5], emb[12] = emb[2], emb[9]
        codes[2], codes[5], codes[9], codes[12] = kept[0], kept[1], kept[2], kept[4]
    elif name == "f":                                                   # three segments of 48, 3 and 130 rows
        emb, codes = make_embeddings(181, 64, 406), make_codes(181, 416, kept, dropped, 0.1)
        return dict(emb=emb, codes=codes, seg=[0, 48, 51, 181], **kw)
    else:
        raise KeyError(name)
    return dict(emb=emb, codes=codes, seg=[0, emb.shape[0]], **kw)
