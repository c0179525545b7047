"""Plain-torch float64 restatement of the soft-neighbourhood matching loss and of both closed-form gradients (with respect to the learned
distances, and through d[t, t'] = |a_t - b_t'|_2 to the gathered rows), checked against the reference-written fixtures
(tests/test_cpu_soft_neighborhood.py) and used for the shapes too large to commit (tests/test_gpu_soft_neighborhood.py); and the seeded
input makers the fixtures were drawn with.

    per pair b, row t, over the unmasked t' of that row:  lp = log_softmax(-d_ref / tau_ref), lq = log_softmax(-d_learned / tau_learned)
    kl[b,t] = sum p (lp - lq) if the row has >= min_valid unmasked entries;  L_b = sum_t kl / rows_b;  loss = sum w_b L_b / sum w_b (active pairs)
    d loss / d d_learned = w_b / (rows_b sum_w) (p - q) / tau_learned on the unmasked entries of contributing rows
    d a_t = sum_t' g[t,t'] (a_t - b_t') / d[t,t'],  d b_t' = -sum_t g[t,t'] (a_t - b_t') / d[t,t'],  0 where d = 0
"""
import torch

STAT_KEYS = ("n_pairs", "n_pairs_active", "n_rows_total", "n_rows_valid", "mean_kl", "mean_overlap", "mean_entropy_p", "mean_entropy_q")


def _masked_log_softmax(logits, mask):
    neg = torch.where(mask, logits, torch.full_like(logits, float("-inf")))
    top = neg.amax(dim=2, keepdim=True)
    top = torch.where(torch.isfinite(top), top, torch.zeros_like(top))
    e = torch.where(mask, torch.exp(logits - top), torch.zeros_like(logits))
    s = e.sum(dim=2, keepdim=True)
    s1 = torch.where(s > 0, s, torch.ones_like(s))
    logp = torch.where(mask, logits - top - torch.log(s1), torch.zeros_like(logits))
    return logp, e / s1


def soft_nbr_f64(d_reference, d_learned, mask, tau_ref=1.0, tau_learned=1.0, pair_weights=None, min_valid_per_row=2, upstream=1.0):
    """-> (loss python float, stats dict with STAT_KEYS, gradient float64 [B, M, M] of upstream * loss with respect to d_learned)."""
    dr = d_reference.detach().to("cpu", torch.float64)
    dl = d_learned.detach().to("cpu", torch.float64)
    mask = mask.detach().to("cpu", torch.bool)
    b, m, _ = dr.shape
    lp, p = _masked_log_softmax(-dr / tau_ref, mask)
    lq, q = _masked_log_softmax(-dl / tau_learned, mask)
    count = mask.sum(dim=2)
    row_ok = count >= min_valid_per_row
    kl = torch.where(row_ok, (p * (lp - lq)).sum(dim=2), torch.zeros(b, m, dtype=torch.float64))
    rows = row_ok.sum(dim=1).to(torch.float64)
    active = rows > 0
    per_pair = torch.where(active, kl.sum(dim=1) / rows.clamp(min=1), torch.zeros(b, dtype=torch.float64))
    w = torch.ones(b, dtype=torch.float64) if pair_weights is None else pair_weights.detach().to("cpu", torch.float64)
    w = w * active
    sw = float(w.sum())
    grad = torch.zeros_like(dl)
    loss = 0.0
    if sw > 0:
        loss = float((w * per_pair).sum() / sw)
        scale = (upstream * w / (rows.clamp(min=1) * sw)).reshape(b, 1, 1)
        grad = torch.where(mask & row_ok.unsqueeze(2), scale * (p - q) / tau_learned, grad)
    n_ok = int(row_ok.sum())
    mean = (lambda x: float(x[row_ok].mean())) if n_ok > 0 else (lambda x: 0.0)
    stats = {"n_pairs": b, "n_pairs_active": int(active.sum()), "n_rows_total": b * m, "n_rows_valid": n_ok, "mean_kl": loss,
             "mean_overlap": mean(count.to(torch.float64)), "mean_entropy_p": mean(-(p * lp).sum(dim=2)), "mean_entropy_q": mean(-(q * lq).sum(dim=2))}
    return loss, stats, grad


def pair_distances_f64(a, b):
    """a, b [B, M, W] -> |a_t - b_t'|_2 [B, M, M] in float64 from exact differences."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return torch.sqrt(((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(dim=3))


def length_mask(lengths, m, exclude_diagonal):
    ok = torch.arange(m).unsqueeze(0) < lengths.to("cpu").reshape(-1, 1)
    mask = ok.unsqueeze(2) & ok.unsqueeze(1)
    if exclude_diagonal:
        mask = mask & ~torch.eye(m, dtype=torch.bool).unsqueeze(0)
    return mask


def distance_grads_f64(a, b, g):
    """g [B, M, M] = d loss / d d with d = pair_distances_f64(a, b) -> (d loss / d a, d loss / d b), zero gradient where d = 0."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    d = pair_distances_f64(a, b)
    h = torch.where(d > 0, g / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
    ga = a * h.sum(dim=2, keepdim=True) - h @ b
    gb = b * h.sum(dim=1).unsqueeze(2) - h.transpose(1, 2) @ a
    return ga, gb


def gathered_f64(ref, emb, ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b, lengths, exclude_diagonal, tau_ref=1.0, tau_learned=1.0,
                 pair_weights=None, min_valid_per_row=2, upstream=1.0):
    """The gathered form: -> (loss, stats, gradient float64 [R, D] with respect to emb)."""
    ref, emb = ref.detach().to("cpu", torch.float64), emb.detach().to("cpu", torch.float64)
    idx = [r.to("cpu", torch.int64) for r in (ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b)]
    m = idx[0].shape[1]
    mask = length_mask(lengths, m, exclude_diagonal)
    a, b = emb[idx[2]], emb[idx[3]]
    loss, stats, g = soft_nbr_f64(pair_distances_f64(ref[idx[0]], ref[idx[1]]), pair_distances_f64(a, b), mask, tau_ref, tau_learned, pair_weights,
                                  min_valid_per_row, upstream)
    ga, gb = distance_grads_f64(a, b, g)
    de = torch.zeros_like(emb)
    de.index_add_(0, idx[2].reshape(-1), ga.reshape(-1, emb.shape[1]))
    de.index_add_(0, idx[3].reshape(-1), gb.reshape(-1, emb.shape[1]))
    return loss, stats, de


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def grid(x):
    """Values on a 2^-8 grid: exactly representable in float32, bfloat16-safe differences, and the stored arrays compress well."""
    return (torch.round(x.double() * 256.0) / 256.0).float()


def make_distances(b, m, seed, scale=2.0):
    """Two seeded non-negative [B, M, M] float32 blocks on the grid (reference, learned)."""
    g = torch.Generator().manual_seed(seed)
    return grid(torch.rand(b, m, m, generator=g, dtype=torch.float64) * scale), grid(torch.rand(b, m, m, generator=g, dtype=torch.float64) * scale)


def make_points(b, m, w, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return grid(torch.randn(b, m, w, generator=g, dtype=torch.float64) * scale)


def make_lengths(b, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, (b,), generator=g, dtype=torch.int64)


def make_weights(b, seed, zero_at=None):
    g = torch.Generator().manual_seed(seed)
    w = grid(0.25 + torch.rand(b, generator=g, dtype=torch.float64))
    if zero_at is not None:
        w[zero_at] = 0.0
    return w


def make_random_mask(b, m, seed, keep=0.6, lengths=None, exclude_diagonal=True):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(b, m, m, generator=g) < keep
    return mask & length_mask(torch.full((b,), m) if lengths is None else lengths, m, exclude_diagonal)


def make_ysfc(n, t, seed, reset=0.2):
    """Years-since-disturbance ramps with random resets: integer-valued float32 [N, T]."""
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(n, t)
    cur = torch.randint(0, 6, (n,), generator=g).float()
    for k in range(t):
        hit = torch.rand(n, generator=g) < reset
        cur = torch.where(hit, torch.zeros(n), cur + (1.0 if k > 0 else 0.0))
        y[:, k] = cur
    return y

