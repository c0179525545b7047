"""Phase margin losses micro-benchmark, one JSON line per loss and size (appended to --out): forward + backward of the fused HIP path
(losses.phase_recovery_discrimination_loss; losses.phase_spread_ranking_gathered on the rows of one phase_alignment call made outside the
timed region) against the reference's formula composed from stock torch ops on the same device in the same run: for the recovery loss the
reference's own sequence (class masks, two host reads, the compaction to active pixels, the [N_a, T, T, D] difference tensor, softplus
over the masked pairs, autograd); for the spread ranking the two gathers, two torch.cdist blocks, the length mask and the ranking tail,
with none of the diagnostics.  Shapes are those of the reference's step: N = 964 pixels and 16 x 964, T = 15, D = 12, B = 4 N pairs, ysfc
ramps with resets.  Both sides are called with stats off (the fused side makes no host read).  5 warm-up calls, then the median / min
of 30 calls, HIP events around each Python call and a device synchronise after it, the two sides alternating.  A second pass records the
library's per-kernel event times of the fused call.
Usage: python tools/phase_margin_bench.py [--out profiles/phase_margin_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import phase_alignment, phase_recovery_discrimination_loss, phase_spread_ranking_gathered  # noqa: E402

DEV = "cuda:0"


def ramps(n, t, g, reset=0.2):
    """Years-since-disturbance ramps with random resets, integer-valued float32 [N, T]."""
    y = torch.zeros(n, t)
    cur = torch.randint(0, 6, (n,), generator=g).float()
    for k in range(t):
        cur = torch.where(torch.rand(n, generator=g) < reset, torch.zeros(n), cur + (1.0 if k > 0 else 0.0))
        y[:, k] = cur
    return y


def stock_recovery(z, ysfc, margin=0.5, low_ysfc_max=1.0, high_ysfc_min=5.0):
    valid = torch.isfinite(ysfc) & (ysfc >= 0)
    is_low, is_high = valid & (ysfc <= low_ysfc_max), valid & (ysfc >= high_ysfc_min)
    active = is_low.any(dim=1) & is_high.any(dim=1)
    if int(active.sum().item()) == 0:
        return torch.zeros((), device=z.device, requires_grad=True)
    za, low_a, high_a = z[active], is_low[active], is_high[active]
    pair_mask = low_a.unsqueeze(2) & high_a.unsqueeze(1)
    int(pair_mask.sum().item())                                          # the reference's n_pairs read
    dists = (za.unsqueeze(2) - za.unsqueeze(1)).pow(2).sum(dim=-1).clamp(min=1e-12).sqrt()
    return F.softplus(margin - dists)[pair_mask].mean()


def stock_spread(emb, rows_i, rows_j, lengths, ref_diff, margin=0.1, delta=0.5):
    a, b = emb[rows_i], emb[rows_j]
    d_i, d_j = torch.cdist(a, a), torch.cdist(b, b)
    m = rows_i.shape[1]
    ok = torch.arange(m, device=emb.device).unsqueeze(0) < lengths.unsqueeze(1)
    mask = ok.unsqueeze(2) & ok.unsqueeze(1) & ~torch.eye(m, dtype=torch.bool, device=emb.device).unsqueeze(0)
    nb = mask.float().sum(dim=(1, 2)).clamp(min=1)
    si, sj = (d_i * mask).sum(dim=(1, 2)) / nb, (d_j * mask).sum(dim=(1, 2)) / nb
    return (F.softplus(sj - si + margin) * (ref_diff > delta).float() + F.softplus(si - sj + margin) * (ref_diff < -delta).float()).mean()


def timed(fns, n=30, warm=5):
    """fns: callables timed alternately -> [(median us, min us)] in their order."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return [(sorted(t)[len(t) // 2], min(t)) for t in ts]


def compare(name, x, fused_loss, stock_loss, extra):
    """x: the leaf both sides differentiate.  -> the JSON line."""
    from frl_hip import ops
    out = {}

    def fused():
        x.grad = None
        loss = fused_loss()
        loss.backward()
        out["fused"] = loss

    def stock():
        x.grad = None
        loss = stock_loss()
        loss.backward()
        out["stock"] = loss

    (fm, fmin), (sm, smin) = timed([fused, stock])
    fused()
    g_fused, l_fused = x.grad.clone(), float(out["fused"].detach())
    stock()
    l_stock = float(out["stock"].detach())
    grad_dev = float((g_fused - x.grad).abs().max() / x.grad.abs().max().clamp(min=1e-30))
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(10):
        fused()
    torch.cuda.synchronize()
    kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
    ops.kernel_timing(False)
    line = {"case": name, **extra, "fused_us_median": round(fm, 1), "fused_us_min": round(fmin, 1), "torch_ops_us_median": round(sm, 1),
            "torch_ops_us_min": round(smin, 1), "speedup_at_median": round(sm / fm, 2), "loss_fused": l_fused, "loss_torch_ops": l_stock,
            "grad_max_dev_over_max": grad_dev,
            "timing": "call time, HIP events around the Python call (stats off), a synchronise after each, the two sides alternating",
            "fused_kernel_us_mean_of_10": kernels}
    print(json.dumps(line), flush=True)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t, d, lines = 15, 12, []
    for samples in (1, 16):
        n = 964 * samples
        g = torch.Generator().manual_seed(samples)
        z = (torch.randn(n, t, d, generator=g) * 0.25).to(DEV).requires_grad_(True)
        ysfc = ramps(n, t, g).to(DEV)
        lines.append(compare("recovery_discrimination_fwd_bwd", z, lambda: phase_recovery_discrimination_loss(z, ysfc, stats=False)[0],
                             lambda: stock_recovery(z, ysfc), {"N": n, "T": t, "D": d}))
        pairs = torch.randint(0, n, (4 * n, 2), generator=g).to(DEV)
        dyn = torch.randn(n, generator=g).to(DEV)
        valid, rows_i, rows_j, lengths = phase_alignment(ysfc, pairs, 3)
        kept = pairs[valid]
        ref_diff = dyn[kept[:, 0]] - dyn[kept[:, 1]]
        emb = z.detach().reshape(n * t, d).clone().requires_grad_(True)
        lines.append(compare("spread_ranking_gathered_fwd_bwd", emb,
                             lambda: phase_spread_ranking_gathered(emb, rows_i, rows_j, lengths, ref_diff, stats=False)[0],
                             lambda: stock_spread(emb, rows_i, rows_j, lengths, ref_diff),
                             {"N": n, "T": t, "D": d, "pairs": int(pairs.shape[0]), "valid_pairs": int(lengths.numel()), "M": int(rows_i.shape[1])}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
