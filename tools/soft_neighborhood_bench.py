"""Phase neighbourhood (soft-neighbourhood KL) loss micro-benchmark, one JSON line per shape (appended to --out):
forward + backward of the fused HIP path (losses.phase_neighborhood_loss: phase_alignment, two gathered-form kernels each way, the
sorted-segment sum) against the same formula composed from stock torch ops (phase_alignment, row gathers, four torch.cdist, where /
log_softmax / softmax, autograd), on the same device in the same run, at B in {4096, 65536} valid pairs, M = T in {5, 15}, D = 12,
C = 8: 5 warm-up calls, then the median / min of 30 calls, HIP events around each call and a device synchronise after it, the two sides
alternating.  Two layouts per shape: "ramp", every pixel's ysfc is 0..T-1, so every pair is valid with K = M = T and nothing is padded;
"ragged", ramps with random resets, the first B pairs of a random pool with an overlap >= 3, K_b ragged and most pairs padded to M.
The times are call times: they include the index plumbing both sides share and the launch gaps of either side; the fused side also returns the diagnostics (one device-to-host
copy), the stock side computes none.  A second pass records the number of library calls per `_timed` span of one fused call and the
library's per-kernel event times.
Usage: python tools/soft_neighborhood_bench.py [--out profiles/soft_neighborhood_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import phase_alignment, phase_neighborhood_loss  # noqa: E402

DEV = "cuda:0"


def stock_term(d_ref, d_learned, mask, tau_ref, tau_learned, weights, min_valid=2):
    neg = torch.full((), -1e9, device=d_ref.device)
    lr = torch.where(mask, -d_ref / tau_ref, neg)
    ll = torch.where(mask, -d_learned / tau_learned, neg)
    row_ok = mask.sum(dim=2) >= min_valid
    lp, lq = lr.log_softmax(dim=2), ll.log_softmax(dim=2)
    kl = torch.where(row_ok, (lr.softmax(dim=2) * (lp - lq)).sum(dim=2), torch.zeros((), device=d_ref.device))
    rows = row_ok.float().sum(dim=1)
    w = weights * (rows > 0).float()
    return (w * kl.sum(dim=1) / rows.clamp(min=1)).sum() / w.sum()


def stock_phase_loss(spectral, phase, ysfc, pairs, weights, tau_ref=0.1, tau_learned=0.1):
    valid, ri, rj, lengths = phase_alignment(ysfc, pairs)
    m = ri.shape[1]
    ref, emb = spectral.reshape(-1, spectral.shape[2]), phase.reshape(-1, phase.shape[2])
    si, sj, zi, zj = ref[ri], ref[rj], emb[ri], emb[rj]
    ok = torch.arange(m, device=ysfc.device).unsqueeze(0) < lengths.unsqueeze(1)
    mask_cross = ok.unsqueeze(2) & ok.unsqueeze(1)
    mask_self = mask_cross & ~torch.eye(m, dtype=torch.bool, device=ysfc.device).unsqueeze(0)
    w = weights[valid]
    return (stock_term(torch.cdist(sj, sj), torch.cdist(zi, zi), mask_self, tau_ref, tau_learned, w)
            + stock_term(torch.cdist(si, sj), torch.cdist(zi, zj), mask_cross, tau_ref, tau_learned, w))


def ragged_ysfc(n, t, g, reset=0.2):
    """Years-since-disturbance ramps with random resets, integer-valued float32 [N, T]."""
    y = torch.zeros(n, t)
    cur = torch.randint(0, 6, (n,), generator=g).float()
    for k in range(t):
        cur = torch.where(torch.rand(n, generator=g) < reset, torch.zeros(n), cur + (1.0 if k > 0 else 0.0))
        y[:, k] = cur
    return y


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from frl_hip import ops
    lines = []
    c, d, n = 8, 12, 8192
    for b, t, layout in [(b, t, layout) for b in (4096, 65536) for t in (5, 15) for layout in ("ramp", "ragged")]:
        g = torch.Generator().manual_seed(b + t)
        spectral = torch.randn(n, t, c, generator=g).to(DEV)
        phase = torch.randn(n, t, d, generator=g).to(DEV).requires_grad_(True)
        if layout == "ramp":                             # K = M = T for every pair: no padding
            ysfc = torch.arange(t, dtype=torch.float32).repeat(n, 1).to(DEV)
            pairs = torch.randint(0, n, (b, 2), generator=g).to(DEV)
        else:                                            # ramps with random resets: K_b ragged in [3, M], padded positions in most pairs
            ysfc = ragged_ysfc(n, t, g).to(DEV)
            pool = torch.randint(0, n, (4 * b, 2), generator=g).to(DEV)
            pairs = pool[phase_alignment(ysfc, pool)[0]][:b].contiguous()
            assert pairs.shape[0] == b
        lengths = phase_alignment(ysfc, pairs)[3]
        weights = (0.25 + torch.rand(b, generator=g)).to(DEV)
        out = {}

        def fused():
            phase.grad = None
            loss, stats = phase_neighborhood_loss(spectral, phase, ysfc, pairs, pair_weights=weights)
            loss.backward()
            out["fused"], out["stats"] = float(loss.detach()), stats

        def stock():
            phase.grad = None
            loss = stock_phase_loss(spectral, phase, ysfc, pairs, weights)
            loss.backward()
            out["stock"] = float(loss.detach())

        (fm, fmin), (sm, smin) = timed([fused, stock])
        assert out["stats"]["n_pairs_sufficient_overlap"] == b and out["stats"]["self_n_rows_valid"] == int(lengths.sum())
        ops.set_timing(True)
        fused()
        spans = {k: v[0] for k, v in ops.timing_summary().items()}
        ops.set_timing(False)
        ops.kernel_timing(True)
        ops.kernel_timing_report()
        for _ in range(10):
            fused()
        torch.cuda.synchronize()
        kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
        ops.kernel_timing(False)
        line = {"case": "phase_neighborhood_fwd_bwd", "B_valid": b, "T": t, "layout": layout, "M": int(lengths.max()),
                "K_mean": round(float(lengths.float().mean()), 2), "padded_positions": int((int(lengths.max()) - lengths).sum()), "D": d, "C": c,
                "N": n, "fused_us_median": round(fm, 1), "fused_us_min": round(fmin, 1), "torch_ops_us_median": round(sm, 1), "torch_ops_us_min": round(smin, 1),
                "speedup_at_median": round(sm / fm, 2), "loss_fused": out["fused"], "loss_torch_ops": out["stock"],
                "timing": "call time, HIP events around the Python call, a synchronise after each, the two sides alternating",
                "fused_library_calls_per_span": spans, "fused_kernel_us_mean_of_10": kernels}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
