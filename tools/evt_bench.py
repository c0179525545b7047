"""EVT soft-neighbourhood loss micro-benchmark, one JSON line per shape (appended to --out): forward + backward of the fused HIP path
(losses.evt_soft_neighborhood_loss_batched: the code lookup, one forward launch pair, one backward launch, the one device-to-host copy of
the diagnostics) against the reference's formula composed from stock torch ops on the same device in the same run (per segment:
torch.cdist, two masked logit matrices, two log_softmax, a softmax, autograd), at 1 and 16 segments of N = 964 anchors, D = 64, a metric
of K = 60 codes, about 10 % unknown codes.  The stock side gets the tensorised code lookup too, so the comparison is about the kernels; it
computes none of the diagnostics.  5 warm-up calls, then the median / min of 30 calls, HIP events around each call and a device
synchronise after it, the two sides alternating.  The reference's own lookup (three `.item()` reads per anchor in Python list
comprehensions) is timed once for one segment with a host clock and reported separately.  A second pass records the library's per-kernel
event times of the fused call.
Usage: python tools/evt_bench.py [--out profiles/evt_bench.jsonl]"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import EvtDiffusionMetric, evt_soft_neighborhood_loss_batched  # noqa: E402

DEV = "cuda:0"


def synthetic_metric(k=60, seed=0):
    g = np.random.default_rng(seed)
    codes = [7000 + 3 * i for i in range(k)]
    table = np.where(g.random((k, k)) < 0.15, g.integers(1, 80, (k, k)), 0)
    table[np.arange(k), np.arange(k)] = g.integers(60, 500, k)
    counts = {str(c): int(v) for c, v in zip(codes, g.integers(200, 200000, k))}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "confusion.csv")
        with open(path, "w", newline="") as fh:
            out = csv.writer(fh)
            out.writerow(["", *codes])
            for c, row in zip(codes, table.tolist()):
                out.writerow([c, *row])
        return EvtDiffusionMetric(path, counts), codes


def stock_segment(emb, idx, S, w, tau_ref=0.5, tau_learned=0.5):
    """The reference's loss on one segment from stock torch ops, with a tensorised lookup (idx = metric.code_index(codes))."""
    valid = idx >= 0
    ix = idx[valid].long()
    e = emb[valid]
    d_ref = 1.0 - S[ix[:, None], ix[None, :]]
    d = torch.cdist(e, e)
    mask = ix[:, None] != ix[None, :]
    neg = torch.tensor(-1e9, device=emb.device)
    lr, ll = torch.where(mask, -d_ref / tau_ref, neg), torch.where(mask, -d / tau_learned, neg)
    active = mask.sum(dim=1) >= 2
    lp, lq, p = lr.log_softmax(dim=1), ll.log_softmax(dim=1), lr.softmax(dim=1)
    kl = torch.where(active, (p * (lp - lq)).sum(dim=1), torch.zeros((), device=emb.device))
    rw = w[ix] * active.float()
    return (rw * kl).sum() / rw.sum()


def reference_lookup_seconds(codes, metric):
    """The reference's reference_distances + anchor_weights lookups for one segment: three .item() reads per anchor."""
    table = metric._code_to_idx
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    valid = torch.tensor([c.item() in table for c in codes], dtype=torch.bool, device=codes.device)
    idx = torch.tensor([table.get(c.item(), 0) for c in codes], dtype=torch.long, device=codes.device)
    wts = torch.tensor([metric._freq_weights[table[c.item()]].item() if c.item() in table else 0.0 for c in codes], device=codes.device)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, (valid, idx, wts)


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
    metric, kept = synthetic_metric()
    metric.to(DEV)
    n, d = 964, 64
    lines = []
    lookup_s, _ = reference_lookup_seconds(torch.tensor(kept, device=DEV)[torch.arange(n, device=DEV) % len(kept)], metric)
    for nseg in (1, 16):
        g = torch.Generator().manual_seed(nseg)
        emb = (torch.randn(nseg * n, d, generator=g) * 0.25).to(DEV).requires_grad_(True)
        codes = torch.tensor(kept)[torch.randint(0, len(kept), (nseg * n,), generator=g)]
        codes = torch.where(torch.rand(nseg * n, generator=g) < 0.1, torch.full_like(codes, 9999), codes).to(DEV)
        seg = [n * s for s in range(nseg + 1)]
        out = {}

        def fused():
            emb.grad = None
            loss, stats = evt_soft_neighborhood_loss_batched(emb, codes, seg, metric)
            loss.backward()
            out["fused"], out["stats"] = float(loss.detach()), stats

        def stock():
            emb.grad = None
            idx = metric.code_index(codes)
            loss = sum(stock_segment(emb[a:b], idx[a:b], metric._S, metric._freq_weights) for a, b in zip(seg[:-1], seg[1:])) / nseg
            loss.backward()
            out["stock"] = float(loss.detach())

        (fm, fmin), (sm, smin) = timed([fused, stock])
        fused()
        g_fused = emb.grad.clone()
        stock()
        grad_dev = float((g_fused - emb.grad).abs().max() / emb.grad.abs().max())
        ops.kernel_timing(True)
        ops.kernel_timing_report()
        for _ in range(10):
            fused()
        torch.cuda.synchronize()
        kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
        ops.kernel_timing(False)
        line = {"case": "evt_soft_neighborhood_fwd_bwd", "segments": nseg, "N_per_segment": n, "D": d, "K": metric.n_codes,
                "valid_anchors": out["stats"]["n_anchors_valid"], "fused_us_median": round(fm, 1), "fused_us_min": round(fmin, 1),
                "torch_ops_us_median": round(sm, 1), "torch_ops_us_min": round(smin, 1), "speedup_at_median": round(sm / fm, 2),
                "loss_fused": out["fused"], "loss_torch_ops": out["stock"], "grad_max_dev_over_max": grad_dev,
                "reference_item_lookup_ms_one_segment": round(lookup_s * 1e3, 1),
                "timing": "call time, HIP events around the Python call, a synchronise after each, the two sides alternating; "
                          "the lookup: host clock around one segment's three list comprehensions, timed once, not part of either side",
                "fused_kernel_us_mean_of_10": kernels}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
