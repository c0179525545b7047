"""Phase pair mining micro-benchmark, one JSON line per shape (appended to --out): the fused HIP path (losses.build_phase_pairs /
build_phase_pairs_batched, stats off) against the reference's formula composed from stock torch ops on the same device in the same run:
torch.cdist, the diagonal fill, topk, the [N, classes] float presence matrix (with the reference's host read of the largest ysfc value)
times its transpose, the two filters by boolean indexing, exp of the gathered distances, the self pairs, the concatenation.
Shapes are those of the reference's step: one sample of 964 anchors, and a batch of 16 samples of 360 anchors; C = 16, T = 15, k = 16,
ysfc ramps with resets.  For the batch the one batched call is timed against 16 single fused calls (shifted and concatenated) and against
16 stock compositions.  5 warm-up calls, then the median / min of 30 calls, HIP events around each Python call and a device synchronise
after it, the sides alternating.  A second pass records the library's per-kernel event times of the fused call.
Usage: python tools/phase_pairs_bench.py [--out profiles/phase_pairs_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import build_phase_pairs, build_phase_pairs_batched  # noqa: E402

DEV = "cuda:0"
K, MIN_OVERLAP, MIN_PAIRS, SIGMA = 16, 3, 5, 5.0


def ramps(n, t, g, reset=0.2):
    """Years-since-disturbance ramps with random resets, integer-valued float32 [N, T]."""
    y = torch.zeros(n, t)
    cur = torch.randint(0, 6, (n,), generator=g).float()
    for k in range(t):
        cur = torch.where(torch.rand(n, generator=g) < reset, torch.zeros(n), cur + (1.0 if k > 0 else 0.0))
        y[:, k] = cur
    return y


def stock_pairs(spec, ysfc, k=K, min_overlap=MIN_OVERLAP, min_pairs=MIN_PAIRS, sigma=SIGMA, self_pair_weight=1.0):
    n, dev = spec.shape[0], spec.device
    dist = torch.cdist(spec, spec)
    no_self = dist.clone()
    no_self.fill_diagonal_(float("inf"))
    kk = min(k, n - 1)
    knn = no_self.topk(kk, dim=1, largest=False).indices
    values = ysfc.long()
    presence = torch.zeros(n, int(values.max().item()) + 1, dtype=torch.float32, device=dev)
    presence.scatter_(1, values, 1.0)
    overlap = torch.gather(presence @ presence.T, 1, knn)
    passed = overlap >= min_overlap
    ok = passed.sum(dim=1) >= min_pairs
    keep = passed & ok.unsqueeze(1)
    rows = torch.arange(n, device=dev).unsqueeze(1).expand(-1, kk)
    cross = torch.stack([rows[keep], knn[keep]], dim=1)
    w = torch.exp(-torch.gather(dist, 1, knn)[keep] / sigma)
    survivors = ok.nonzero().squeeze(1)
    return (torch.cat([cross, survivors.unsqueeze(1).expand(-1, 2)], dim=0),
            torch.cat([w, torch.full((survivors.numel(),), self_pair_weight, device=dev)]))


def looped(fn, spec, ysfc, off):
    parts = [fn(spec[lo:hi], ysfc[lo:hi]) for lo, hi in zip(off[:-1], off[1:])]
    return torch.cat([p[0] + lo for p, lo in zip(parts, off[:-1])], dim=0), torch.cat([p[1] for p in parts])


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
    return [(round(sorted(t)[len(t) // 2], 1), round(min(t), 1)) for t in ts]


def agreement(got, want):
    """Pairs of the fused call against the stock composition's (whose cdist may take the matrix-multiply route and rank near-ties otherwise)."""
    same = got[0].shape == want[0].shape and bool((got[0] == want[0]).all())
    out = {"pairs_fused": int(got[0].shape[0]), "pairs_torch_ops": int(want[0].shape[0]), "pairs_equal": same}
    if same and got[0].shape[0]:
        out["weight_max_dev"] = float((got[1] - want[1]).abs().max())
    return out


def kernel_times(fn):
    from frl_hip import ops
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
    ops.kernel_timing(False)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    c, t, lines = 16, 15, []
    note = "call time, HIP events around the Python call (stats off), a synchronise after each, the sides alternating"

    g = torch.Generator().manual_seed(1)
    spec, ysfc = torch.randn(964, c, generator=g).to(DEV), ramps(964, t, g).to(DEV)
    fused = lambda: build_phase_pairs(spec, ysfc, K, MIN_OVERLAP, MIN_PAIRS, sigma=SIGMA, stats=False)[:2]  # noqa: E731
    stock = lambda: stock_pairs(spec, ysfc)  # noqa: E731
    (fm, fmin), (sm, smin) = timed([fused, stock])
    lines.append({"case": "single", "samples": 1, "anchors": 964, "C": c, "T": t, "k": K, "fused_us_median": fm, "fused_us_min": fmin,
                  "torch_ops_us_median": sm, "torch_ops_us_min": smin, "speedup_at_median": round(sm / fm, 2), **agreement(fused(), stock()),
                  "timing": note, "fused_kernel_us_mean_of_10": kernel_times(fused)})
    print(json.dumps(lines[-1]), flush=True)

    g = torch.Generator().manual_seed(16)
    n, off = 16 * 360, [360 * j for j in range(17)]
    spec, ysfc = torch.randn(n, c, generator=g).to(DEV), ramps(n, t, g).to(DEV)
    batched = lambda: build_phase_pairs_batched(spec, ysfc, off, K, MIN_OVERLAP, MIN_PAIRS, sigma=SIGMA, stats=False)[:2]  # noqa: E731
    singles = lambda: looped(lambda s, y: build_phase_pairs(s, y, K, MIN_OVERLAP, MIN_PAIRS, sigma=SIGMA, stats=False)[:2], spec, ysfc, off)  # noqa: E731
    stocks = lambda: looped(stock_pairs, spec, ysfc, off)  # noqa: E731
    (bm, bmin), (gm, gmin), (sm, smin) = timed([batched, singles, stocks])
    one, many = batched(), singles()
    lines.append({"case": "batch", "samples": 16, "anchors": 360, "C": c, "T": t, "k": K, "batched_us_median": bm, "batched_us_min": bmin,
                  "fused_16_calls_us_median": gm, "fused_16_calls_us_min": gmin, "torch_ops_16_calls_us_median": sm, "torch_ops_16_calls_us_min": smin,
                  "speedup_over_16_fused_calls": round(gm / bm, 2), "speedup_over_torch_ops": round(sm / bm, 2),
                  "batched_equals_16_calls": bool(torch.equal(one[0], many[0]) and torch.equal(one[1], many[1])), **agreement(one, stocks()),
                  "timing": note, "fused_kernel_us_mean_of_10": kernel_times(batched)})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
