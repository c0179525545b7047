"""Anchor sampling micro-benchmark, one JSON line per shape (appended to --out): the fused HIP path (data.sample_anchors_batched, with
data.inverse_frequency_weights in front of it for the inverse-frequency case) against the reference's sequence composed from stock torch
ops on the same device in the same run, per sample: two randint().item() host reads for the jitter, arange / meshgrid / boolean indexing
for the grid, a where over the mask, randperm or multinomial over all valid pixels, and unique(return_inverse) + scatter_add_ for the
inverse-frequency weights.
Shapes: 1 and 16 samples of 256 x 256 with about 10 % invalid pixels, stride 16, border 16, jitter radius 4, 104 supplement points,
unweighted, weighted, and weighted by the inverse frequency of a 40-level channel; one line for 1 x 1024 x 1024, unweighted.
Warm-up calls, then the median / min of the timed calls, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times of the fused call; the rest of the call is host time and torch's
own kernels (the random inputs, the final compaction).
Usage: python tools/anchor_bench.py [--out profiles/anchor_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.data import inverse_frequency_weights, sample_anchors_batched  # noqa: E402

DEV = "cuda:0"
STRIDE, BORDER, RADIUS, N_SUP, LEVELS = 16, 16, 4, 104, 40


def stock_inverse_frequency(data, valid):
    keep = valid & data.isfinite()
    vals = data[keep]
    _, inverse = vals.unique(return_inverse=True)
    counts = torch.zeros(int(inverse.max()) + 1, device=data.device).scatter_add_(0, inverse, torch.ones_like(vals))
    out = torch.zeros_like(data)
    out[keep] = 1.0 / counts[inverse]
    return out


def stock_sample(mask, weights, levels):
    """One sample with stock torch ops -> anchors [N, 2]."""
    dev = mask.device
    h, w = mask.shape
    jr = torch.randint(-RADIUS, RADIUS + 1, (1,), device=dev).item()
    jc = torch.randint(-RADIUS, RADIUS + 1, (1,), device=dev).item()
    rows, cols = torch.arange(BORDER + jr, h - BORDER, STRIDE, device=dev), torch.arange(BORDER + jc, w - BORDER, STRIDE, device=dev)
    grid = torch.stack([g.reshape(-1) for g in torch.meshgrid(rows, cols, indexing="ij")], dim=1)
    grid = grid[mask[grid[:, 0], grid[:, 1]]]
    if levels is not None:
        weights = stock_inverse_frequency(levels, mask)
    valid = torch.where(mask.reshape(-1))[0]
    n = min(N_SUP, valid.numel())
    if weights is None:
        pick = valid[torch.randperm(valid.numel(), device=dev)[:n]]
    else:
        p = weights.reshape(-1)[valid].clamp(min=0.0)
        pick = valid[torch.multinomial(p / p.sum(), n, replacement=False)]
    return torch.cat([grid, torch.stack([pick // w, pick % w], dim=1)])


def fused(masks, weights, levels):
    if levels is not None:
        weights = inverse_frequency_weights(levels, masks)
    return sample_anchors_batched(masks, stride=STRIDE, border=BORDER, jitter_radius=RADIUS, supplement_n=N_SUP, weights=weights)


def timed(fns, n, warm):
    """fns: callables timed alternately -> [(median us, min us)] in their order."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[j].append(a.elapsed_time(b) * 1e3)
    return [(round(sorted(t)[len(t) // 2], 1), round(min(t), 1)) for t in ts]


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


def inputs(s, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    masks = (torch.rand(s, h, w, generator=g) >= 0.1).to(DEV)
    weights = torch.rand(s, h, w, generator=g).to(DEV)
    levels = torch.randint(0, LEVELS, (s, h, w), generator=g).float().to(DEV)
    return masks, weights, levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    note = "call time, HIP events around the Python call, a synchronise after each, the sides alternating"
    for s, h, w, kinds, n, warm in ((1, 256, 256, ("uniform", "weighted", "inverse_frequency"), 20, 3),
                                    (16, 256, 256, ("uniform", "weighted", "inverse_frequency"), 10, 2), (1, 1024, 1024, ("uniform",), 10, 2)):
        masks, weights, levels = inputs(s, h, w, 100 * s + h)
        for kind in kinds:
            wgt, lev = (weights if kind == "weighted" else None), (levels if kind == "inverse_frequency" else None)
            one = lambda: fused(masks, wgt, lev)  # noqa: E731
            stock = lambda: [stock_sample(masks[i], None if wgt is None else wgt[i], None if lev is None else lev[i]) for i in range(s)]  # noqa: E731
            (fm, fmin), (sm, smin) = timed([one, stock], n=n, warm=warm)
            got, want = one(), stock()
            kernels = kernel_times(one)
            lines.append({"case": kind, "samples": s, "H": h, "W": w, "stride": STRIDE, "border": BORDER, "jitter_radius": RADIUS,
                          "supplement_n": N_SUP, "fused_us_median": fm, "fused_us_min": fmin, "torch_ops_us_median": sm, "torch_ops_us_min": smin,
                          "speedup_at_median": round(sm / fm, 2), "anchors_fused": int(got["anchors"].shape[0]),
                          "anchors_torch_ops": sum(int(a.shape[0]) for a in want), "supplement_fused": sum(got["stats"]["n_supplement"]),
                          "timing": note, "fused_kernel_us_mean_of_10": kernels, "fused_kernels_us_sum": round(sum(kernels.values()), 1)})
            print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
