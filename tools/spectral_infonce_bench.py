"""Cross-patch spectral negatives micro-benchmark, one JSON line per shape (appended to --out): losses.cross_patch_negatives (one launch of
csrc/spectral_negatives.hip behind a torch.randint for the draws) against the reference's sequence of step.py:757-773 composed from stock
torch ops on the same device in the same run: two torch.randint per ordered patch pair, the concatenations, two row gathers, the norm of
the difference and the weight.
Shapes: 2 x 329, 16 x 329 and 16 x 964 anchors (patches x anchors per patch), C in {16, 64} spectral channels, 20 negatives per anchor.
Warm-up calls, then the median / min of the timed calls, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times of the fused call and counts its launches per call (1: the draws
are torch's); the rest of the call is host time and torch's own kernels.  One more line times losses.global_spectral_infonce forward and
backward (mutual-kNN positives, negatives, InfoNCE, the similarity statistics with their host read) at 16 x 329 anchors, C = 16, D = 64.
Usage: python tools/spectral_infonce_bench.py [--out profiles/spectral_infonce_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import cross_patch_negatives, global_spectral_infonce  # noqa: E402
from frl_hip.losses.spectral_infonce import negatives_per_patch_pair  # noqa: E402

DEV = "cuda:0"
NEG_PER_ANCHOR, TAU, MIN_W = 20, 1.0, 0.05


def stock_negatives(spec, offsets, n_per):
    """The reference's composition: -> (pairs [Q, 2], dist [Q], weights [Q])."""
    dev, s = spec.device, len(offsets) - 1
    left, right = [], []
    for pi in range(s):
        for pj in range(s):
            if pi != pj:
                left.append(torch.randint(offsets[pi], offsets[pi + 1], (n_per,), device=dev))
                right.append(torch.randint(offsets[pj], offsets[pj + 1], (n_per,), device=dev))
    i, j = torch.cat(left), torch.cat(right)
    dist = torch.norm(spec[i] - spec[j], dim=1)
    return torch.stack([i, j], dim=1), dist, (1.0 - torch.exp(-dist / TAU)).clamp(min=MIN_W, max=1.0)


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


def kernel_times(fn, calls=10):
    """-> ({kernel: mean us per launch}, library launches per call)."""
    from frl_hip import ops
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    report = ops.kernel_timing_report()
    ops.kernel_timing(False)
    return {k: round(v[1] / v[0] * 1e3, 1) for k, v in report.items()}, sum(v[0] for v in report.values()) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    note = "call time, HIP events around the Python call, a synchronise after each, the sides alternating"
    for s, per_patch, n, warm in ((2, 329, 30, 5), (16, 329, 20, 3), (16, 964, 20, 3)):
        offsets = [p * per_patch for p in range(s + 1)]
        for c in (16, 64):
            spec = torch.randn(s * per_patch, c, generator=torch.Generator().manual_seed(100 * s + c)).to(DEV)
            n_per = negatives_per_patch_pair(NEG_PER_ANCHOR, s * per_patch, s)
            one = lambda: cross_patch_negatives(spec, offsets, NEG_PER_ANCHOR, TAU, MIN_W)  # noqa: E731
            stock = lambda: stock_negatives(spec, offsets, n_per)  # noqa: E731
            (fm, fmin), (sm, smin) = timed([one, stock], n=n, warm=warm)
            got, want = one(), stock()
            kernels, launches = kernel_times(one)
            lines.append({"case": "cross_patch_negatives", "patches": s, "anchors_per_patch": per_patch, "C": c, "neg_per_anchor": NEG_PER_ANCHOR,
                          "n_per": n_per, "negatives": int(got["neg_pairs"].shape[0]), "negatives_torch_ops": int(want[0].shape[0]),
                          "torch_randint_calls": 2 * s * (s - 1), "fused_us_median": fm, "fused_us_min": fmin, "torch_ops_us_median": sm,
                          "torch_ops_us_min": smin, "speedup_at_median": round(sm / fm, 2),
                          "mean_weight_fused": round(float(got["neg_weights"].mean()), 4), "mean_weight_torch_ops": round(float(want[2].mean()), 4),
                          "timing": note, "fused_kernel_us_mean_of_10": kernels, "library_launches_per_call": launches})
            print(json.dumps(lines[-1]), flush=True)

    s, per_patch, c, d = 16, 329, 16, 64
    g = torch.Generator().manual_seed(7)
    offsets = [p * per_patch for p in range(s + 1)]
    spec = torch.randn(s * per_patch, c, generator=g).to(DEV)
    z = torch.randn(s * per_patch, d, generator=g).to(DEV).requires_grad_(True)
    coords = [torch.randint(0, 256, (per_patch, 2), generator=g).to(DEV) for _ in range(s)]
    info = {}

    def step():
        z.grad = None
        loss, out = global_spectral_infonce(z, spec, coords, offsets)
        loss.backward()
        info.update(n_pos=out["n_pos"], n_neg=out["n_neg"], loss=float(loss.detach()))

    ((m, mn),) = timed([step], n=20, warm=3)
    kernels, launches = kernel_times(step)
    lines.append({"case": "global_spectral_infonce_fwd_bwd", "patches": s, "anchors_per_patch": per_patch, "C": c, "D": d, "positive_k": 16,
                  "neg_per_anchor": NEG_PER_ANCHOR, "n_pos": info["n_pos"], "n_neg": info["n_neg"], "loss": round(info["loss"], 4),
                  "us_median": m, "us_min": mn, "timing": note, "kernel_us_mean_of_10": kernels, "library_launches_per_call": launches})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
