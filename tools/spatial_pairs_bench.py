"""Spatial pair mining micro-benchmark, one JSON line per shape (appended to --out): the fused HIP path (losses.build_spatial_pairs /
build_spatial_pairs_batched) against the block of the reference's step (step.py:325-401) composed from stock torch ops on the same device
in the same run: the offset grid with its argsort, the bounds and mask tests, boolean indexing; per anchor the float distances to every
valid pixel, a where and a randperm; torch.unique(dim=0, return_inverse=True); the gather at the unique coordinates and the two weights.
Shapes: 1 x 329, 1 x 964 and 16 x 329 anchors on 256 x 256 masks with about 10 % invalid pixels, C = 8, k = 4 within radius 8, 4 negatives
beyond 16 pixels.  For the batch the one batched call is timed against 16 single fused calls and against 16 stock compositions.
Warm-up calls, then the median / min of the timed calls, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times of the fused call.
Usage: python tools/spatial_pairs_bench.py [--out profiles/spatial_pairs_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import build_spatial_pairs, build_spatial_pairs_batched  # noqa: E402

DEV = "cuda:0"
H = W = 256
C, K, RADIUS, MIN_DIST, N_NEG, TAU, MIN_W = 8, 4, 8, 16.0, 4, 1.0, 0.05


def stock_block(anchors, mask, feat):
    """One sample with stock torch ops -> (unique_coords, pos_pairs, neg_pairs, pos_weights, neg_weights)."""
    dev, n = anchors.device, anchors.shape[0]
    span = torch.arange(-RADIUS, RADIUS + 1, device=dev)
    grid = torch.stack(torch.meshgrid(span, span, indexing="ij"), dim=-1).reshape(-1, 2)
    dist = grid.float().pow(2).sum(dim=1).sqrt()
    near = (dist > 0) & (dist <= RADIUS)
    grid = grid[near][torch.argsort(dist[near])[:K]]
    nbr = anchors.unsqueeze(1) + grid.unsqueeze(0)
    inside = (nbr[..., 0] >= 0) & (nbr[..., 0] < H) & (nbr[..., 1] >= 0) & (nbr[..., 1] < W)
    ok = (mask[nbr[..., 0].clamp(0, H - 1), nbr[..., 1].clamp(0, W - 1)] & inside).reshape(-1)
    pos_anchor = torch.arange(n, device=dev).repeat_interleave(grid.shape[0])[ok]
    pos_rc = nbr.reshape(-1, 2)[ok]
    valid = mask.nonzero()
    valid_f = valid.float()
    neg_anchor, neg_rc = [], []
    for i in range(n):                                                   # the reference's loop: [V] distances, a where, a randperm
        far = ((valid_f - anchors[i].float()).pow(2).sum(dim=1).sqrt() >= MIN_DIST).nonzero().squeeze(1)
        if far.numel() == 0:
            continue
        take = far[torch.randperm(far.numel(), device=dev)[:N_NEG]]
        neg_anchor.append(torch.full((take.numel(),), i, dtype=torch.long, device=dev))
        neg_rc.append(valid[take])
    neg_anchor, neg_rc = torch.cat(neg_anchor), torch.cat(neg_rc)
    unique, inverse = torch.unique(torch.cat([anchors, pos_rc, neg_rc]), dim=0, return_inverse=True)
    a2u = inverse[:n]
    pos_pairs = torch.stack([a2u[pos_anchor], inverse[n:n + pos_rc.shape[0]]], dim=1)
    neg_pairs = torch.stack([a2u[neg_anchor], inverse[n + pos_rc.shape[0]:]], dim=1)
    f = feat[:, unique[:, 0], unique[:, 1]].T
    dpos = (f[pos_pairs[:, 0]] - f[pos_pairs[:, 1]]).norm(dim=1)
    dneg = (f[neg_pairs[:, 0]] - f[neg_pairs[:, 1]]).norm(dim=1)
    return (unique, pos_pairs, neg_pairs, torch.exp(-dpos / TAU).clamp(MIN_W, 1.0), (1.0 - torch.exp(-dneg / TAU)).clamp(MIN_W, 1.0))


def fused_one(anchors, mask, feat):
    return build_spatial_pairs(anchors, mask, feat, k=K, max_radius=RADIUS, min_distance=MIN_DIST, n_per_anchor=N_NEG, tau=TAU, min_w=MIN_W)


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


def agreement(got, want):
    """The fused result against the stock one: the positives and the unique map must agree up to the negatives, which are drawn otherwise."""
    pos_got = got["unique_coords"][got["pos_pairs"]].reshape(-1, 4)
    pos_want = want[0][want[1]].reshape(-1, 4)
    same = pos_got.shape == pos_want.shape and bool((torch.unique(pos_got, dim=0) == torch.unique(pos_want, dim=0)).all())
    return {"pos_pairs": int(pos_got.shape[0]), "neg_pairs_fused": int(got["neg_pairs"].shape[0]), "neg_pairs_torch_ops": int(want[2].shape[0]),
            "positives_equal_as_sets": same}


def sample(n, g):
    mask = torch.rand(H, W, generator=g) >= 0.1
    valid = mask.nonzero()
    anchors = valid[torch.randperm(valid.shape[0], generator=g)[:n]]
    return anchors.to(DEV), mask.to(DEV), torch.randn(C, H, W, generator=g).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    note = "call time, HIP events around the Python call, a synchronise after each, the sides alternating"
    for n in (329, 964):
        anchors, mask, feat = sample(n, torch.Generator().manual_seed(n))
        fused = lambda: fused_one(anchors, mask, feat)  # noqa: E731
        stock = lambda: stock_block(anchors, mask, feat)  # noqa: E731
        (fm, fmin), (sm, smin) = timed([fused, stock], n=20, warm=3)
        lines.append({"case": "single", "samples": 1, "anchors": n, "H": H, "W": W, "C": C, "k": K, "n_per_anchor": N_NEG, "fused_us_median": fm,
                      "fused_us_min": fmin, "torch_ops_us_median": sm, "torch_ops_us_min": smin, "speedup_at_median": round(sm / fm, 2),
                      **agreement(fused(), stock()), "timing": note, "fused_kernel_us_mean_of_10": kernel_times(fused)})
        print(json.dumps(lines[-1]), flush=True)

    s, n = 16, 329
    g = torch.Generator().manual_seed(16)
    parts = [sample(n, g) for _ in range(s)]
    anchors_all, masks, feats = torch.cat([p[0] for p in parts]), torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts])
    off = [n * j for j in range(s + 1)]
    batched = lambda: build_spatial_pairs_batched(anchors_all, masks, feats, off, k=K, max_radius=RADIUS, min_distance=MIN_DIST,  # noqa: E731
                                                  n_per_anchor=N_NEG, tau=TAU, min_w=MIN_W)
    singles = lambda: [fused_one(*p) for p in parts]  # noqa: E731
    stocks = lambda: [stock_block(*p) for p in parts]  # noqa: E731
    (bm, bmin), (gm, gmin), (sm, smin) = timed([batched, singles, stocks], n=8, warm=2)
    one, many = batched(), stocks()
    lines.append({"case": "batch", "samples": s, "anchors": n, "H": H, "W": W, "C": C, "k": K, "n_per_anchor": N_NEG, "batched_us_median": bm,
                  "batched_us_min": bmin, "fused_16_calls_us_median": gm, "fused_16_calls_us_min": gmin, "torch_ops_16_calls_us_median": sm,
                  "torch_ops_16_calls_us_min": smin, "speedup_over_16_fused_calls": round(gm / bm, 2), "speedup_over_torch_ops": round(sm / bm, 2),
                  "pos_pairs": int(one["pos_pairs"].shape[0]), "pos_pairs_torch_ops": sum(int(m[1].shape[0]) for m in many),
                  "neg_pairs_fused": int(one["neg_pairs"].shape[0]), "neg_pairs_torch_ops": sum(int(m[2].shape[0]) for m in many),
                  "timing": note, "fused_kernel_us_mean_of_10": kernel_times(batched)})
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
