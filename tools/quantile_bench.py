"""Exact-quantile micro-benchmark, one JSON line per configuration (--out is rewritten): frl_hip/quantiles.py and strata.RecoveryCurves
(csrc/quantile.hip) against the same quantiles composed from stock torch ops on the same device in the same run.

  recovery   RecoveryCurves.add + table (its one host read included) over 16 x 15 x 256 x 256 observations, 20 and 200 EVT codes, mask
             densities 1.0 and 0.3: 8 ysfc bins x codes cells, q25 / q50 / q75 of predicted NBR and the median of observed NBR.  Baselines,
             both exact and both ending in the same host read: `sort`, a composite-key torch.sort per column (values, then a stable sort by
             cell) and a gather of the bracketing ranks; `cells`, a boolean mask per cell plus torch.quantile (timed at 20 codes only; at
             200 codes it is 1600 masks over 15.7 M observations).  The reference itself copies every pixel to the host and fills a
             reservoir in a Python loop per item.
  masked     masked_quantiles of q25 / q50 / q75 over 67 108 864 float32 gate values in [0, 1], a fifth of them saturated at exactly 0 or 1.
             Baselines: the reference's randperm + 2^23 subsample + 3 x torch.quantile (approximate), and a full torch.sort plus a
             gather (exact).
Per call: 3 warm-up calls, then the median / min of 10 (5 for the `cells` baseline), HIP events around each Python call and a device
synchronise after it, the sides alternating.  A second pass records the library's per-kernel event times.  Peak memory: the allocator's
peak during one call above what was allocated before it.
Usage: python tools/quantile_bench.py [--out profiles/quantile_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip import ops  # noqa: E402
from frl_hip.quantiles import masked_quantiles  # noqa: E402
from frl_hip.strata import RECOVERY_YSFC_BINS, RecoveryCurves  # noqa: E402

DEV = "cuda:0"
B, T, H, W = 16, 15, 256, 256
QS = [0.25, 0.5, 0.75]
EDGES = [float(a) for a, _ in RECOVERY_YSFC_BINS] + [float(RECOVERY_YSFC_BINS[-1][1])]


def make(g, density, seed, dev=DEV, shape=(B, T, H, W)):
    b, t, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    vocab = torch.sort(torch.randperm(4 * g, generator=gen)[:g] + 1).values.to(torch.int32)
    small = torch.randint(0, g, (b, max(h // 32, 1), max(w // 32, 1)), generator=gen)               # blocks of 32 x 32 pixels: a vegetation map
    col = small.repeat_interleave(h // small.shape[1], 1).repeat_interleave(w // small.shape[2], 2)
    codes = vocab[col].to(torch.float32).to(dev)
    gd = torch.Generator(device=dev).manual_seed(seed)
    ysfc = torch.randint(0, 31, (b, t, h, w), generator=gd, device=dev).to(torch.float32)
    obs = torch.randn(b, t, h, w, generator=gd, device=dev) + 0.03 * ysfc
    pred = obs + 0.4 * torch.randn(b, t, h, w, generator=gd, device=dev)
    mask = torch.rand(b, t, h, w, generator=gd, device=dev) < density
    return vocab.to(dev), codes, ysfc, pred, obs, mask


# ---- the stock compositions ----------------------------------------------------------------------------------------------------------
def stock_cells(codes, ysfc, mask, vocab, max_ysfc):
    """-> (selected bool [B, T, H, W], cell int64 [B, T, H, W] = bin G + column)."""
    valid = torch.isfinite(codes) & (codes > 0)
    ci = torch.where(valid, codes, torch.zeros_like(codes)).to(torch.int32)
    col = torch.searchsorted(vocab, ci).clamp(max=vocab.numel() - 1)
    valid = valid & (vocab[col] == ci)
    keep = mask & (ysfc >= 0) & (ysfc <= max_ysfc) & (ysfc < EDGES[-1]) & valid.unsqueeze(1)
    idx = torch.bucketize(ysfc, torch.tensor(EDGES, dtype=torch.float32, device=ysfc.device), right=True) - 1
    return keep, idx.clamp(0, len(EDGES) - 2) * vocab.numel() + col.unsqueeze(1)


def _lerp(lo, hi, t):
    lo, hi = lo.double(), hi.double()
    return torch.where(t < 0.5, lo + (hi - lo) * t, hi - (hi - lo) * (1.0 - t))


def stock_sort(codes, ysfc, pred, obs, mask, vocab, max_ysfc=30.0):
    """Composite-key sort -> (count [C], quantiles float64 [C, 2, 3]) on the host."""
    keep, cell = stock_cells(codes, ysfc, mask, vocab, max_ysfc)
    c = cell[keep]
    ncell = (len(EDGES) - 1) * vocab.numel()
    count = torch.bincount(c, minlength=ncell)
    start = torch.cumsum(count, 0) - count
    v = (count - 1).clamp(min=0).double().unsqueeze(1) * torch.tensor(QS, dtype=torch.float64, device=c.device)
    k = v.floor().long()
    k1 = torch.minimum(k + 1, (count - 1).clamp(min=0).unsqueeze(1))
    out = []
    for x in (pred, obs):
        xs, i1 = torch.sort(x[keep])
        order = torch.sort(c[i1], stable=True).indices
        xs = torch.cat([xs[order], xs.new_zeros(1)])
        out.append(_lerp(xs[start.unsqueeze(1) + k], xs[start.unsqueeze(1) + k1], v - k))
    q = torch.where((count > 0).view(-1, 1, 1), torch.stack(out, 1), torch.full_like(out[0], float("nan")).unsqueeze(1))
    return count.cpu(), q.cpu()


def stock_per_cell(codes, ysfc, pred, obs, mask, vocab, max_ysfc=30.0):
    """A boolean mask per cell plus torch.quantile -> quantiles float64 [C, 2, 3] on the host."""
    keep, cell = stock_cells(codes, ysfc, mask, vocab, max_ysfc)
    c, p, o = cell[keep], pred[keep], obs[keep]
    ncell = (len(EDGES) - 1) * vocab.numel()
    qs = torch.tensor(QS, dtype=torch.float32, device=p.device)
    out = torch.full((ncell, 2, 3), float("nan"), dtype=torch.float64, device=p.device)
    for i in range(ncell):
        sel = c == i
        if bool(sel.any()):
            out[i, 0], out[i, 1] = torch.quantile(p[sel], qs).double(), torch.quantile(o[sel], qs).double()
    return out.cpu()


def stock_randperm(x):
    """compute_stats of the reference's step.py: a randperm subsample of 2^23, then three torch.quantile."""
    s = x[torch.randperm(len(x), device=x.device)[:2 ** 23]] if len(x) > 2 ** 23 else x
    return torch.stack([torch.quantile(s, 0.25), torch.quantile(s, 0.50), torch.quantile(s, 0.75)])


def stock_full_sort(x):
    xs = torch.sort(x).values
    v = torch.tensor(QS, dtype=torch.float64, device=x.device) * (len(x) - 1)
    k = v.floor().long()
    return _lerp(xs[k], xs[(k + 1).clamp(max=len(x) - 1)], v - k)


# ---- timing ----------------------------------------------------------------------------------------------------------------------
def timed(fns, n=10, warm=3):
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


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def kernel_times(fn):
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    kernels = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
    ops.kernel_timing(False)
    return kernels


TIMING = ("HIP events around the Python call, a synchronise after each, the sides alternating; 3 warm-up calls, median and min of 10 "
          "(5 for the per-cell baseline); kernel times: the library's event pairs, mean of 5 calls")


def put(line, name, med_min, peak=None):
    line[f"{name}_us_median"], line[f"{name}_us_min"] = med_min
    if peak is not None:
        line[f"{name}_peak_bytes"] = peak


def bench_recovery(g, density):
    vocab, codes, ysfc, pred, obs, mask = make(g, density, 5)
    codes_list = vocab.cpu().tolist()
    rc = RecoveryCurves(codes_list, capacity=B * T * H * W)

    def fused():
        rc.reset()
        rc.add(codes, ysfc, pred, obs, mask)
        return rc.table(codes_list)

    def sort():
        return stock_sort(codes, ysfc, pred, obs, mask, vocab)

    line = {"case": "recovery", "B": B, "T": T, "H": H, "W": W, "codes": g, "cells": 8 * g, "mask_density": density, "observations": B * T * H * W}
    f, s = timed([fused, sort])
    put(line, "fused", f, peak_bytes(fused))
    put(line, "torch_sort", s, peak_bytes(sort))
    line["fused_buffer_bytes"] = 12 * B * T * H * W
    best, which = s[0], "torch_sort"
    if g <= 20:
        def cells():
            return stock_per_cell(codes, ysfc, pred, obs, mask, vocab)
        c = timed([cells], n=5, warm=1)[0]
        put(line, "torch_per_cell", c, peak_bytes(cells))
        if c[0] < best:
            best, which = c[0], "torch_per_cell"
    line["baseline"], line["speedup_at_median"] = which, round(best / f[0], 2)
    table = fused()
    count, q = sort()
    line["records"] = int(count.sum())
    want = [(codes_list[i % g], i // g, int(count[i]), *[float(v) for v in (q[i, 0, 0], q[i, 0, 1], q[i, 0, 2], q[i, 1, 1])])
            for c0 in range(g) for i in range(c0, 8 * g, g) if count[i] > 0]
    got = [(r["evt_code"], rc.labels.index(r["ysfc_bin"]), r["n_samples"], r["pred_nbr_q25"], r["pred_nbr_median"], r["pred_nbr_q75"], r["obs_nbr_median"])
           for r in table]
    line["table_equal_to_torch_sort"] = got == want
    line["dropped"], line["nonfinite"] = rc.dropped_, rc.nonfinite_
    line["fused_kernel_us_mean_of_5"] = kernel_times(fused)
    line["timing"] = TIMING
    return line


def bench_masked():
    n = 1 << 26
    gd = torch.Generator(device=DEV).manual_seed(7)
    x = torch.rand(n, generator=gd, device=DEV)
    x = torch.where(x < 0.1, torch.zeros_like(x), torch.where(x > 0.9, torch.ones_like(x), x))       # saturated gates
    calls = {"fused": lambda: masked_quantiles(x, QS), "torch_randperm_3_quantile": lambda: stock_randperm(x), "torch_full_sort": lambda: stock_full_sort(x)}
    line = {"case": "masked", "N": n, "probabilities": QS}
    for (name, fn), t in zip(calls.items(), timed(list(calls.values()))):
        put(line, name, t, peak_bytes(fn))
    line["speedup_vs_randperm_at_median"] = round(line["torch_randperm_3_quantile_us_median"] / line["fused_us_median"], 2)
    line["speedup_vs_full_sort_at_median"] = round(line["torch_full_sort_us_median"] / line["fused_us_median"], 2)
    line["equal_to_full_sort"] = bool(torch.equal(calls["fused"](), calls["torch_full_sort"]()))
    line["randperm_max_abs_error"] = float((calls["torch_randperm_3_quantile"]().double() - calls["fused"]()).abs().max())
    line["input_bytes"] = 4 * n
    line["fused_GBps_of_input_at_median"] = round(4 * n / line["fused_us_median"] / 1e3, 1)
    line["fused_kernel_us_mean_of_5"] = kernel_times(calls["fused"])
    line["timing"] = TIMING
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for g in (20, 200):
        for density in (1.0, 0.3):
            lines.append(bench_recovery(g, density))
            print(json.dumps(lines[-1]), flush=True)
            torch.cuda.empty_cache()
    lines.append(bench_masked())
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:                                            # a run replaces the file: no stale lines
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
