"""Linear-probe micro-benchmark, one JSON line per shape (appended to --out): RidgeProbe.partial_fit and partial_evaluate of
frl_hip/probe.py (csrc/probe.hip) against the reference's data path composed from stock torch ops on the same device in the same run.

  static   16 x 256 x 256 pixels, D = 64, five targets, mask densities 1.0 and 0.3 (fit_linear_probe.py): per batch the composition
           makes the channels-last copies, gathers by the boolean mask, appends the ones column, casts to float64 and runs the two
           float64 matmuls; its evaluation is the einsum, the gathers and the per-metric sums.
  phase    16 x 8 x 256 x 256 observations, z_type 64 + z_phase 12 columns, seven targets, halo 16, the additive design
           (fit_phase_linear_probe.py): the composition runs the reference's two passes (statistics, then the standardised normal
           equations); the fused path is one pass.
The composition is favoured where the reference is slower than it needs to be: it stays on the device (the reference moves rows to the
CPU in the phase script), keeps its sums on the device (the reference reads three scalars per metric and batch) and keeps the
per-metric prediction lists on the device.  Latents are channels-first views of channels-last tensors, as this project's models
return them; targets are channels-first contiguous, as the feature builder returns them (the fused path makes its one channels-last
copy of them inside the timed call).
Per call: 3 warm-up calls, then the median / min of 10, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times; the accumulate kernel's rate is the bytes of every staged
row, B T P (D + Cy) 4, over its time, against an HBM peak of 8 TB/s (6.3 TB/s is what a copy achieves).  Peak memory: the allocator's
peak during one call above what was allocated before it.
Usage: python tools/probe_bench.py [--out profiles/probe_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip import ops  # noqa: E402
from frl_hip.probe import RidgeProbe, halo_mask  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12
LAM = 1e-3


def make_static(b, h, w, d, cy, density, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(b, h, w, d, generator=g) * (0.5 + 1.5 * torch.rand(d, generator=g))).to(DEV)
    y = (torch.randn(b, cy, h, w, generator=g)).to(DEV) + z[..., :cy].permute(0, 3, 1, 2)
    m = (torch.rand(b, h, w, generator=g) < density).to(DEV)
    return z.permute(0, 3, 1, 2), y.contiguous(), m


def make_phase(b, t, h, w, dt, dp, cy, seed):
    g = torch.Generator().manual_seed(seed)
    zt = torch.randn(b, h, w, dt, generator=g).to(DEV)
    zp = torch.randn(b, t, h, w, dp, generator=g).to(DEV)
    y = torch.randn(b, cy, t, h, w, generator=g).to(DEV) + zp[..., :cy].permute(0, 4, 1, 2, 3)
    m = (torch.rand(b, h, w, generator=g) < 0.8).to(DEV)
    return zt.permute(0, 3, 1, 2), zp.permute(0, 4, 1, 2, 3), y.contiguous(), m


# ---- the reference's composition -----------------------------------------------------------------------------------------------------
def stock_fit(z, y, m, A, B):
    d, t = z.shape[1], y.shape[1]
    z_perm = z.permute(0, 2, 3, 1).contiguous()
    y_perm = y.permute(0, 2, 3, 1).contiguous()
    m_flat = m.reshape(-1)
    X = z_perm.reshape(-1, d)[m_flat]
    Y = y_perm.reshape(-1, t)[m_flat]
    ones = torch.ones((X.shape[0], 1), device=X.device, dtype=X.dtype)
    Xaug = torch.cat([X, ones], dim=1).to(torch.float64)
    Y = Y.to(torch.float64)
    A += Xaug.T @ Xaug
    B += Xaug.T @ Y


def stock_solve(A, B):
    reg = torch.eye(A.shape[0], device=A.device, dtype=torch.float64) * LAM
    reg[-1, -1] = 0.0
    wb = torch.linalg.solve(A + reg, B)
    return wb[:-1].float(), wb[-1].float()


def stock_eval(z, y, m, W, b, sums, keep):
    t = y.shape[1]
    pred = torch.einsum("bdhw,dt->bthw", z, W) + b.view(1, -1, 1, 1)
    pred_perm = pred.permute(0, 2, 3, 1).contiguous()
    y_perm = y.permute(0, 2, 3, 1).contiguous()
    m_flat = m.reshape(-1)
    P = pred_perm.reshape(-1, t)[m_flat]
    Y = y_perm.reshape(-1, t)[m_flat]
    for i in range(t):
        yt, pt = Y[:, i], P[:, i]
        err = pt - yt
        sums[i, 0] += (err * err).sum()
        sums[i, 1] += yt.sum()
        sums[i, 2] += (yt * yt).sum()
        keep.append((pt, yt))


def stock_phase_rows(zt, zp, m, halo):
    b, dt, h, w = zt.shape
    t, dp = zp.shape[2], zp.shape[1]
    full = m & halo_mask(h, w, halo, m.device).unsqueeze(0)
    ztl = zt.permute(0, 2, 3, 1).contiguous()
    zpl = zp.permute(0, 2, 3, 4, 1).contiguous()
    m_flat = full.unsqueeze(1).expand(-1, t, -1, -1).reshape(-1)
    zt_flat = ztl.unsqueeze(1).expand(-1, t, -1, -1, -1).reshape(-1, dt)[m_flat]
    zp_flat = zpl.reshape(-1, dp)[m_flat]
    return zt_flat, zp_flat, m_flat


def stock_phase_fit(zt, zp, y, m, halo):
    # pass 1
    zt_flat, zp_flat, _ = stock_phase_rows(zt, zp, m, halo)
    X_raw = torch.cat([zt_flat, zp_flat], dim=1).to(torch.float64)
    n = X_raw.shape[0]
    mean = X_raw.sum(0) / n
    std = ((X_raw * X_raw).sum(0) / n - mean * mean).clamp(min=1e-16).sqrt()
    mean, std = mean.float(), std.float()
    del X_raw
    # pass 2
    zt_flat, zp_flat, m_flat = stock_phase_rows(zt, zp, m, halo)
    c = y.shape[1]
    Y = y.permute(0, 2, 3, 4, 1).contiguous().reshape(-1, c)[m_flat]
    X = ((torch.cat([zt_flat, zp_flat], dim=1).double() - mean.double()) / std.double()).float()
    Xaug = torch.cat([X, torch.ones((X.shape[0], 1), dtype=X.dtype, device=X.device)], dim=1).to(torch.float64)
    Y64 = Y.to(torch.float64)
    return stock_solve(Xaug.T @ Xaug, Xaug.T @ Y64) + (mean, std)


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


def rate(kern, name, nbytes):
    us = next((v for k, v in kern.items() if name in k), None)
    if not us:
        return None, None
    return round(nbytes / (us * 1e-6), -9), round(nbytes / (us * 1e-6) / HBM_PEAK, 4)


TIMING = ("HIP events around the Python call, a synchronise after each, the sides alternating; 3 warm-up calls, median and min of 10; "
          "kernel times: the library's event pairs, mean of 5 calls")


def bench_static(b, h, w, d, cy, density):
    z, y, m = make_static(b, h, w, d, cy, density, 7)
    A = torch.zeros(d + 1, d + 1, dtype=torch.float64, device=DEV)
    B = torch.zeros(d + 1, cy, dtype=torch.float64, device=DEV)
    probe = RidgeProbe(LAM)

    def fused_fit():
        probe.partial_fit(z, y, m)

    def st_fit():
        stock_fit(z, y, m, A, B)

    (ff, ffm), (sf, sfm) = timed([fused_fit, st_fit])
    # one batch each for the comparison of what they compute
    one = RidgeProbe(LAM).partial_fit(z, y, m)
    W, bb = one.solve()
    A.zero_(), B.zero_()
    st_fit()
    Ws, bs = stock_solve(A, B)
    dev_w = float((W.to(DEV) - Ws).abs().max())
    ev = RidgeProbe(LAM).set_model(W, bb, pivot=one.moments()[2])
    ev_norank = RidgeProbe(LAM).set_model(W, bb, pivot=one.moments()[2])
    Wd, bd = W.to(DEV), bb.to(DEV)
    sums = torch.zeros(cy, 3, dtype=torch.float32, device=DEV)
    keep = []

    def fused_eval():
        ev._pairs.clear()
        ev.partial_evaluate(z, y, m)

    def fused_eval_norank():
        ev_norank.partial_evaluate(z, y, m, rank=False)

    def st_eval():
        keep.clear()
        stock_eval(z, y, m, Wd, bd, sums, keep)

    (fe, fem), (fn_, fnm), (se, sem) = timed([fused_eval, fused_eval_norank, st_eval])
    kern = kernel_times(lambda: (fused_fit(), fused_eval_norank()))
    nbytes = b * h * w * (d + cy) * 4
    acc_rate, acc_frac = rate(kern, "probe_acc_kernel", nbytes)
    ev_rate, ev_frac = rate(kern, "probe_eval_kernel", nbytes)
    line = {"case": "probe_static", "B": b, "H": h, "W": w, "D": d, "Cy": cy, "mask_density": density, "n_valid": int(m.sum()),
            "fused_fit_us_median": ff, "fused_fit_us_min": ffm, "torch_ops_fit_us_median": sf, "torch_ops_fit_us_min": sfm,
            "fit_speedup_at_median": round(sf / ff, 2),
            "fused_eval_us_median": fe, "fused_eval_us_min": fem, "fused_eval_no_rank_us_median": fn_, "fused_eval_no_rank_us_min": fnm,
            "torch_ops_eval_us_median": se, "torch_ops_eval_us_min": sem, "eval_speedup_at_median": round(se / fe, 2),
            "fused_kernel_us_mean_of_5": kern, "staged_bytes": nbytes, "acc_kernel_bytes_per_s": acc_rate, "acc_kernel_fraction_of_hbm_peak": acc_frac,
            "eval_kernel_bytes_per_s": ev_rate, "eval_kernel_fraction_of_hbm_peak": ev_frac, "hbm_peak_bytes_per_s": HBM_PEAK,
            "W_max_dev_vs_torch_ops": dev_w,
            "fused_fit_peak_bytes": peak_bytes(fused_fit), "torch_ops_fit_peak_bytes": peak_bytes(st_fit),
            "fused_eval_peak_bytes": peak_bytes(fused_eval), "torch_ops_eval_peak_bytes": peak_bytes(st_eval), "timing": TIMING}
    return line


def bench_phase(b, t, h, w, dt, dp, cy, halo):
    zt, zp, y, m = make_phase(b, t, h, w, dt, dp, cy, 11)
    ycl = y.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)           # the same targets, already channels-last in memory

    def fused():
        return RidgeProbe(LAM, standardize=True).partial_fit((zt, zp), y, m, halo=halo)

    def fused_cl():
        return RidgeProbe(LAM, standardize=True).partial_fit((zt, zp), ycl, m, halo=halo)

    def stock():
        return stock_phase_fit(zt, zp, y, m, halo)

    (ff, ffm), (fc, fcm), (sf, sfm) = timed([fused, fused_cl, stock], n=5, warm=2)
    g = fused()
    W, bb = g.solve()
    Ws, bs, mean, std = stock()
    kern = kernel_times(fused_cl)
    n_obs = b * t * h * w
    nbytes = n_obs * (dt + dp + cy) * 4
    acc_rate, acc_frac = rate(kern, "probe_acc_kernel", nbytes)
    return {"case": "probe_phase_additive", "B": b, "T": t, "H": h, "W": w, "D": dt + dp, "Cy": cy, "halo": halo, "n_valid": g.n_obs_,
            "fused_fit_us_median": ff, "fused_fit_us_min": ffm, "fused_fit_channels_last_targets_us_median": fc,
            "fused_fit_channels_last_targets_us_min": fcm, "torch_ops_two_pass_us_median": sf, "torch_ops_two_pass_us_min": sfm,
            "fit_speedup_at_median": round(sf / ff, 2), "fused_kernel_us_mean_of_5": kern, "staged_bytes": nbytes,
            "unique_bytes": (b * h * w * dt + n_obs * (dp + cy)) * 4,
            "acc_kernel_bytes_per_s": acc_rate, "acc_kernel_fraction_of_hbm_peak": acc_frac, "hbm_peak_bytes_per_s": HBM_PEAK,
            "W_max_dev_vs_torch_ops": float((W.to(DEV) - Ws).abs().max()), "std_max_dev_vs_torch_ops": float((g.std_.to(DEV) - std).abs().max()),
            "fused_fit_peak_bytes": peak_bytes(fused), "fused_fit_channels_last_targets_peak_bytes": peak_bytes(fused_cl),
            "torch_ops_two_pass_peak_bytes": peak_bytes(stock),
            "timing": TIMING.replace("3 warm-up calls, median and min of 10", "2 warm-up calls, median and min of 5")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for density in (1.0, 0.3):
        lines.append(bench_static(16, 256, 256, 64, 5, density))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    lines.append(bench_phase(16, 8, 256, 256, 64, 12, 7, 16))
    print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
