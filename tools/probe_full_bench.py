"""Micro-benchmark of the phase probe's "full" design, one JSON line per mask density (appended to --out): InteractionProbe.partial_fit,
solve and partial_evaluate of frl_hip/probe.py (csrc/probe_full.hip) against the reference's two passes composed from stock torch ops on
the same device in the same run.

  16 x 8 x 256 x 256 observations, z_type 64 + z_phase 12 columns, seven targets, halo 16, interaction_pca_k = 20, mask densities 1.0
  and 0.3 (fit_phase_linear_probe.py with its defaults).  The composition gathers the unmasked rows once per pass and walks them in
  chunks of --chunk rows so that the [chunk, 844] float64 design block fits: pass 1 sums x, x^2 and the 768 x 768 interaction outer
  product, pass 2 transforms every chunk with the stored float32 preprocessor and adds the normal equations; its evaluation is the
  transform, X @ W + b in float32 and the per-metric sums.  It is favoured where the reference is slower than it needs to be: it stays
  on the device (the reference moves every row to the CPU) and keeps its sums there.
Method of tools/probe_bench.py: HIP events around each Python call, a synchronise after each, the sides alternating, medians.  A second
pass records the library's per-kernel event times and its launches per call; the moment kernel's share of the FP32 matrix peak
(157.3 TFLOP/s) counts 2 * 256 * (blocks of Scq and of the upper triangle of Sqq) FLOP per staged observation, an observation being
staged when its tile of 64 pixels has an unmasked one.  Peak memory: the allocator's peak during one call above what was allocated
before it.
Usage: python tools/probe_full_bench.py [--out profiles/probe_full_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "vq-vae_amd"), HERE]
from frl_hip import ops  # noqa: E402
from frl_hip.probe import InteractionProbe, halo_mask  # noqa: E402
from probe_bench import DEV, LAM, make_phase, peak_bytes, stock_phase_rows, stock_solve, timed  # noqa: E402

F32_MATRIX_PEAK = 157.3e12
K = 20


def design(zt, zp):
    return torch.cat([zt, zp, (zt.unsqueeze(2) * zp.unsqueeze(1)).reshape(zt.shape[0], -1)], dim=1)


def stock_transform(zt, zp, pre):
    mean, std, comp = pre
    x = (design(zt, zp).double() - mean.double()) / std.double()
    dm = zt.shape[1] + zp.shape[1]
    return torch.cat([x[:, :dm], x[:, dm:] @ comp.double()], dim=1).float()


def stock_fit(zt, zp, y, m, halo, chunk):
    dt, dp = zt.shape[1], zp.shape[1]
    dm, dq = dt + dp, dt * dp
    # pass 1
    zt_flat, zp_flat, _ = stock_phase_rows(zt, zp, m, halo)
    n = zt_flat.shape[0]
    sx = torch.zeros(dm + dq, dtype=torch.float64, device=DEV)
    sx2, sxx = torch.zeros_like(sx), torch.zeros(dq, dq, dtype=torch.float64, device=DEV)
    for i in range(0, n, chunk):
        X = design(zt_flat[i:i + chunk], zp_flat[i:i + chunk]).to(torch.float64)
        sx += X.sum(0)
        sx2 += (X * X).sum(0)
        sxx += X[:, dm:].T @ X[:, dm:]
        del X
    mean = sx / n
    std = (sx2 / n - mean * mean).clamp(min=1e-16).sqrt()
    inv = 1.0 / std[dm:]
    vals, vecs = torch.linalg.eigh(inv.unsqueeze(1) * (sxx / n - torch.outer(mean[dm:], mean[dm:])) * inv.unsqueeze(0))
    comp = (vecs[:, -K:].flip(dims=[1]) / vals[-K:].flip(dims=[0]).clamp(min=1e-12).sqrt().unsqueeze(0)).float()
    pre = (mean.float(), std.float(), comp)
    del zt_flat, zp_flat
    # pass 2
    zt_flat, zp_flat, m_flat = stock_phase_rows(zt, zp, m, halo)
    c = y.shape[1]
    Y = y.permute(0, 2, 3, 4, 1).contiguous().reshape(-1, c)[m_flat]
    A = torch.zeros(dm + K + 1, dm + K + 1, dtype=torch.float64, device=DEV)
    B = torch.zeros(dm + K + 1, c, dtype=torch.float64, device=DEV)
    for i in range(0, n, chunk):
        X = stock_transform(zt_flat[i:i + chunk], zp_flat[i:i + chunk], pre)
        Xaug = torch.cat([X, torch.ones((X.shape[0], 1), dtype=X.dtype, device=DEV)], dim=1).to(torch.float64)
        A += Xaug.T @ Xaug
        B += Xaug.T @ Y[i:i + chunk].to(torch.float64)
    return stock_solve(A, B) + (pre,)


def stock_eval(zt, zp, y, m, halo, W, b, pre, chunk, sums, keep):
    zt_flat, zp_flat, m_flat = stock_phase_rows(zt, zp, m, halo)
    c = y.shape[1]
    Y = y.permute(0, 2, 3, 4, 1).contiguous().reshape(-1, c)[m_flat]
    for i in range(0, zt_flat.shape[0], chunk):
        P = stock_transform(zt_flat[i:i + chunk], zp_flat[i:i + chunk], pre) @ W + b
        for j in range(c):
            yt, pt = Y[i:i + chunk, j], P[:, j]
            err = pt - yt
            sums[j, 0] += (err * err).sum()
            sums[j, 1] += yt.sum()
            sums[j, 2] += (yt * yt).sum()
            keep.append((pt, yt))


def bench(b, t, h, w, dt, dp, cy, halo, density, chunk):
    zt, zp, y, m = make_phase(b, t, h, w, dt, dp, cy, 11)
    g0 = torch.Generator().manual_seed(5)
    m = (torch.rand(b, h, w, generator=g0) < density).to(DEV) if density < 1.0 else torch.ones_like(m)
    ycl = y.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)           # channels-last in memory: no copy inside the timed call
    state = {}

    def fused_fit():
        state["g"] = InteractionProbe(LAM, K).partial_fit((zt, zp), ycl, m, halo=halo)

    def st_fit():
        state["s"] = stock_fit(zt, zp, y, m, halo, chunk)

    (ff, ffm), (sf, sfm) = timed([fused_fit, st_fit], n=3, warm=1)
    g = state["g"]
    g.moments()
    (so, som), = timed([lambda: g.solve()], n=3, warm=1)                         # host float64 algebra; the events bracket an idle device
    W, bb = g.solve()
    Ws, bs, pre = state["s"]
    # what the two compute: predictions of a few thousand unmasked rows through either preprocessor
    zf, pf, _ = stock_phase_rows(zt, zp, m, halo)
    rows = torch.linspace(0, zf.shape[0] - 1, 4096, device=DEV).long()
    own = g.transform(zf[rows].cpu(), pf[rows].cpu()).double() @ W.double() + bb.double()
    ref = (stock_transform(zf[rows], pf[rows], pre).double() @ Ws.double() + bs.double()).cpu()
    del zf, pf
    ev, ev_norank = InteractionProbe(LAM, K), InteractionProbe(LAM, K)
    for e in (ev, ev_norank):
        e.set_model(W, bb, g.mean_, g.std_, g.pca_components_, d_type=dt, d_phase=dp, pivot=g.moments()[4])
    sums = torch.zeros(cy, 3, dtype=torch.float32, device=DEV)
    keep = []

    def fused_eval():
        ev._pairs.clear()
        ev.partial_evaluate((zt, zp), ycl, m, halo=halo)

    def fused_eval_norank():
        ev_norank.partial_evaluate((zt, zp), ycl, m, halo=halo, rank=False)

    def st_eval():
        keep.clear()
        stock_eval(zt, zp, y, m, halo, Ws, bs, pre, chunk, sums, keep)

    (fe, fem), (fn_, fnm), (se, sem) = timed([fused_eval, fused_eval_norank, st_eval], n=3, warm=1)
    ops.kernel_timing(True)
    ops.kernel_timing_report()
    for _ in range(3):
        fused_fit()
    torch.cuda.synchronize()
    rep = ops.kernel_timing_report()
    fit_kern = {k: round(v[1] / v[0] * 1e3, 1) for k, v in rep.items()}
    fit_launches = sum(v[0] for v in rep.values()) / 3
    for _ in range(3):
        fused_eval_norank()
    torch.cuda.synchronize()
    rep = ops.kernel_timing_report()
    ev_kern = {k: round(v[1] / v[0] * 1e3, 1) for k, v in rep.items()}
    ev_launches = sum(v[0] for v in rep.values()) / 3
    ops.kernel_timing(False)
    full = m & halo_mask(h, w, halo, m.device).unsqueeze(0)
    staged = int(full.reshape(b, -1, 64).any(-1).sum()) * 64 * t
    c1, dq = dt + dp + cy + 1, dt * dp
    qb = (dq + 15) // 16
    blocks = ((c1 + 15) // 16) * qb + qb * (qb + 1) // 2
    flop = 2.0 * 256 * blocks * staged
    acc_us = next((v for k, v in fit_kern.items() if "probe_full_acc_kernel" in k), None)
    return {"case": "probe_phase_full", "B": b, "T": t, "H": h, "W": w, "Dt": dt, "Dp": dp, "Cy": cy, "halo": halo, "interaction_pca_k": K,
            "mask_density": density, "n_valid": g.n_obs_, "staged_observations": staged, "torch_ops_chunk_rows": chunk,
            "fused_fit_us_median": ff, "fused_fit_us_min": ffm, "torch_ops_two_pass_us_median": sf, "torch_ops_two_pass_us_min": sfm,
            "fit_speedup_at_median": round(sf / ff, 2), "solve_host_us_median": so, "solve_host_us_min": som,
            "fused_eval_us_median": fe, "fused_eval_us_min": fem, "fused_eval_no_rank_us_median": fn_, "fused_eval_no_rank_us_min": fnm,
            "torch_ops_eval_us_median": se, "torch_ops_eval_us_min": sem, "eval_speedup_at_median": round(se / fe, 2),
            "fit_kernel_us_mean_of_3": fit_kern, "fit_library_launches_per_call": fit_launches,
            "eval_kernel_us_mean_of_3": ev_kern, "eval_library_launches_per_call": ev_launches,
            "moment_blocks_16x16": blocks, "moment_flop": flop, "moment_kernel_flop_per_s": None if not acc_us else round(flop / (acc_us * 1e-6), -9),
            "moment_kernel_share_of_f32_matrix_peak": None if not acc_us else round(flop / (acc_us * 1e-6) / F32_MATRIX_PEAK, 4),
            "f32_matrix_peak_flop_per_s": F32_MATRIX_PEAK, "pred_max_dev_vs_torch_ops": float((own - ref).abs().max()),
            "pred_max_abs": float(ref.abs().max()),
            "fused_fit_peak_bytes": peak_bytes(fused_fit), "torch_ops_two_pass_peak_bytes": peak_bytes(st_fit),
            "fused_eval_peak_bytes": peak_bytes(fused_eval), "fused_eval_no_rank_peak_bytes": peak_bytes(fused_eval_norank),
            "torch_ops_eval_peak_bytes": peak_bytes(st_eval),
            "timing": "HIP events around the Python call, a synchronise after each, the sides alternating; 1 warm-up call, median and min of 3; "
                      "kernel times: the library's event pairs, mean of 3 calls"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "probe_full_bench.jsonl"))
    ap.add_argument("--chunk", type=int, default=1 << 18)
    args = ap.parse_args()
    lines = []
    for density in (1.0, 0.3):
        lines.append(bench(16, 8, 256, 256, 64, 12, 7, 16, density, args.chunk))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
