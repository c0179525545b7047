"""Type-local baseline and phase-type leakage micro-benchmark, one JSON line per function and size (appended to --out): the fused HIP
call (losses.type_local_baseline; losses.phase_type_leakage_loss forward + backward) against the reference's lines composed from stock
torch ops on the same device in the same run:
  baseline: Z_k @ Z_k.T, fill_diagonal_(-inf), topk, spec.mean(1), the gathered mean, the subtraction (step.py:922-928);
  leakage:  the two centrings, h_c.T @ Z_c / (N - 1), pow(2).sum().sqrt() and autograd's backward to h (step.py:1015-1021).
Sizes: N = 964 (one sample), 5760 (16 x 360) and 15424 (16 x 964); K = 8, k = 20, T = 15, C = 16, P = 12, Dz = 64.
5 warm-up calls, then the median / min of 30 calls, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times of the fused call.  For the baseline the peak of
torch.cuda.max_memory_allocated over one call of each side is recorded, above what was allocated before the call.
Usage: python tools/type_phase_bench.py [--out profiles/type_phase_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import phase_type_leakage_loss, type_local_baseline  # noqa: E402

DEV = "cuda:0"
SIZES = (964, 5760, 15424)
RANK, K_NBRS, T, C, P, DZ = 8, 20, 15, 16, 12, 64


def stock_baseline(z_k, spec, k_nbrs=K_NBRS):
    sim = z_k @ z_k.T
    sim.fill_diagonal_(float("-inf"))
    idx = sim.topk(min(k_nbrs, sim.shape[0] - 1), dim=1).indices
    s_hat = spec.mean(dim=1)[idx].mean(dim=1)
    return spec - s_hat.unsqueeze(1), s_hat, idx


def stock_leakage(h, z):
    z_sg = z.detach()
    h_c = h - h.mean(0, keepdim=True)
    z_c = z_sg - z_sg.mean(0, keepdim=True)
    return (h_c.T @ z_c / max(h_c.shape[0] - 1, 1)).pow(2).sum().sqrt()


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


def peak_bytes(fn):
    """Peak device memory of one call above what was allocated before it (the outputs of the call included)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    note = "call time, HIP events around the Python call, a synchronise after each, the sides alternating"
    lines = []
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        z_type = torch.randn(n, DZ, generator=g).to(DEV)
        z_c = z_type - z_type.mean(0, keepdim=True)
        z_k = torch.pca_lowrank(z_c, q=RANK, center=False)[0].contiguous()
        spec = torch.randn(n, T, C, generator=g).to(DEV)
        fused = lambda: type_local_baseline(z_k, spec, K_NBRS, return_parts=True)  # noqa: E731
        stock = lambda: stock_baseline(z_k, spec)  # noqa: E731
        (fm, fmin), (sm, smin) = timed([fused, stock])
        got, want = fused(), stock()
        rows_equal = float((got[2] == want[2]).all(dim=1).float().mean())   # torch's matmul may round a near-tie the other way
        lines.append({"case": "type_local_baseline", "N": n, "K": RANK, "k": K_NBRS, "T": T, "C": C, "fused_us_median": fm, "fused_us_min": fmin,
                      "torch_ops_us_median": sm, "torch_ops_us_min": smin, "speedup_at_median": round(sm / fm, 2),
                      "fused_peak_bytes": peak_bytes(fused), "fused_workspace_bytes": n * C * 4, "torch_ops_peak_bytes": peak_bytes(stock),
                      "rows_with_equal_indices": rows_equal, "spec_demeaned_max_dev": float((got[0] - want[0]).abs().max()),
                      "timing": note, "fused_kernel_us_mean_of_10": kernel_times(fused)})
        print(json.dumps(lines[-1]), flush=True)

        h = (0.5 * z_type[:, :P] + torch.randn(n, P, generator=g).to(DEV)).requires_grad_(True)

        def fused_l():
            h.grad = None
            phase_type_leakage_loss(h, z_type).backward()
            return h.grad

        def stock_l():
            h.grad = None
            stock_leakage(h, z_type).backward()
            return h.grad

        (fm, fmin), (sm, smin) = timed([fused_l, stock_l])
        gf, gs = fused_l().clone(), stock_l().clone()
        lf, ls = float(phase_type_leakage_loss(h, z_type).detach()), float(stock_leakage(h, z_type).detach())
        lines.append({"case": "phase_type_leakage_loss fwd+bwd", "N": n, "P": P, "Dz": DZ, "fused_us_median": fm, "fused_us_min": fmin,
                      "torch_ops_us_median": sm, "torch_ops_us_min": smin, "speedup_at_median": round(sm / fm, 2), "loss_fused": lf,
                      "loss_torch_ops": ls, "grad_max_dev_over_max": float((gf - gs).abs().max() / gs.abs().max()), "timing": note,
                      "fused_kernel_us_mean_of_10": kernel_times(fused_l)})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
