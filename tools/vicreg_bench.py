"""VICReg variance-covariance loss micro-benchmark, one JSON line per case (appended to --out):
  * forward + backward of the fused HIP path (losses.variance_covariance_loss) at [262144, 64] bf16 and f32 and [1310720, 12] bf16
    (z_type and z_phase rows of the bench.py workload), against the same formula written with stock torch ops (what the reference
    executes), on the same device in the same run: 5 warm-up calls, then the median / min of 30 calls, HIP events around each call, the two
    sides alternating.  Every call takes the next of a ring of input buffers whose total exceeds twice the 256 MB last-level cache, so
    the rows come from HBM as they do in a train step.  The times are call times (HIP events around the Python call, a device
    synchronise after each): they include the launch gaps of either side -- 4 launches + a 3-scalar stack on the fused side, about
    twenty on the stock side.  A second pass with the library's per-kernel event timing gives the kernels' own times and the
    bytes / s and FLOP / s the moments and backward kernels reach;
  * ms/step of the bench.py workload (256 tiles of 5x32x32x64, K = 512, bf16, graph-captured step) with lambda_vcr = 0.1 against
    lambda_vcr = 0, interleaved repeats, for information.
Usage: python tools/vicreg_bench.py [--out profiles/vicreg_bench.jsonl] [--no-step]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip.losses import variance_covariance_loss  # noqa: E402

DEV = "cuda:0"


def torch_formula(x, vw=1.0, cw=1.0, target=1.0, eps=1e-4):
    n, d = x.shape
    xc = x - x.mean(dim=0, keepdim=True)
    std = torch.sqrt(xc.var(dim=0) + eps)
    vl = torch.relu(target - std).mean()
    cov = (xc.T @ xc) / (n - 1)
    off = cov.clone()
    off.fill_diagonal_(0.0)
    cl = (off ** 2).sum() / d
    return vw * vl + cw * cl, vl, cl


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


def step_cost(emit):
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer
    g = torch.Generator().manual_seed(0)
    tiles = [torch.randn(256, 5, 32, 32, 64, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2)]
    trainers = {}
    for lam in (0.0, 0.1):
        torch.manual_seed(0)
        m = VQVAE(in_features=64, codebook_size=512, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
                  compute_dtype=torch.bfloat16, lambda_vcr=lam).to(DEV)
        m.init_codebook_from_tiles(tiles[0], seed=7)
        tr = VQVAETrainer(m, lr=1e-4, total_steps=10000)
        for i in range(6):                                   # captures (one per buffer) + warm-up
            tr.step_graphed(tiles[i % 2])
        trainers[lam] = tr
    ms = {0.0: [], 0.1: []}
    for _ in range(5):                                       # interleaved repeats of 10 steps
        for lam, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(10):
                tr.step_graphed(tiles[i % 2])
            torch.cuda.synchronize()
            ms[lam].append((time.perf_counter() - t0) * 100.0)
    med = {lam: sorted(v)[len(v) // 2] for lam, v in ms.items()}
    emit({"case": "train_step", "workload": "256 tiles 5x32x32x64, K=512, bf16, graphed step", "ms_per_step_lambda_vcr_0": round(med[0.0], 3),
          "ms_per_step_lambda_vcr_0.1": round(med[0.1], 3), "added_ms": round(med[0.1] - med[0.0], 3),
          "added_percent": round(100.0 * (med[0.1] / med[0.0] - 1.0), 2), "repeats": 5, "steps_per_repeat": 10})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    from frl_hip import ops
    g = torch.Generator().manual_seed(0)
    for n, d, dt in ((262144, 64, torch.bfloat16), (262144, 64, torch.float32), (1310720, 12, torch.bfloat16)):
        nbytes = n * d * (2 if dt == torch.bfloat16 else 4)
        ring = [(torch.randn(n, d, generator=g) * 0.7 + 0.3).to(dt).to(DEV).requires_grad_(True) for _ in range(-(-(512 << 20) // nbytes))]
        turn = [0]

        def run(fn):
            x = ring[turn[0] % len(ring)]
            turn[0] += 1
            x.grad = None
            fn(x)[0].backward()

        fused, stock = timed([lambda: run(variance_covariance_loss), lambda: run(torch_formula)])
        ops.kernel_timing(True)
        ops.kernel_timing_report()
        for _ in range(20):
            run(variance_covariance_loss)
        torch.cuda.synchronize()
        rep = {k: round(v[1] / v[0] * 1e3, 1) for k, v in ops.kernel_timing_report().items()}
        ops.kernel_timing(False)
        dp = -(-d // 16) * 16
        mom = next((v for k, v in rep.items() if "moments" in k), None)
        bwd = next((v for k, v in rep.items() if "bwd" in k), None)
        emit({"case": "vicreg_fwd_bwd", "N": n, "D": d, "dtype": str(dt).replace("torch.", ""), "input_ring_buffers": len(ring),
              "fused_us_median": round(fused[0], 1), "fused_us_min": round(fused[1], 1), "torch_ops_us_median": round(stock[0], 1),
              "torch_ops_us_min": round(stock[1], 1), "speedup_at_median": round(stock[0] / fused[0], 2),
              "timing": "call time, HIP events around the Python call, inputs rotate through a ring larger than the last-level cache",
              "fused_kernel_us_mean_of_20": rep,
              "moments_TB/s": None if not mom else round(nbytes / mom / 1e6, 2),
              "moments_mfma_TFLOP/s_padded": None if not mom else round(2.0 * n * dp * (dp + 16) / mom / 1e6, 1),
              "bwd_TB/s": None if not bwd else round(2 * nbytes / bwd / 1e6, 2)})
        del ring
        torch.cuda.empty_cache()
    if not args.no_step:
        step_cost(emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
