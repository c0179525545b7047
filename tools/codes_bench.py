"""Code-map inference micro-benchmark (median / min of 30 runs, HIP events around the call), one JSON line per case:
  * VQVAE.encode_tiles at BASELINE configs[1] (256 tiles of 5x32x32x64, K = 512, bf16), without and with a K = 1024 phase codebook;
  * the decode gather (ops.decode_codes) for the type map at cfg2 and the phase map (B=256 T=5 32x32), bytes per second and the
    fraction of the 6.3 TB/s measured copy ceiling;
  * the phase chain (ops.tcn_chain_fwd) training launch (y1, y2, y3 kept) vs the inference variant.
Usage: python tools/codes_bench.py [--out profiles/codes_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip import ops  # noqa: E402
from frl_hip.models import VQVAE  # noqa: E402

DEV = "cuda:0"
CEIL = 6.3e12


def timed(fn, n=30, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    g = torch.Generator().manual_seed(0)
    tile = torch.randn(256, 5, 32, 32, 64, generator=g).to(torch.bfloat16).to(DEV)
    for pk in (0, 1024):
        torch.manual_seed(0)
        m = VQVAE(in_features=64, codebook_size=512, emb_dim=64, phase_codebook_size=pk, compute_dtype=torch.bfloat16).to(DEV)
        m.init_codebook_from_tiles(tile[:8])
        med, mn = timed(lambda: m.encode_tiles(tile))
        emit({"case": "encode_tiles", "tiles": 256, "K": 512, "phase_K": pk, "us_median": round(med, 1), "us_min": round(mn, 1)})
        if pk:
            enc = m.encode_tiles(tile)
            med, mn = timed(lambda: m.decode_codes(enc["idx"], enc["idx_phase"]))
            emit({"case": "decode_codes (tables + both gathers)", "us_median": round(med, 1), "us_min": round(mn, 1)})

    for name, p, k in (("type map, cfg2", 256 * 32 * 32, 512), ("phase map, B=256 T=5 32x32", 256 * 5 * 32 * 32, 1024)):
        table = torch.randn(k, 64, generator=g).to(torch.bfloat16).to(DEV)
        idx = torch.randint(0, k, (p,), generator=g, dtype=torch.int32).to(DEV)
        med, mn = timed(lambda: ops.decode_codes(idx, table))
        nbytes = p * (4 + 64 * 2)
        emit({"case": "decode_gather", "shape": name, "pixels": p, "K": k, "F": 64, "dtype": "bf16", "bytes": nbytes,
              "us_median": round(med, 2), "us_min": round(mn, 2), "TB/s_at_median": round(nbytes / med / 1e6, 3),
              "frac_of_6.3TB/s_at_median": round(nbytes / med / 1e6 / (CEIL / 1e12), 3),
              "floor_us": round(nbytes / CEIL * 1e6, 2)})

    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=512, emb_dim=64, compute_dtype=torch.bfloat16).to(DEV).eval()
    layers = list(m.phase_tcn.layers)
    blocks = [(l.conv.weight, l.conv.bias, l.norm.weight, l.norm.bias, l.gate.weight, l.gate.bias, l.dilation, l.norm.num_groups,
               l.needs_projection) for l in layers]
    hw, hb = m.phase_head.weight, m.phase_head.bias
    x = tile.reshape(256, 5, 32 * 32, 64).contiguous()
    assert ops.tcn_chain_supported(x, blocks, hw)
    with torch.no_grad():
        h_train = ops.tcn_chain_fwd(x, blocks, hw, hb)[3]
        h_inf = ops.tcn_chain_fwd(x, blocks, hw, hb, keep_intermediates=False)[3]
        same = bool(torch.equal(h_train, h_inf))
        for keep in (True, False):
            med, mn = timed(lambda: ops.tcn_chain_fwd(x, blocks, hw, hb, keep_intermediates=keep))
            emit({"case": "tcn_chain_fwd", "variant": "training (y1, y2, y3 kept)" if keep else "inference (h only)",
                  "pixels": 256 * 1024, "us_median": round(med, 1), "us_min": round(mn, 1), "h_bitwise_equal": same})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
