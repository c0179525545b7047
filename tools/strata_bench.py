"""EVT-stratified diagnostics micro-benchmark, one JSON line per configuration (appended to --out): the contingency table and the
grouped moments of frl_hip/strata.py (csrc/strata.hip) against the same accumulation composed from stock torch ops on the same device in
the same run.

Workload: 16 x 256 x 256 pixels, 20 clusters, mask densities 1.0 and 0.3, vocabularies of 20 and 200 EVT codes, labels and codes either
spatially coherent (blocks of 32 x 32 pixels for the codes and 16 x 16 for the clusters: a vegetation map) or uniformly random.
  table      ContingencyTable.partial_fit (vocabulary given) against searchsorted + bincount.
  moments    GroupedMoments.partial_fit, observations mode, D = 12, T = 1 (FiLM gamma) against a boolean gather, a float64 cast and
             index_add_ into float64 sums.
  temporal   GroupedMoments.partial_fit, temporal mode, D = 12, T = 15 (z_phase) against mean / var over t, then the same.
The composition stays on the device and keeps its sums there; the reference itself moves every row to the host.  With 200 codes the
moments kernel runs twice (a window of the vocabulary holds 128 groups); both passes are inside the timed call.
Per call: 3 warm-up calls, then the median / min of 10, HIP events around each Python call and a device synchronise after it, the sides
alternating.  A second pass records the library's per-kernel event times.  Peak memory: the allocator's peak during one call above what
was allocated before it.
Usage: python tools/strata_bench.py [--out profiles/strata_bench.jsonl]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vq-vae_amd"))
from frl_hip import ops  # noqa: E402
from frl_hip.strata import ContingencyTable, GroupedMoments  # noqa: E402

DEV = "cuda:0"
B, H, W, R, D, T = 16, 256, 256, 20, 12, 15


def blocky(gen, n, block):
    small = torch.randint(0, n, (B, H // block, W // block), generator=gen)
    return small.repeat_interleave(block, 1).repeat_interleave(block, 2)


def make(g, density, coherent, seed):
    gen = torch.Generator().manual_seed(seed)
    vocab = torch.sort(torch.randperm(4 * g, generator=gen)[:g] + 1).values.to(torch.int32)
    col = blocky(gen, g, 32) if coherent else torch.randint(0, g, (B, H, W), generator=gen)
    lab = blocky(gen, R, 16) if coherent else torch.randint(0, R, (B, H, W), generator=gen)
    codes = vocab[col].to(torch.float32)                                         # the reference's evt_grid is float32
    mask = torch.rand(B, H, W, generator=gen) < density
    gd = torch.Generator(device=DEV).manual_seed(seed)
    gamma = torch.randn(B, H, W, D, generator=gd, device=DEV) + col.to(DEV).unsqueeze(-1) * 0.1
    z = torch.randn(B, T, H, W, D, generator=gd, device=DEV) * 0.3 + gamma.unsqueeze(1)
    return vocab.to(DEV), codes.to(DEV), lab.to(torch.int32).to(DEV), mask.to(DEV), gamma, z


# ---- the stock compositions ----------------------------------------------------------------------------------------------------------
def stock_columns(codes, mask, vocab):
    """-> (selected bool [B, H, W], column int64 [B, H, W]) of the valid codes the vocabulary holds."""
    valid = torch.isfinite(codes) & (codes > 0) & mask
    ci = torch.where(valid, codes, torch.zeros_like(codes)).to(torch.int32)
    col = torch.searchsorted(vocab, ci).clamp(max=vocab.numel() - 1)
    return valid & (vocab[col] == ci), col


def stock_table(lab, codes, mask, vocab, table):
    sel, col = stock_columns(codes, mask, vocab)
    sel = sel & (lab >= 0) & (lab < R)
    idx = lab.to(torch.int64) * vocab.numel() + col
    table += torch.bincount(idx[sel], minlength=table.numel()).view_as(table)


def stock_moments(x, codes, mask, vocab, pivot, n, s1, s2):
    sel, col = stock_columns(codes, mask, vocab)
    c = col[sel]
    y = (x[sel] - pivot).to(torch.float64)
    n += torch.bincount(c, minlength=n.numel())
    s1.index_add_(0, c, y)
    s2.index_add_(0, c, y * y)


def stock_temporal(z, codes, mask, vocab, pivot, n, s1, s2, sw):
    sel, col = stock_columns(codes, mask, vocab)
    c = col[sel]
    mu = (z.mean(dim=1)[sel] - pivot).to(torch.float64)
    w = z.var(dim=1, correction=0)[sel].to(torch.float64)
    n += torch.bincount(c, minlength=n.numel())
    s1.index_add_(0, c, mu)
    s2.index_add_(0, c, mu * mu)
    sw.index_add_(0, c, w)


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


TIMING = ("HIP events around the Python call, a synchronise after each, the sides alternating; 3 warm-up calls, median and min of 10; "
          "kernel times: the library's event pairs, mean of 5 calls")


def bench(g, density, coherent):
    vocab, codes, lab, mask, gamma, z = make(g, density, coherent, 5)
    codes_list = vocab.cpu().tolist()
    table = ContingencyTable(R, codes_list)
    st_table = torch.zeros(R, g, dtype=torch.int64, device=DEV)
    pivot = gamma[mask].mean(dim=0)
    mom = GroupedMoments(codes_list, D, pivot=pivot.cpu().numpy())
    tmp = GroupedMoments(codes_list, D, temporal=True, pivot=pivot.cpu().numpy())

    def zeros():
        return torch.zeros(g, dtype=torch.int64, device=DEV), *(torch.zeros(g, D, dtype=torch.float64, device=DEV) for _ in range(3))

    (n1, a1, a2, _), (n2, b1, b2, bw) = zeros(), zeros()
    calls = {
        "table": (lambda: table.partial_fit(lab, codes, mask), lambda: stock_table(lab, codes, mask, vocab, st_table)),
        "moments": (lambda: mom.partial_fit(gamma, codes, mask), lambda: stock_moments(gamma, codes, mask, vocab, pivot, n1, a1, a2)),
        "temporal": (lambda: tmp.partial_fit(z, codes, mask), lambda: stock_temporal(z, codes, mask, vocab, pivot, n2, b1, b2, bw)),
    }
    line = {"case": "strata", "B": B, "H": H, "W": W, "clusters": R, "codes": g, "mask_density": density, "labels": "blocks" if coherent else "random",
            "D": D, "T_temporal": T, "n_valid": int(mask.sum()), "moment_windows": -(-g // mom.window)}
    for name, (fused, stock) in calls.items():
        (f, fm), (s, sm) = timed([fused, stock])
        line.update({f"{name}_fused_us_median": f, f"{name}_fused_us_min": fm, f"{name}_torch_ops_us_median": s, f"{name}_torch_ops_us_min": sm,
                     f"{name}_speedup_at_median": round(s / f, 2), f"{name}_fused_peak_bytes": peak_bytes(fused),
                     f"{name}_torch_ops_peak_bytes": peak_bytes(stock)})
    # one call each on fresh state for the comparison of what they compute
    one = ContingencyTable(R, codes_list).partial_fit(lab, codes, mask)
    st_table.zero_()
    stock_table(lab, codes, mask, vocab, st_table)
    line["table_equal_to_torch_ops"] = bool((torch.from_numpy(one.table()[0]).to(DEV) == st_table).all())
    m1 = GroupedMoments(codes_list, D, temporal=True, pivot=pivot.cpu().numpy()).partial_fit(z, codes, mask)
    for t in (n2, b1, b2, bw):
        t.zero_()
    stock_temporal(z, codes, mask, vocab, pivot, n2, b1, b2, bw)
    line["temporal_count_equal"] = bool((torch.from_numpy(m1.count_).to(DEV) == n2).all())
    line["temporal_S1_max_dev_vs_torch_ops"] = float((torch.from_numpy(m1.pivoted()[1]).to(DEV) - b1).abs().max())
    line["temporal_SW_max_dev_vs_torch_ops"] = float((torch.from_numpy(m1.within_).to(DEV) - bw).abs().max())
    line["fused_kernel_us_mean_of_5"] = kernel_times(lambda: [c[0]() for c in calls.values()])
    line["timing"] = TIMING
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for g in (20, 200):
        for density in (1.0, 0.3):
            for coherent in (True, False):
                lines.append(bench(g, density, coherent))
                print(json.dumps(lines[-1]), flush=True)
                torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
