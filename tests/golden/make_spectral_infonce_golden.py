"""Writes tests/golden/spectral_infonce_{a,b,c,d}.npz: what the global spectral InfoNCE block of the REFERENCE's step
(frl/training/representation/step.py:721-809) gives for the seeded inputs of tests/spectral_infonce_cases.py.  The reference does not
travel; only these arrays do, and they hold expected outputs only (the inputs come from the seeds).

Per case: pos = the reference's pairs_mutual_knn_chunked on the float32 spectral rows; neg = the cross-patch pairs of the loop of
step.py:757-769 under the recorded draws (torch.randint's stream cannot be matched: the pick of a draw is the documented map of
tests/spectral_infonce_cases.py); neg_dist, neg_w = the inline formulas of :772-773 and loss, grad = the reference's contrastive_loss and
its autograd gradient with respect to z, all in float64; stats = pos_mean, pos_std, neg_mean, neg_std of :798-807 in float64.

The maker asserts what the tests rely on: the mutual-kNN list is the same in float32 and float64, the k + 1 nearest distances of every row
are at least 1e-5 apart (relative), the case's seed is the first of 0..31 with both, and each case shows what it is there for.

    python tests/golden/make_spectral_infonce_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl"))
from losses.contrastive import contrastive_loss  # noqa: E402
from losses.pairs import pairs_mutual_knn_chunked  # noqa: E402

import spectral_infonce_cases as SC  # noqa: E402

MIN_GAP = 1e-5


def knn_gap(spec, coords, offsets, k):
    """The smallest relative gap between consecutive distances among the k + 1 nearest admissible neighbours of any row (float64)."""
    x = torch.from_numpy(spec).double()
    d = torch.cdist(x, x)
    d.fill_diagonal_(float("inf"))
    for p, c in enumerate(coords):
        a, b = offsets[p], offsets[p + 1]
        sp = torch.cdist(torch.from_numpy(c).float(), torch.from_numpy(c).float())
        blk = d[a:b, a:b]
        blk[sp < SC.MIN_SPATIAL] = float("inf")
    near = torch.sort(d, dim=1).values[:, :k + 1]
    lo, hi = near[:, :-1], near[:, 1:]
    ok = torch.isfinite(hi)
    return float(((hi - lo) / hi)[ok].min()) if ok.any() else float("inf")


def positives(inp, k, dtype):
    coords = [torch.from_numpy(c) for c in inp["coords"]]
    return pairs_mutual_knn_chunked(torch.from_numpy(inp["spec"]).to(dtype), coords, inp["offsets"], k, pos_min_spatial=SC.MIN_SPATIAL,
                                    chunk_size=32)


def qualifies(name, seed):
    inp, k = SC.make_inputs(name, seed), SC.CASES[name]["k"]
    same = torch.equal(positives(inp, k, torch.float32), positives(inp, k, torch.float64))
    gap = knn_gap(inp["spec"], inp["coords"], inp["offsets"], k)
    return same and gap >= MIN_GAP, gap


def main():
    for name, case in SC.CASES.items():
        for seed in range(32):
            ok, gap = qualifies(name, seed)
            print(f"case {name} seed {seed}: gap {gap:.1e} {'passes' if ok else 'fails'}")
            if ok:
                break
        assert ok and seed == case["seed"], f"case {name}: the first qualifying seed is {seed}, the table says {case['seed']}"
        inp = SC.make_inputs(name)
        offsets, n_per = inp["offsets"], inp["n_per"]
        s, n = len(offsets) - 1, offsets[-1]
        pos = positives(inp, case["k"], torch.float32)
        assert pos.shape[0] > 0

        # step.py:757-769 under the recorded draws
        i_parts, j_parts, q = [], [], 0
        for pi in range(s):
            for pj in range(s):
                if pi == pj:
                    continue
                for _ in range(n_per):
                    i_parts.append(SC.pick(inp["draws"][q][0], offsets[pi], offsets[pi + 1]))
                    j_parts.append(SC.pick(inp["draws"][q][1], offsets[pj], offsets[pj + 1]))
                    q += 1
        neg_i, neg_j = torch.tensor(i_parts), torch.tensor(j_parts)
        neg = torch.stack([neg_i, neg_j], dim=1)
        assert n_per == max(1, case["neg_per_anchor"] * n // (s * (s - 1))) and neg.shape[0] == n_per * s * (s - 1)
        spec64 = torch.from_numpy(inp["spec"]).double()
        neg_dist = torch.norm(spec64[neg_i] - spec64[neg_j], dim=1)                                     # :772
        neg_w = (1.0 - torch.exp(-neg_dist / SC.TAU)).clamp(min=SC.MIN_W, max=1.0)                      # :773
        z = torch.from_numpy(inp["z"]).double().requires_grad_(True)
        loss = contrastive_loss(z, pos, neg, temperature=SC.TEMPERATURE, similarity="l2", neg_weights=neg_w)
        loss.backward()
        with torch.no_grad():                                                                          # :798-807
            d = z.shape[1]
            sp = -(z[pos[:, 0]] - z[pos[:, 1]]).pow(2).sum(1) / d
            sn = -(z[neg[:, 0]] - z[neg[:, 1]]).pow(2).sum(1) / d
            stats = [sp.mean().item(), sp.std().item(), sn.mean().item(), sn.std().item()]

        clamped = int((neg_w == SC.MIN_W).sum())
        if name == "b":
            assert n_per == 24 and 1 in case["patches"]
        if name == "c":
            assert clamped > 0, "no weight on the min_w clamp"
        if name == "d":
            assert n_per == 4
        path = os.path.join(HERE, f"spectral_infonce_{name}.npz")
        np.savez_compressed(path, pos=pos.numpy().astype(np.int32), neg=neg.numpy().astype(np.int32), neg_dist=neg_dist.numpy(),
                            neg_w=neg_w.numpy(), loss=np.float64(loss.item()), grad=z.grad.numpy(), stats=np.asarray(stats, dtype=np.float64))
        print(f"case {name}: seed {seed}, {pos.shape[0]} positives, {neg.shape[0]} negatives (n_per {n_per}), {clamped} weights on the clamp, "
              f"loss {loss.item():.4f}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
