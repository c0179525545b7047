"""Writes tests/golden/soft_nbr_{a..f}.npz and tests/golden/phase_nbr_a.npz by running the REFERENCE's soft_neighborhood_matching_loss
(frl/losses/soft_neighborhood.py:46-208) and phase_neighborhood_loss / build_phase_neighborhood_batch (frl/losses/phase_neighborhood.py),
importable where the reference tree is present (they need torch only).  The reference does not travel; only these arrays do.

soft_nbr_*: the seeded float32 inputs on a 2^-8 grid (tests/soft_neighborhood_cases.py draws them), the parameters, loss64 / the stats /
grad64 = d loss / d d_learned evaluated in float64, loss32 / grad32 from the same function in float32 on the CPU (how far the reference
itself sits from float64).  The cases built from points (b, c, f) also hold the points (ref_a, ref_b [B, M, C], emb_a, emb_b [B, M, D];
shared = 1 when role b is role a, the self-similarity layout), lengths, and loss64_points / grad64_emb_a / grad64_emb_b (with shared = 1
the whole gradient is in grad64_emb_a) from the same function on torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist") of the
points in float64: exact differences.  Their d_reference / d_learned are those distances rounded to float32 and zeroed where masked.

phase_nbr_a: spectral [N, T, C], phase [N, T, D], ysfc [N, T], pairs [B, 2], weights [B], the loss / stats / grad64 with respect to the
phase embeddings, and the reference batch: valid_pair_mask, M, mask_self, mask_cross and the four distance matrices on their unmasked
entries (d_*_self[mask_self], d_*_cross[mask_cross], row-major; masked entries never enter the loss).

    python tests/golden/make_soft_neighborhood_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl"))
sys.path.insert(0, os.path.dirname(HERE))
from losses.phase_neighborhood import build_phase_neighborhood_batch, phase_neighborhood_loss  # noqa: E402
from losses.soft_neighborhood import soft_neighborhood_matching_loss  # noqa: E402

import soft_neighborhood_cases as SC  # noqa: E402

NO_MM = "donot_use_mm_for_euclid_dist"


def matrix_case(b, m, seed, mask, **kw):
    d_ref, d_learned = SC.make_distances(b, m, seed)
    return dict(d_reference=d_ref, d_learned=d_learned, mask=mask, **kw)


def points_case(b, m, c, d, seed, lengths, exclude_diagonal, shared, scale=1.0, **kw):
    ref_a, emb_a = SC.make_points(b, m, c, seed, scale), SC.make_points(b, m, d, seed + 1, scale)
    ref_b = ref_a if shared else SC.make_points(b, m, c, seed + 2, scale)
    emb_b = emb_a if shared else SC.make_points(b, m, d, seed + 3, scale)
    return dict(ref_a=ref_a, ref_b=ref_b, emb_a=emb_a, emb_b=emb_b, shared=shared, lengths=lengths, exclude_diagonal=exclude_diagonal,
                mask=SC.length_mask(lengths, m, exclude_diagonal), **kw)


def case_e():
    mask = torch.zeros(6, 4, 4, dtype=torch.bool)
    mask[:, torch.arange(4), (torch.arange(4) + 1) % 4] = True          # one unmasked entry per row: every row below min_valid_per_row
    return matrix_case(6, 4, 205, mask, tau_ref=1.0, tau_learned=1.0, min_valid_per_row=2)


def cases():
    full = lambda b, m: torch.full((b,), m, dtype=torch.int64)  # noqa: E731
    return {
        "a": matrix_case(37, 5, 201, SC.length_mask(full(37, 5), 5, True), tau_ref=1.0, tau_learned=1.0, min_valid_per_row=2),
        "b": points_case(64, 15, 6, 12, 202, SC.make_lengths(64, 1, 15, 212), True, True, scale=0.1, tau_ref=0.1, tau_learned=0.1,
                         min_valid_per_row=2, pair_weights=SC.make_weights(64, 222, zero_at=5)),
        "c": points_case(50, 10, 6, 12, 203, SC.make_lengths(50, 1, 10, 213), False, False, tau_ref=1.0, tau_learned=1.0, min_valid_per_row=2,
                         pair_weights=SC.make_weights(50, 223)),
        "d": matrix_case(9, 33, 204, SC.make_random_mask(9, 33, 214, keep=0.5, lengths=SC.make_lengths(9, 2, 33, 224)), tau_ref=0.5,
                         tau_learned=0.25, min_valid_per_row=4),
        "e": case_e(),
        "f": points_case(16, 15, 6, 12, 206, full(16, 15), True, True, tau_ref=0.01, tau_learned=1.0, min_valid_per_row=2),
    }


def run_reference(case, d_ref, d_learned, dtype):
    kw = dict(tau_ref=case["tau_ref"], tau_learned=case["tau_learned"], min_valid_per_row=case["min_valid_per_row"],
              pair_weights=None if case.get("pair_weights") is None else case["pair_weights"].to(dtype))
    loss, stats = soft_neighborhood_matching_loss(d_ref, d_learned, case["mask"], **kw)
    loss.backward()
    return np.float64(float(loss.detach())), stats


def evaluate_matrices(case, dtype):
    d_learned = case["d_learned"].clone().to(dtype).requires_grad_(True)
    loss, stats = run_reference(case, case["d_reference"].to(dtype), d_learned, dtype)
    return loss, stats, (torch.zeros_like(d_learned) if d_learned.grad is None else d_learned.grad).numpy()


def evaluate_points(case, dtype=torch.float64):
    ea = case["emb_a"].clone().to(dtype).requires_grad_(True)
    eb = ea if case["shared"] else case["emb_b"].clone().to(dtype).requires_grad_(True)
    d_ref = torch.cdist(case["ref_a"].to(dtype), case["ref_b"].to(dtype), compute_mode=NO_MM)
    loss, _ = run_reference(case, d_ref, torch.cdist(ea, eb, compute_mode=NO_MM), dtype)
    zero = torch.zeros_like(ea)
    return loss, (zero if ea.grad is None else ea.grad).numpy(), (zero if case["shared"] or eb.grad is None else eb.grad).numpy()


def write_soft_nbr(name, case):
    if "emb_a" in case:
        # the matrix form of a points case: the float64 distances rounded to float32 (what a float32 caller holds), zero where masked
        for key, a, b in (("d_reference", "ref_a", "ref_b"), ("d_learned", "emb_a", "emb_b")):
            d = torch.cdist(case[a].double(), case[b].double(), compute_mode=NO_MM).float()
            case[key] = torch.where(case["mask"], d, torch.zeros_like(d))
    l64, stats, g64 = evaluate_matrices(case, torch.float64)
    l32, _, g32 = evaluate_matrices(case, torch.float32)
    arrays = {k: (v.numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in case.items() if v is not None}
    arrays.update(loss64=l64, grad64=g64, loss32=l32, grad32=g32)
    if "emb_a" in case:
        lp, ga, gb = evaluate_points(case)
        arrays.update(loss64_points=lp, grad64_emb_a=ga, grad64_emb_b=gb)
    for k, v in stats.items():
        arrays["stat_" + k] = np.float64(v)
    path = os.path.join(HERE, f"soft_nbr_{name}.npz")
    np.savez_compressed(path, **arrays)
    gmax = max(np.abs(g64).max(), 1e-30)
    print(name, tuple(case["mask"].shape), "loss64", l64, "rows", stats["n_rows_valid"], "active", stats["n_pairs_active"], "/", stats["n_pairs"],
          "f32 loss dev", abs(l32 - l64), "f32 grad dev / max", np.abs(g32 - g64).max() / gmax, "finite", bool(np.isfinite(g64).all()),
          os.path.getsize(path), "bytes")


def write_phase_nbr():
    n, t, c, d, b = 40, 15, 6, 12, 200
    g = torch.Generator().manual_seed(301)
    spectral, phase = SC.make_points(n, t, c, 302), SC.make_points(n, t, d, 303)
    ysfc = SC.make_ysfc(n, t, 304)
    pairs = torch.randint(0, n, (b, 2), generator=g, dtype=torch.int64)
    pairs[:20, 1] = pairs[:20, 0]                                        # (i, i) self-pairs: zero distances on the cross term's diagonal
    weights = SC.make_weights(b, 305)
    kw = dict(tau_ref=0.5, tau_learned=0.5, min_overlap=6, min_valid_per_row=2, self_similarity_weight=1.0, cross_pixel_weight=0.5)
    res = {}
    for dtype in (torch.float64, torch.float32):
        z = phase.clone().to(dtype).requires_grad_(True)
        loss, stats = phase_neighborhood_loss(spectral.to(dtype), z, ysfc, pairs, pair_weights=weights.to(dtype), **kw)
        loss.backward()
        res[dtype] = (float(loss.detach()), z.grad.numpy(), stats)
    batch = build_phase_neighborhood_batch(spectral.double(), phase.double(), ysfc, pairs, min_overlap=kw["min_overlap"])
    l64, g64, stats = res[torch.float64]
    l32, g32, _ = res[torch.float32]
    arrays = dict(spectral=spectral.numpy(), phase=phase.numpy(), ysfc=ysfc.numpy(), pairs=pairs.numpy(), weights=weights.numpy(),
                  loss64=np.float64(l64), grad64=g64, loss32=np.float64(l32), valid_pair_mask=batch["valid_pair_mask"].numpy(),
                  M=np.int64(batch["M"]), mask_self=batch["mask_self"].numpy(), mask_cross=batch["mask_cross"].numpy(),
                  **{k: np.float64(v) for k, v in kw.items()})
    for key, mk in (("d_ref_self", "mask_self"), ("d_learned_self", "mask_self"), ("d_ref_cross", "mask_cross"), ("d_learned_cross", "mask_cross")):
        arrays[key] = batch[key][batch[mk]].numpy()
    for k, v in stats.items():
        if not k.startswith("d_ref_"):                                  # the calibration keys are not produced by this package
            arrays["stat_" + k] = np.float64(v)
    path = os.path.join(HERE, "phase_nbr_a.npz")
    np.savez_compressed(path, **arrays)
    print("phase_nbr_a loss64", l64, "valid pairs", int(batch["valid_pair_mask"].sum()), "M", batch["M"], "f32 loss dev", abs(l32 - l64),
          "f32 grad dev / max", np.abs(g32 - g64).max() / np.abs(g64).max(), "finite", bool(np.isfinite(g64).all()), os.path.getsize(path), "bytes")


def main():
    for name, case in cases().items():
        write_soft_nbr(name, case)
    write_phase_nbr()


if __name__ == "__main__":
    main()
