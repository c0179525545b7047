"""Writes tests/golden/recovery_disc_{a..e}.npz and tests/golden/spread_rank_{a..e}.npz by running the REFERENCE's
phase_recovery_discrimination_loss (frl/losses/triplet_phase.py:352-426) and compute_phase_spread_ranking on the batch of
build_phase_neighborhood_batch (frl/losses/phase_neighborhood.py:268-451, 637-740) in float64, torch.cdist held on the exact-difference
route.  The reference does not travel; only these arrays do.  Inputs come from the seeded makers of tests/soft_neighborhood_cases.py and
tests/phase_margin_cases.py (points and dynamism on the 2^-8 grid, ysfc ramps with resets).

recovery_disc_*: z [N, T, D] float32, ysfc [N, T] float32 (NaN / -1 planted), margin, low_ysfc_max, high_ysfc_min, loss64, stat_n_pairs,
stat_n_active_pixels, and grad64 = d loss / d z of the pixels grad_pixels (all of them in a and d; every 4th in b, every 8th in c and every 16th plus the
last in e, whose full gradients would be up to a megabyte each: the float64 restatement, pinned to these rows at 1e-12, stands in for the rest).

spread_rank_*: phase [N, T, D] float32, ysfc, pairs [B, 2], dynamism [N], min_overlap, margin, delta, loss64, the seven stat_* values,
grad64 = d loss / d phase; and the reference batch: valid_pair_mask, M, lengths, mask_self, d_self_i / d_self_j = the two float64 blocks
on the unmasked entries (row-major), grad64_pair = d loss / d d_learned_self on the unmasked entries of each pair (the maker asserts it is
one value per pair there, zero elsewhere, and that d loss / d d_learned_self_j is its negative).

Each case asserts the property it is there for, so a reseed cannot quietly empty it.

    python tests/golden/make_phase_margin_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl"))
sys.path.insert(0, os.path.dirname(HERE))
from losses.phase_neighborhood import build_phase_neighborhood_batch, compute_phase_spread_ranking  # noqa: E402
from losses.triplet_phase import phase_recovery_discrimination_loss  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "vq-vae_amd"))
from frl_hip.losses.soft_neighborhood import phase_alignment  # noqa: E402

import phase_margin_cases as PC  # noqa: E402
import soft_neighborhood_cases as SC  # noqa: E402

_cdist = torch.cdist
torch.cdist = lambda a, b, *args, **kw: _cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist")   # exact differences at any size


# ---------------------------------------------------------------------------------------------------------------------------
# recovery discrimination
# ---------------------------------------------------------------------------------------------------------------------------
def recovery_cases():
    def case(n, t, d, seed, scale, nan_frac=0.0, neg_frac=0.0, low=1.0, high=5.0, every=1):
        return dict(z=SC.make_points(n, t, d, seed, scale), ysfc=PC.plant_invalid(SC.make_ysfc(n, t, seed + 1), seed + 2, nan_frac, neg_frac),
                    margin=0.5, low_ysfc_max=low, high_ysfc_min=high, every=every)

    cases = {"a": case(37, 5, 12, 401, 1.0, 0.10, 0.05), "b": case(203, 15, 12, 411, 0.1, every=4), "c": case(64, 32, 64, 421, 0.05, low=3.0, high=3.0, every=8),
             "d": case(16, 5, 12, 431, 1.0), "e": case(1031, 15, 12, 441, 1.0, 0.20, every=16)}
    y = cases["d"]["ysfc"]                                               # every pixel lacks one class: the even ones keep no ysfc >= 5, the odd ones none <= 1
    y[0::2] = torch.clamp(y[0::2], max=4.0)
    y[1::2] = torch.clamp(y[1::2], min=2.0)
    return cases


def write_recovery(name, case):
    z = case["z"].double().requires_grad_(True)
    kw = dict(margin=case["margin"], low_ysfc_max=case["low_ysfc_max"], high_ysfc_min=case["high_ysfc_min"])
    loss, stats = phase_recovery_discrimination_loss(z, case["ysfc"].double(), **kw)
    if stats["n_pairs"] > 0:
        loss.backward()
    g64 = (torch.zeros_like(z) if z.grad is None else z.grad).numpy()
    n = z.shape[0]
    low, high = PC.recovery_classes(case["ysfc"], case["low_ysfc_max"], case["high_ysfc_min"])
    if name == "a":
        assert 0 < stats["n_active_pixels"] < n // 2 and np.isnan(case["ysfc"].numpy()).any() and (case["ysfc"] == -1).any()
    if name in ("b", "e"):
        assert stats["n_active_pixels"] > n // 2 and n % 4 != 0
    if name == "c":
        assert bool((low & high).any()), "no timestep in both classes: no (t, t) pair"
    if name == "d":
        assert stats["n_pairs"] == 0 and float(loss.detach()) == 0.0 and not g64.any() and bool(low.any()) and bool(high.any())
    if name == "e":
        assert np.isnan(case["ysfc"].numpy()).mean() > 0.15 and n > 1024
    pixels = np.arange(0, n, case["every"])
    if pixels[-1] != n - 1:
        pixels = np.append(pixels, n - 1)
    arrays = dict(z=case["z"].numpy(), ysfc=case["ysfc"].numpy(), loss64=np.float64(float(loss.detach())), grad_pixels=pixels.astype(np.int64),
                  grad64=g64[pixels], grad_max=np.float64(np.abs(g64).max()), stat_n_pairs=np.int64(stats["n_pairs"]),
                  stat_n_active_pixels=np.int64(stats["n_active_pixels"]), **{k: np.float64(v) for k, v in kw.items()})
    path = os.path.join(HERE, f"recovery_disc_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"recovery_disc_{name}", tuple(z.shape), "loss64", float(loss.detach()), "pairs", stats["n_pairs"], "active", stats["n_active_pixels"],
          "(t, t) pairs", int((low & high).sum()), "finite", bool(np.isfinite(g64).all()), os.path.getsize(path), "bytes")


# ---------------------------------------------------------------------------------------------------------------------------
# spread ranking
# ---------------------------------------------------------------------------------------------------------------------------
def spread_cases():
    def case(n, t, b, seed, min_overlap, delta, self_pairs=0):
        return dict(phase=SC.make_points(n, t, 12, seed), ysfc=SC.make_ysfc(n, t, seed + 1), pairs=PC.make_pairs(n, b, seed + 2, self_pairs),
                    dynamism=PC.make_dynamism(n, seed + 3), min_overlap=min_overlap, margin=0.1, delta=delta)

    return {"a": case(40, 5, 64, 501, 3, 0.5, self_pairs=2), "b": case(120, 15, 300, 511, 3, 0.5), "c": case(40, 5, 64, 521, 3, 100.0),
            "d": case(40, 5, 64, 531, 6, 0.5), "e": case(40, 15, 64, 555, 1, 0.25)}


def write_spread(name, case):
    phase = case["phase"].double().requires_grad_(True)
    n, t, d = phase.shape
    spectral = SC.make_points(n, t, 2, 599).double()                    # the batch builder wants spectra; the spread ranking never reads them
    batch = build_phase_neighborhood_batch(spectral, phase, case["ysfc"], case["pairs"], min_overlap=case["min_overlap"])
    valid = batch["valid_pair_mask"]
    idx_i, idx_j = case["pairs"][valid, 0], case["pairs"][valid, 1]
    for key in ("d_learned_self", "d_learned_self_j"):
        if batch[key].requires_grad:
            batch[key].retain_grad()
    loss, stats = compute_phase_spread_ranking(batch, idx_i, idx_j, case["dynamism"].double(), margin=case["margin"], delta=case["delta"])
    bv = int(valid.sum())
    if bv > 0 and loss.requires_grad and loss.grad_fn is not None:
        loss.backward()
    g64 = (torch.zeros_like(phase) if phase.grad is None else phase.grad).numpy()
    mask = batch["mask_self"]
    m = int(batch["M"]) if bv > 0 else 0
    _, rows_i, rows_j, lengths = phase_alignment(case["ysfc"], case["pairs"], case["min_overlap"])   # the package's own alignment
    arrays = dict(phase=case["phase"].numpy(), ysfc=case["ysfc"].numpy(), pairs=case["pairs"].numpy(), dynamism=case["dynamism"].numpy(),
                  min_overlap=np.int64(case["min_overlap"]), margin=np.float64(case["margin"]), delta=np.float64(case["delta"]),
                  loss64=np.float64(float(loss.detach())), grad64=g64, valid_pair_mask=valid.numpy(), M=np.int64(m))
    for k, v in stats.items():
        arrays["stat_" + k] = np.float64(v)
    n_con = stats["n_constrained_i"] + stats["n_constrained_j"]
    if bv > 0:
        assert lengths.shape == (bv,) and rows_i.shape == (bv, m) and torch.equal(SC.length_mask(lengths, m, True), mask)
        gi = batch["d_learned_self"].grad if batch["d_learned_self"].grad is not None else torch.zeros(bv, m, m, dtype=torch.float64)
        gj = batch["d_learned_self_j"].grad if batch["d_learned_self_j"].grad is not None else torch.zeros(bv, m, m, dtype=torch.float64)
        per_pair = torch.where(mask, gi, torch.zeros_like(gi)).sum(dim=(1, 2)) / mask.sum(dim=(1, 2)).clamp(min=1)
        assert torch.allclose(gi, per_pair.reshape(bv, 1, 1) * mask, rtol=0, atol=1e-18) and torch.allclose(gj, -gi, rtol=0, atol=1e-18)
        arrays.update(lengths=lengths.numpy(), mask_self=mask.numpy(), d_self_i=batch["d_learned_self"].detach()[mask].numpy(),
                      d_self_j=batch["d_learned_self_j"].detach()[mask].numpy(), grad64_pair=per_pair.numpy())
        nb = mask.sum(dim=(1, 2)).clamp(min=1).double()
        si = (batch["d_learned_self"].detach() * mask).sum(dim=(1, 2)) / nb
        sj = (batch["d_learned_self_j"].detach() * mask).sum(dim=(1, 2)) / nb
        r = (case["dynamism"][idx_i] - case["dynamism"][idx_j]).double()
        con = r.abs() > case["delta"]
        assert int(con.sum()) == n_con
        assert bool((((si - sj).abs() - case["margin"]).abs()[con] > 1e-4).all()), "a constrained pair sits on the margin"
        assert m <= 32
    if name == "a":
        assert bool(valid[:2].all()) and n_con > 0 and stats["n_constrained_i"] > 0 and stats["n_constrained_j"] > 0
        assert not arrays["grad64_pair"][:2].any()                      # the two (i, i) pairs lead the valid ones and are unconstrained
    if name == "b":
        assert bv > 250 and stats["n_constrained_i"] > 50 and stats["n_constrained_j"] > 50 and m > 8
    if name == "c":
        assert bv > 0 and n_con == 0 and float(loss) == 0.0 and not g64.any()
    if name == "d":
        assert bv == 0 and float(loss) == 0.0
    if name == "e":
        assert bv == case["pairs"].shape[0] and bool((lengths == 1).any()), "no pair with a single shared value"
        inside = torch.arange(m).unsqueeze(0) < lengths.unsqueeze(1)
        con_rows = torch.cat([rows_i[con][inside[con]], rows_j[con][inside[con]]])
        assert n_con > 0 and int(torch.bincount(con_rows).max()) >= 3, "no embedding row shared by three constrained pairs"
    path = os.path.join(HERE, f"spread_rank_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"spread_rank_{name}", tuple(phase.shape), "loss64", float(loss.detach()), "valid", bv, "M", m, "constrained", stats["n_constrained_i"], "+",
          stats["n_constrained_j"], "frac_satisfied", stats["frac_satisfied"], "lengths == 1:", int((lengths == 1).sum()) if bv else 0,
          "finite", bool(np.isfinite(g64).all()), os.path.getsize(path), "bytes")


def main():
    for name, case in recovery_cases().items():
        write_recovery(name, case)
    for name, case in spread_cases().items():
        write_spread(name, case)


if __name__ == "__main__":
    main()
