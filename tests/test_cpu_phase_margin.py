"""The float64 restatement of the phase margin losses (tests/phase_margin_cases.py) against the fixtures written by the REFERENCE's
phase_recovery_discrimination_loss and compute_phase_spread_ranking (tests/golden/make_phase_margin_golden.py): losses and gradients to
1e-12, counts equal; the public names; and the argument errors that are raised before any device is touched."""
import os

import numpy as np
import pytest
import torch

import phase_margin_cases as PC
import soft_neighborhood_cases as SC

CASES = ["a", "b", "c", "d", "e"]


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


def _close(got, want, what, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    dev = np.abs(got - want).max(initial=0.0)
    assert got.shape == want.shape and dev <= tol, f"{what}: dev {dev:.3e}"


@pytest.mark.parametrize("case", CASES)
def test_recovery_restatement_reproduces_the_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"recovery_disc_{case}")
    loss, stats, grad = PC.recovery_f64(torch.from_numpy(fx["z"]), torch.from_numpy(fx["ysfc"]), float(fx["margin"]), float(fx["low_ysfc_max"]),
                                        float(fx["high_ysfc_min"]))
    _close(loss, fx["loss64"], "loss")
    assert stats["n_pairs"] == int(fx["stat_n_pairs"]) and stats["n_active_pixels"] == int(fx["stat_n_active_pixels"])
    _close(grad.numpy()[fx["grad_pixels"]], fx["grad64"], "grad")
    _close(grad.abs().max(), fx["grad_max"], "largest gradient entry")
    assert fx["grad_pixels"][-1] == fx["z"].shape[0] - 1 and os.path.getsize(os.path.join(golden_dir, f"recovery_disc_{case}.npz")) < 512 * 1024
    if case == "d":
        assert loss == 0.0 and stats["n_pairs"] == 0 and not grad.any()
    if case == "c":                                                      # overlapping classes: (t, t) pairs sit on the clamp with zero gradient
        low, high = PC.recovery_classes(torch.from_numpy(fx["ysfc"]), float(fx["low_ysfc_max"]), float(fx["high_ysfc_min"]))
        assert bool((low & high).any()) and np.isfinite(fx["grad64"]).all()


def _spread_inputs(fx):
    return {k: torch.from_numpy(fx[k]) for k in ("phase", "ysfc", "pairs", "dynamism")}


def _blocks(fx):
    """The fixture's two float64 blocks [Bv, M, M] (zero where masked) and its mask."""
    mask = fx["mask_self"]
    out = []
    for key in ("d_self_i", "d_self_j"):
        full = np.zeros(mask.shape, dtype=np.float64)
        full[mask] = fx[key]
        out.append(torch.from_numpy(full))
    return out[0], out[1], torch.from_numpy(mask)


def _ref_diff(fx):
    t = _spread_inputs(fx)
    pairs = t["pairs"][torch.from_numpy(fx["valid_pair_mask"])]
    return t["dynamism"].double()[pairs[:, 0]] - t["dynamism"].double()[pairs[:, 1]]


def _check_spread_stats(stats, fx):
    for key in PC.SPREAD_COUNTS:
        assert stats[key] == int(fx["stat_" + key]), key
    for key in PC.SPREAD_MEANS:
        _close(stats[key], fx["stat_" + key], key)


@pytest.mark.parametrize("case", CASES)
def test_spread_restatement_reproduces_the_fixture(golden_dir, case):
    from frl_hip.losses import phase_alignment
    fx = _fx(golden_dir, f"spread_rank_{case}")
    t = _spread_inputs(fx)
    valid, rows_i, rows_j, lengths = phase_alignment(t["ysfc"], t["pairs"], int(fx["min_overlap"]))
    assert np.array_equal(valid.numpy(), fx["valid_pair_mask"])
    if case == "d":
        assert lengths.numel() == 0 and float(fx["loss64"]) == 0.0 and int(fx["stat_n_pairs"]) == 0 and not fx["grad64"].any()
        return
    assert np.array_equal(lengths.numpy(), fx["lengths"]) and rows_i.shape[1] == int(fx["M"]) <= 32
    kw = dict(margin=float(fx["margin"]), delta=float(fx["delta"]))
    # the matrix form on the reference's own blocks
    d_i, d_j, mask = _blocks(fx)
    loss, stats, (gi, gj), (si, sj) = PC.spread_matrix_f64(d_i, d_j, mask, _ref_diff(fx), **kw)
    _close(loss, fx["loss64"], "matrix loss")
    _check_spread_stats(stats, fx)
    _close(gi.numpy(), fx["grad64_pair"].reshape(-1, 1, 1) * fx["mask_self"], "d loss / d d_i")
    _close(gj.numpy(), -fx["grad64_pair"].reshape(-1, 1, 1) * fx["mask_self"], "d loss / d d_j")
    # the gathered form from the embeddings, through the package's alignment
    emb = t["phase"].reshape(-1, t["phase"].shape[2])
    loss_g, stats_g, de = PC.spread_gathered_f64(emb, rows_i, rows_j, lengths, _ref_diff(fx), **kw)
    _close(loss_g, fx["loss64"], "gathered loss")
    _check_spread_stats(stats_g, fx)
    _close(de.reshape(t["phase"].shape).numpy(), fx["grad64"], "d loss / d phase")
    # the properties the cases are there for
    con = _ref_diff(fx).abs() > kw["delta"]
    assert bool((((si - sj).abs() - kw["margin"]).abs()[con] > 1e-4).all())
    if case == "a":
        assert np.array_equal(fx["pairs"][:2, 0], fx["pairs"][:2, 1]) and fx["valid_pair_mask"][:2].all() and not fx["grad64_pair"][:2].any()
    if case == "c":
        assert loss == 0.0 and not con.any() and not fx["grad64"].any()
    if case == "e":
        inside = torch.arange(rows_i.shape[1]).unsqueeze(0) < lengths.unsqueeze(1)
        assert bool((lengths == 1).any()) and int(torch.bincount(torch.cat([rows_i[con][inside[con]], rows_j[con][inside[con]]])).max()) >= 3


def test_public_names_are_exported():
    import frl_hip.losses as L
    for name in ("phase_recovery_discrimination_loss", "compute_phase_spread_ranking", "phase_spread_ranking_gathered", "phase_spread_ranking_loss"):
        assert callable(getattr(L, name)), name


def test_argument_errors_need_no_device():
    from frl_hip.losses import (compute_phase_spread_ranking, phase_recovery_discrimination_loss, phase_spread_ranking_gathered,
                                phase_spread_ranking_loss)
    with pytest.raises(ValueError, match="T <= 32"):
        phase_recovery_discrimination_loss(torch.zeros(4, 33, 12), torch.zeros(4, 33))
    with pytest.raises(ValueError, match="D <= 256"):
        phase_recovery_discrimination_loss(torch.zeros(4, 5, 257), torch.zeros(4, 5))
    with pytest.raises(ValueError, match="ysfc"):
        phase_recovery_discrimination_loss(torch.zeros(4, 5, 12), torch.zeros(4, 6))
    with pytest.raises(ValueError, match="z_phase"):
        phase_recovery_discrimination_loss(torch.zeros(20, 12), torch.zeros(4, 5))
    rows, lengths, r = torch.zeros(3, 33, dtype=torch.int64), torch.ones(3, dtype=torch.int64), torch.zeros(3)
    with pytest.raises(ValueError, match="M <= 32"):
        phase_spread_ranking_gathered(torch.zeros(10, 12), rows, rows, lengths, r)
    with pytest.raises(ValueError, match="D <= 256"):
        phase_spread_ranking_gathered(torch.zeros(10, 257), rows[:, :5], rows[:, :5], lengths, r)
    with pytest.raises(ValueError, match="share one shape"):
        phase_spread_ranking_gathered(torch.zeros(10, 12), rows[:, :5], rows[:, :6], lengths, r)
    with pytest.raises(ValueError, match="lengths and ref_diff"):
        phase_spread_ranking_gathered(torch.zeros(10, 12), rows[:, :5], rows[:, :5], lengths[:2], r)
    with pytest.raises(ValueError, match="lengths and ref_diff"):
        phase_spread_ranking_gathered(torch.zeros(10, 12), rows[:, :5], rows[:, :5], lengths, torch.zeros(4))
    batch = {"d_learned_self": torch.zeros(3, 5, 5), "d_learned_self_j": torch.zeros(3, 5, 4), "mask_self": torch.zeros(3, 5, 5, dtype=torch.bool)}
    idx = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="one shape"):
        compute_phase_spread_ranking(batch, idx, idx, torch.zeros(8))
    batch["d_learned_self_j"] = torch.zeros(3, 5, 5)
    with pytest.raises(ValueError, match="idx_i_valid"):
        compute_phase_spread_ranking(batch, idx[:2], idx, torch.zeros(8))
    with pytest.raises(ValueError, match="D <= 256"):
        phase_spread_ranking_loss(torch.zeros(4, 5, 257), torch.zeros(4, 5), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(4))
    with pytest.raises(ValueError, match="dynamism_ref"):
        phase_spread_ranking_loss(torch.zeros(4, 5, 12), torch.zeros(4, 5), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(5))
    with pytest.raises(ValueError, match="M <= 32"):                    # 33 shared ysfc values: the alignment runs, the launch is refused
        y = torch.arange(33.0).repeat(2, 1)
        phase_spread_ranking_loss(torch.zeros(2, 33, 12), y, torch.tensor([[0, 1]]), torch.zeros(2))


def test_empty_input_launches_nothing():
    from frl_hip.losses import compute_phase_spread_ranking, phase_spread_ranking_loss
    empty = {"n_pairs": 0, "n_constrained_i": 0, "n_constrained_j": 0, "frac_satisfied": 1.0, "mean_spread_i": 0.0, "mean_spread_j": 0.0,
             "mean_ref_diff": 0.0}
    batch = {"d_learned_self": torch.zeros(0, 5, 5), "d_learned_self_j": torch.zeros(0, 5, 5), "mask_self": torch.zeros(0, 5, 5, dtype=torch.bool)}
    idx = torch.zeros(0, dtype=torch.int64)
    loss, stats = compute_phase_spread_ranking(batch, idx, idx, torch.zeros(8))          # CPU tensors: a launch would raise
    assert float(loss.detach()) == 0.0 and loss.requires_grad and stats == empty
    y = SC.make_ysfc(6, 5, 3)
    loss, stats = phase_spread_ranking_loss(torch.zeros(6, 5, 12), y, torch.tensor([[0, 1], [2, 3]]), torch.zeros(6), min_overlap=6)
    assert float(loss.detach()) == 0.0 and loss.requires_grad and stats == empty
    assert phase_spread_ranking_loss(torch.zeros(6, 5, 12), y, torch.tensor([[0, 1]]), torch.zeros(6), min_overlap=6, stats=False)[1] == {}
