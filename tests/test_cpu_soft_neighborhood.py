"""Soft-neighbourhood matching (phase KL) loss, host side: the float64 restatement (tests/soft_neighborhood_cases.py) against the fixtures
the REFERENCE's functions wrote (tests/golden/make_soft_neighborhood_golden.py), the fixtures themselves, the public surface (signatures,
argument errors, no CPU fallback) and the index plumbing of `phase_alignment`, which runs on CPU tensors."""
import inspect
import os

import numpy as np
import pytest
import torch

import soft_neighborhood_cases as SC
from frl_hip.losses import (phase_alignment, phase_neighborhood_loss, soft_neighborhood_loss_gathered,
                            soft_neighborhood_matching_loss)

CASES = ["a", "b", "c", "d", "e", "f"]
POINT_CASES = ["b", "c", "f"]


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


def _kw(fx):
    return dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), min_valid_per_row=int(fx["min_valid_per_row"]),
                pair_weights=torch.from_numpy(fx["pair_weights"]) if "pair_weights" in fx.files else None)


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0)), what


def _matrices(fx):
    return torch.from_numpy(fx["d_reference"]), torch.from_numpy(fx["d_learned"])


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"soft_nbr_{case}")
    d_ref, d_learned = _matrices(fx)
    loss, stats, grad = SC.soft_nbr_f64(d_ref, d_learned, torch.from_numpy(fx["mask"]), **_kw(fx))
    _close(loss, fx["loss64"], f"{case} loss")
    _close(grad.numpy(), fx["grad64"], f"{case} grad")
    for key in SC.STAT_KEYS:
        if "stat_" + key not in fx.files:                                # (the reference's all-rows-skipped return has no entropy keys)
            continue
        if key == "mean_overlap":                                        # the reference averages the counts in float32 whatever the input
            assert abs(stats[key] - float(fx["stat_" + key])) <= 2.0 ** -20 * max(1.0, stats[key]), f"{case} {key}"   # dtype: a few float32 ulps
        else:
            _close(stats[key], fx["stat_" + key], f"{case} {key}")
    assert os.path.getsize(os.path.join(golden_dir, f"soft_nbr_{case}.npz")) < 256 * 1024


@pytest.mark.parametrize("case", POINT_CASES)
def test_restated_point_gradients_match_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"soft_nbr_{case}")
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    ea, eb = t("emb_a"), t("emb_b")
    d_ref, d_learned = SC.pair_distances_f64(t("ref_a"), t("ref_b")), SC.pair_distances_f64(ea, eb)
    assert np.array_equal(torch.where(t("mask"), d_learned.float(), torch.zeros(())).numpy(), fx["d_learned"])     # the stored blocks are these,
    assert np.array_equal(torch.where(t("mask"), d_ref.float(), torch.zeros(())).numpy(), fx["d_reference"])       # rounded to float32
    loss, _, g = SC.soft_nbr_f64(d_ref, d_learned, t("mask"), **_kw(fx))
    _close(loss, fx["loss64_points"], f"{case} loss from the points")
    ga, gb = SC.distance_grads_f64(ea, eb, g)
    if bool(fx["shared"]):
        _close((ga + gb).numpy(), fx["grad64_emb_a"], f"{case} d emb (both roles)")
    else:
        _close(ga.numpy(), fx["grad64_emb_a"], f"{case} d emb_a")
        _close(gb.numpy(), fx["grad64_emb_b"], f"{case} d emb_b")
    # and the gathered restatement: the points as rows of one matrix
    b, m, d = ea.shape
    ref = torch.cat([torch.from_numpy(fx["ref_a"]).reshape(b * m, -1), torch.from_numpy(fx["ref_b"]).reshape(b * m, -1)])
    emb = torch.cat([ea.reshape(b * m, d), eb.reshape(b * m, d)])
    ra = torch.arange(b * m).reshape(b, m)
    rb = ra if bool(fx["shared"]) else ra + b * m
    loss, _, de = SC.gathered_f64(ref, emb, ra, rb, ra, rb, torch.from_numpy(fx["lengths"]), bool(fx["exclude_diagonal"]), **_kw(fx))
    _close(loss, fx["loss64_points"], f"{case} gathered loss")
    _close(de[:b * m].reshape(b, m, d).numpy(), fx["grad64_emb_a"], f"{case} gathered d emb_a")
    _close(de[b * m:].reshape(b, m, d).numpy(), fx["grad64_emb_b"], f"{case} gathered d emb_b")


def test_fixture_cases_are_the_ones_they_claim(golden_dir):
    fx = {c: _fx(golden_dir, f"soft_nbr_{c}") for c in CASES}
    assert {c: fx[c]["mask"].shape for c in CASES} == {"a": (37, 5, 5), "b": (64, 15, 15), "c": (50, 10, 10), "d": (9, 33, 33), "e": (6, 4, 4),
                                                      "f": (16, 15, 15)}
    off = ~np.eye(5, dtype=bool)
    assert (fx["a"]["mask"] == off).all() and "pair_weights" not in fx["a"].files
    b = fx["b"]
    assert b["emb_a"].shape == (64, 15, 12) and bool(b["shared"]) and bool(b["exclude_diagonal"])
    assert b["lengths"].min() == 1 and b["lengths"].max() == 15
    rows_per_pair = (b["mask"].sum(axis=2) >= 2).sum(axis=1)
    assert (rows_per_pair == 0).any() and int(b["stat_n_pairs_active"]) == int((rows_per_pair > 0).sum()) < 64    # pairs without a contributing row
    assert (b["pair_weights"] == 0).sum() == 1 and (float(b["tau_ref"]), float(b["tau_learned"])) == (0.1, 0.1)
    c = fx["c"]
    assert not bool(c["shared"]) and not bool(c["exclude_diagonal"]) and c["mask"][:, 0, 0].all()                # the diagonal is in c's mask
    assert len(set(c["lengths"].tolist())) > 3 and "pair_weights" in c.files
    d = fx["d"]
    assert int(d["min_valid_per_row"]) == 4 and (float(d["tau_ref"]), float(d["tau_learned"])) == (0.5, 0.25) and "emb_a" not in d.files
    e = fx["e"]
    assert (e["mask"].sum(axis=2) < int(e["min_valid_per_row"])).all() and float(e["loss64"]) == 0.0 and not e["grad64"].any()
    f = fx["f"]
    assert float(f["tau_ref"]) == 0.01 and np.isfinite(f["grad64"]).all() and float(f["stat_mean_entropy_p"]) < 0.1   # a nearly one-hot p
    for c in CASES:                                                      # inputs on the 2^-8 grid, results finite
        for key in ("d_reference", "d_learned", "ref_a", "ref_b", "emb_a", "emb_b"):
            if key in fx[c].files and not (key.startswith("d_") and "emb_a" in fx[c].files):     # (a points case's blocks are its distances)
                assert fx[c][key].dtype == np.float32 and (fx[c][key] * 256 == np.round(fx[c][key] * 256)).all()
        assert np.isfinite(fx[c]["grad64"]).all() and fx[c]["grad64"].dtype == np.float64


def test_phase_fixture_is_what_it_claims(golden_dir):
    fx = _fx(golden_dir, "phase_nbr_a")
    assert fx["spectral"].shape == (40, 15, 6) and fx["phase"].shape == (40, 15, 12) and fx["ysfc"].shape == (40, 15)
    pairs = fx["pairs"]
    assert pairs.shape == (200, 2) and (pairs[:, 0] == pairs[:, 1]).sum() >= 20
    assert (np.diff(fx["ysfc"], axis=1) < 0).any() and (fx["ysfc"] == np.round(fx["ysfc"])).all()                  # ramps with resets
    valid = fx["valid_pair_mask"]
    assert 0 < valid.sum() < 200 and valid[:20].any()                   # some pairs fall short of the overlap; self-pairs take part
    assert np.isfinite(fx["grad64"]).all() and fx["grad64"].shape == (40, 15, 12)
    assert os.path.getsize(os.path.join(golden_dir, "phase_nbr_a.npz")) < 256 * 1024


def test_signatures_match_reference():
    sig = inspect.signature(soft_neighborhood_matching_loss)
    pos = [p for p in sig.parameters.values() if p.kind is not inspect.Parameter.KEYWORD_ONLY]
    assert [p.name for p in pos] == ["d_reference", "d_learned", "mask", "tau_ref", "tau_learned", "pair_weights", "min_valid_per_row"]
    assert [p.default for p in pos[3:]] == [1.0, 1.0, None, 2]
    assert sig.parameters["stats"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["stats"].default is True
    sig = inspect.signature(phase_neighborhood_loss)
    assert list(sig.parameters) == ["spectral_features", "phase_embeddings", "ysfc", "pair_indices", "pair_weights", "tau_ref", "tau_learned",
                                    "min_overlap", "min_valid_per_row", "self_similarity_weight", "cross_pixel_weight", "_batch"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [None, 0.1, 0.1, 3, 2, 1.0, 1.0, None]
    sig = inspect.signature(soft_neighborhood_loss_gathered)
    assert list(sig.parameters) == ["ref", "emb", "ref_rows_a", "ref_rows_b", "emb_rows_a", "emb_rows_b", "lengths", "exclude_diagonal",
                                    "tau_ref", "tau_learned", "pair_weights", "min_valid_per_row", "stats"]
    assert list(inspect.signature(phase_alignment).parameters) == ["ysfc", "pair_indices", "min_overlap"]
    assert inspect.signature(phase_alignment).parameters["min_overlap"].default == 3


def _gathered_args(b=3, m=4, c=2, d=3):
    rows = torch.arange(b * m).reshape(b, m)
    return (torch.randn(b * m, c), torch.randn(b * m, d), rows, rows, rows, rows, torch.full((b,), m, dtype=torch.int64), True)


def test_min_valid_per_row_below_two_raises():
    d = torch.rand(2, 3, 3)
    mask = torch.ones(2, 3, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match="min_valid_per_row"):
        soft_neighborhood_matching_loss(d, d, mask, min_valid_per_row=1)
    with pytest.raises(ValueError, match="min_valid_per_row"):
        soft_neighborhood_loss_gathered(*_gathered_args(), min_valid_per_row=1)
    with pytest.raises(ValueError, match="min_valid_per_row"):
        phase_neighborhood_loss(torch.randn(4, 5, 2), torch.randn(4, 5, 3), torch.zeros(4, 5), torch.zeros(2, 2, dtype=torch.int64),
                                min_valid_per_row=1)


def test_cpu_tensors_are_refused():
    from frl_hip import ops
    from frl_hip._lib import FrlHipError
    d = torch.rand(2, 3, 3)
    mask = torch.ones(2, 3, 3, dtype=torch.bool)
    with pytest.raises(FrlHipError, match="GPU"):
        soft_neighborhood_matching_loss(d, d, mask)
    with pytest.raises(FrlHipError, match="GPU"):
        soft_neighborhood_loss_gathered(*_gathered_args())
    with pytest.raises(FrlHipError, match="GPU"):
        ops.soft_nbr_fwd(d, d, mask)
    with pytest.raises(FrlHipError, match="GPU"):
        ops.soft_nbr_bwd(d, torch.zeros(2, 6), None, torch.zeros(2), torch.ones(1))
    ref, emb, rows, _, _, _, lengths, _ = _gathered_args()
    with pytest.raises(FrlHipError, match="GPU"):
        ops.soft_nbr_gathered_fwd(ref, emb, torch.stack([rows] * 4), lengths, True)
    with pytest.raises(FrlHipError, match="GPU"):
        ops.soft_nbr_gathered_bwd(ref, emb, torch.stack([rows] * 4), lengths, True, None, 1.0, 1.0, 2, torch.zeros(3, 6), torch.zeros(2), torch.ones(1))


def test_gathered_form_names_its_limits():
    with pytest.raises(ValueError, match="M <= 32"):
        soft_neighborhood_loss_gathered(*_gathered_args(b=2, m=33))
    with pytest.raises(ValueError, match="256"):
        soft_neighborhood_loss_gathered(*_gathered_args(c=257))
    with pytest.raises(ValueError, match="256"):
        soft_neighborhood_loss_gathered(*_gathered_args(d=257))


def test_phase_alignment_reproduces_the_reference_batch(golden_dir):
    fx = _fx(golden_dir, "phase_nbr_a")
    ysfc, pairs = torch.from_numpy(fx["ysfc"]), torch.from_numpy(fx["pairs"])
    valid, rows_i, rows_j, lengths = phase_alignment(ysfc, pairs, int(fx["min_overlap"]))
    assert valid.dtype == torch.bool and np.array_equal(valid.numpy(), fx["valid_pair_mask"])
    m = int(fx["M"])
    assert rows_i.shape == rows_j.shape == (int(valid.sum()), m) and lengths.shape == (int(valid.sum()),)
    assert rows_i.dtype == rows_j.dtype == lengths.dtype == torch.int64 and int(lengths.max()) == m
    pad = torch.arange(m).unsqueeze(0) >= lengths.unsqueeze(1)
    assert (rows_i[pad] == 0).all() and (rows_j[pad] == 0).all()         # padding holds 0 and sits beyond lengths
    t = ysfc.shape[1]
    pv = pairs[valid]
    assert ((rows_i // t)[~pad] == pv[:, :1].expand(-1, m)[~pad]).all() and ((rows_j // t)[~pad] == pv[:, 1:].expand(-1, m)[~pad]).all()
    mask_cross, mask_self = SC.length_mask(lengths, m, False), SC.length_mask(lengths, m, True)
    assert np.array_equal(mask_cross.numpy(), fx["mask_cross"]) and np.array_equal(mask_self.numpy(), fx["mask_self"])
    spec = torch.from_numpy(fx["spectral"]).double().reshape(-1, fx["spectral"].shape[2])
    emb = torch.from_numpy(fx["phase"]).double().reshape(-1, fx["phase"].shape[2])
    for key, src, ra, rb, mask in (("d_ref_self", spec, rows_j, rows_j, mask_self), ("d_learned_self", emb, rows_i, rows_i, mask_self),
                                   ("d_ref_cross", spec, rows_i, rows_j, mask_cross), ("d_learned_cross", emb, rows_i, rows_j, mask_cross)):
        _close(SC.pair_distances_f64(src[ra], src[rb])[mask].numpy(), fx[key], key)
    # and the whole loss, restated over those rows, is the reference's
    w = torch.from_numpy(fx["weights"])[valid]
    kw = dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), pair_weights=w, min_valid_per_row=int(fx["min_valid_per_row"]))
    ls, _, gs = SC.gathered_f64(spec, emb, rows_j, rows_j, rows_i, rows_i, lengths, True, **kw)
    lc, _, gc = SC.gathered_f64(spec, emb, rows_i, rows_j, rows_i, rows_j, lengths, False, **kw)
    ws, wc = float(fx["self_similarity_weight"]), float(fx["cross_pixel_weight"])
    _close(ws * ls + wc * lc, fx["loss64"], "phase loss")
    _close(ls, fx["stat_loss_self"], "loss_self")
    _close(lc, fx["stat_loss_cross"], "loss_cross")
    _close((ws * gs + wc * gc).reshape(fx["grad64"].shape).numpy(), fx["grad64"], "phase grad")


def test_phase_alignment_edge_cases():
    ysfc = torch.tensor([[0, 1, 2, 0, 1, 2, 3], [5, 6, 7, 8, 9, 10, 11], [2, 2, 2, 2, 2, 2, 2]])
    valid, rows_i, rows_j, lengths = phase_alignment(ysfc, torch.tensor([[0, 0], [0, 1], [0, 2]]), min_overlap=1)
    assert valid.tolist() == [True, False, True] and lengths.tolist() == [4, 1]
    # values 0, 1, 2 of pixel 0 come from its longer, second sequence (t = 3, 4, 5); 3 from t = 6
    assert rows_i[0].tolist() == [3, 4, 5, 6] and rows_j[0].tolist() == [3, 4, 5, 6]
    # equal values do not start a sequence: the constant pixel is one sequence, and its most recent t = 6 represents value 2
    assert rows_i[1].tolist() == [5, 0, 0, 0] and rows_j[1].tolist() == [2 * 7 + 6, 0, 0, 0]
    valid, rows_i, rows_j, lengths = phase_alignment(ysfc, torch.tensor([[0, 1]]), min_overlap=3)
    assert valid.tolist() == [False] and rows_i.shape == (0, 0) and rows_j.shape == (0, 0) and lengths.numel() == 0
    loss, stats = phase_neighborhood_loss(torch.randn(3, 7, 2), torch.randn(3, 7, 3), ysfc, torch.tensor([[0, 1]]))
    assert float(loss.detach()) == 0.0 and stats == {"n_pairs_input": 1, "n_pairs_sufficient_overlap": 0, "loss_self": 0.0, "loss_cross": 0.0}
