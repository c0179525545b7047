"""The float64 restatement of phase pair mining (tests/phase_pairs_cases.py) against the fixtures written by the REFERENCE's
build_phase_pairs (tests/golden/make_phase_pairs_golden.py): pairs exact and in order, integer statistics exact, weights and float
statistics to 1e-12; its batched form; its (distance, index) order on exactly tied distances; and the argument errors of the package's
Python layer that need no GPU."""
import os

import numpy as np
import pytest
import torch

import phase_pairs_cases as PP

CASES = list(PP.CASES)


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"phase_pairs_{name}.npz"))


def _kw(fx):
    return dict(k=int(fx["k"]), min_overlap=int(fx["min_overlap"]), min_pairs=int(fx["min_pairs"]), include_self=bool(fx["include_self"]),
                sigma=float(fx["sigma"]), self_pair_weight=float(fx["self_pair_weight"]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(golden_dir, name):
    fx = _fx(golden_dir, name)
    pairs, weights, stats, _ = PP.phase_pairs_f64(torch.from_numpy(fx["spec"]), torch.from_numpy(fx["ysfc"]), **_kw(fx))
    assert pairs.dtype == torch.int64 and np.array_equal(pairs.numpy(), fx["pairs"].astype(np.int64))
    assert np.abs(weights.numpy() - fx["weights64"]).max(initial=0.0) <= 1e-12
    want = {key[5:]: float(fx[key]) for key in fx.files if key.startswith("stat_")}
    assert set(stats) == set(want)
    for key in stats:
        if key in PP.COUNT_KEYS:
            assert stats[key] == int(want[key]), key
        else:
            assert abs(stats[key] - want[key]) <= 1e-12, key


def test_fixture_inputs_come_from_the_seeded_makers(golden_dir):
    for name in CASES:
        fx = _fx(golden_dir, name)
        spec, ysfc, kw = PP.case_inputs(name)
        assert np.array_equal(spec.numpy(), fx["spec"]) and np.array_equal(ysfc.numpy(), fx["ysfc"]) and kw == _kw(fx), name


def test_fixtures_hold_what_they_are_there_for(golden_dir):
    a, g, h, d, e, c, k1 = (_fx(golden_dir, n) for n in ("a", "g", "h", "d", "e", "c", "k1"))
    assert a["pairs"].shape == (295, 2) and int(a["stat_n_anchors_surviving"]) == 27 and int(a["stat_n_after_overlap"]) == 292
    assert np.array_equal(g["pairs"], a["pairs"]) and g["ysfc"].min() < 64 <= g["ysfc"].max()
    assert h["pairs"].shape == (0, 2) and int(h["stat_n_after_overlap"]) == 0 and int(h["stat_n_candidates"]) == 592
    assert d["pairs"].shape == (0, 2) and int(d["stat_n_candidates"]) == 1024 and "stat_dist_mean" not in d.files
    assert int(e["stat_n_self_pairs"]) == 0 and e["pairs"].shape == (1742, 2)
    assert c["pairs"].shape == (64, 2) and int(c["k"]) > c["spec"].shape[0] - 1
    assert int(k1["stat_n_self_pairs"]) == 65 and k1["pairs"].shape == (130, 2)


def test_batched_restatement_is_the_shifted_concatenation():
    parts = [PP.case_inputs("a"), PP.make_inputs(1, 7, 5, 591) + (None,), PP.case_inputs("h")]
    spec = torch.cat([p[0] for p in parts])
    ysfc = torch.cat([p[1] for p in parts])
    off = [0, 37, 38, 38, 75]
    pairs, weights, stats = PP.phase_pairs_batched_f64(spec, ysfc, off)
    p0, w0, s0, _ = PP.phase_pairs_f64(parts[0][0], parts[0][1])
    p2, w2, s2, _ = PP.phase_pairs_f64(parts[2][0], parts[2][1])                  # the same rows as segment 0, under default parameters
    assert torch.equal(pairs, torch.cat([p0, p2 + 38])) and torch.equal(weights, torch.cat([w0, w2]))
    assert torch.equal(pairs[:295], p0) and int(pairs[295:].min()) >= 38
    assert stats["n_anchors"] == 75 and stats["n_total_pairs"] == 590 and stats["n_candidates"] == 2 * 592
    assert [s["n_anchors"] for s in stats["per_segment"]] == [37, 1, 0, 37] and stats["per_segment"][0] == s0
    assert stats["per_segment"][1] == PP.empty_stats(1) and stats["per_segment"][2] == PP.empty_stats(0)


def test_tied_distances_follow_distance_then_index():
    spec, ysfc = PP.make_tied_inputs()
    n, k = spec.shape[0], 16
    d2 = PP.squared_distances_f64(spec)
    d2.fill_diagonal_(float("inf"))
    head = torch.sort(d2, dim=1).values[:, :k + 1]
    assert int((head[:, 1:] == head[:, :-1]).any(dim=1).sum()) > n // 2, "the tied case holds too few ties"
    assert bool((head[:, k] == head[:, k - 1]).any()), "no tie across the k-th place"
    _, _, _, raw = PP.phase_pairs_f64(spec, ysfc, k=k)
    knn, nd2 = raw["knn"], raw["d2"]
    assert bool(((nd2[:, 1:] > nd2[:, :-1]) | ((nd2[:, 1:] == nd2[:, :-1]) & (knn[:, 1:] > knn[:, :-1]))).all())
    for i in range(n):                                                  # a plain loop: sort the (distance, index) tuples
        want = sorted((float(d2[i, j]), j) for j in range(n) if j != i)[:k]
        assert [j for _, j in want] == knn[i].tolist()


def test_restatement_truncates_ysfc_like_long():
    spec, ysfc, kw = PP.case_inputs("a")
    p0, w0, _, _ = PP.phase_pairs_f64(spec, ysfc, **kw)
    p1, w1, _, _ = PP.phase_pairs_f64(spec, ysfc + 0.75, **kw)
    assert torch.equal(p0, p1) and torch.equal(w0, w1)


def test_python_layer_argument_errors():
    from frl_hip import _lib, ops
    from frl_hip.losses import build_phase_pairs, build_phase_pairs_batched
    spec, ysfc, _ = PP.case_inputs("a")
    with pytest.raises(ValueError, match="k must be in 1..64"):
        build_phase_pairs(spec, ysfc, k=65)
    with pytest.raises(ValueError, match="k must be in 1..64"):
        build_phase_pairs(spec, ysfc, k=0)
    with pytest.raises(ValueError, match="sigma must be positive"):
        build_phase_pairs(spec, ysfc, sigma=0.0)
    with pytest.raises(ValueError, match=r"expected spec_features \[N, C\]"):
        build_phase_pairs(spec, ysfc[:-1])
    with pytest.raises(ValueError, match="segment_offsets must rise"):
        build_phase_pairs_batched(spec, ysfc, [0, 20, 10, 37])
    with pytest.raises(ValueError, match="segment_offsets must rise"):
        build_phase_pairs_batched(spec, ysfc, [0, 36])
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):    # a CPU tensor raises: there is no CPU path
        build_phase_pairs(spec, ysfc)
    seg = torch.tensor([0, 37], dtype=torch.int32)
    with pytest.raises(ValueError, match="k must be in 1..64"):
        ops.phase_pairs(spec, ysfc, seg, seg, 65, 3, 5, 5.0)
    with pytest.raises(ValueError, match="at most 256"):
        ops.phase_pairs(torch.zeros(4, 272), torch.zeros(4, 3), torch.tensor([0, 4], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32),
                        2, 3, 5, 5.0)
    pairs, weights, stats = build_phase_pairs(spec[:1], ysfc[:1])       # fewer than two anchors: the reference's empty result, no launch
    assert pairs.shape == (0, 2) and pairs.dtype == torch.int64 and weights.shape == (0,) and weights.dtype == torch.float32
    assert stats == {**PP.empty_stats(1)} and set(stats) == set(PP.EMPTY_KEYS)
    assert build_phase_pairs(spec[:1], ysfc[:1], stats=False)[2] == {}
