"""The restatement of spatial pair mining (tests/spatial_pairs_cases.py) against the fixtures written by the REFERENCE's spatial_knn_pairs
and spatial_negative_pairs (tests/golden/make_spatial_pairs_golden.py): neighbour rows equal after the (anchor, row, col) sort, candidate
sets equal per anchor; the draw rule (distinct picks, all candidates, m = min(n, cnt), the extreme draws, uniformity); the bitmap-rank
mapping against torch.unique; the batched restatement; the package's host logic (offset list, integer thresholds) against the
restatement's; and the argument errors of the package's Python layer, which need no GPU."""
import os

import numpy as np
import pytest
import torch

import spatial_pairs_cases as SP


@pytest.fixture(scope="module")
def knn_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "spatial_knn.npz"))


@pytest.fixture(scope="module")
def neg_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "spatial_neg.npz"))


def _neg_case(fx, i):
    dmax = float(fx[f"max_{i}"])
    return float(fx[f"min_{i}"]), None if np.isnan(dmax) else dmax, fx[f"keys_{i}"].astype(np.int64), fx[f"offs_{i}"].astype(np.int64)


@pytest.mark.parametrize("k", SP.FIXTURE_K)
def test_restatement_reproduces_the_reference_neighbours(knn_fx, k):
    idx, rc = SP.knn_pairs(knn_fx["anchors"], knn_fx["mask"], k, int(knn_fx["max_radius"]))
    assert idx.dtype == np.int64 and rc.dtype == np.int64 and bool((np.diff(idx) >= 0).all())
    assert np.array_equal(SP.sorted_rows(idx, rc), knn_fx[f"rows_{k}"].astype(np.int64))


@pytest.mark.parametrize("i", range(len(SP.FIXTURE_NEG)))
def test_restatement_reproduces_the_reference_candidate_sets(neg_fx, i):
    dmin, dmax, keys, offs = _neg_case(neg_fx, i)
    mask, anchors = neg_fx["mask"], neg_fx["anchors"]
    assert (dmin, dmax) == SP.FIXTURE_NEG[i]
    lo, hi = SP.thresholds(dmin, dmax, *mask.shape)
    for a, (r, c) in enumerate(anchors.tolist()):
        assert np.array_equal(SP.candidates(mask, r, c, lo, hi), keys[offs[a]:offs[a + 1]]), (i, a)


def test_fixture_inputs_come_from_the_seeded_makers(knn_fx, neg_fx):
    mask, anchors = SP.fixture_inputs()
    for fx in (knn_fx, neg_fx):
        assert np.array_equal(fx["mask"], mask) and np.array_equal(fx["anchors"], anchors)
    counts = [np.diff(neg_fx[f"offs_{i}"]) for i in range(len(SP.FIXTURE_NEG))]
    assert int(counts[3].sum()) == 0 and bool(((counts[2] > 0) & (counts[2] < 4)).any()) and int(counts[0].min()) >= 4
    assert [len(knn_fx[f"rows_{k}"]) for k in SP.FIXTURE_K] == [91, 177, 263]


def test_draw_rule_on_the_fixture_candidates(neg_fx):
    mask, anchors = neg_fx["mask"], neg_fx["anchors"]
    n = anchors.shape[0]
    for i, n_per in ((0, 4), (2, 4), (2, 64), (3, 4)):
        dmin, dmax, keys, offs = _neg_case(neg_fx, i)
        draws = SP.make_draws(n, n_per, 70 + i)
        idx, rc = SP.negative_pairs(anchors, mask, draws, dmin, dmax, n_per)
        got = rc[:, 0] * mask.shape[1] + rc[:, 1]
        for a in range(n):
            cand, mine = keys[offs[a]:offs[a + 1]], got[idx == a]
            assert len(mine) == min(n_per, len(cand)) and len(set(mine.tolist())) == len(mine) and set(mine.tolist()) <= set(cand.tolist())
        assert bool((np.diff(idx) >= 0).all())
    assert SP.pick_ranks(5, [0, 0, 0, 0, 0, 0], 6) == [0, 1, 2, 3, 4]                     # always the first of what is left
    assert SP.pick_ranks(5, [2 ** 31 - 1] * 4, 4) == [4, 3, 2, 1]                         # always the last of what is left
    assert SP.pick_ranks(7, [0, 2 ** 31 - 1, 0, 2 ** 31 - 1], 4) == [0, 6, 1, 5]
    assert SP.pick_ranks(3, [2 ** 30] * 8, 8) == [1, 2, 0] and SP.pick_ranks(0, [5], 1) == []


def test_draws_are_uniform_without_replacement(neg_fx):
    """20 000 draws of 4 from the candidates of one anchor: chi-square of the pick counts against the uniform expectation 4 * 20 000 / cnt
    below the 99.9 % quantile of chi-square with cnt - 1 degrees of freedom (Wilson-Hilferty, accurate to a fraction of a unit here)."""
    cnt = int(np.diff(neg_fx["offs_1"]).max())
    assert 40 <= cnt <= 200
    draws = np.random.default_rng(99).integers(0, 2 ** 31, (20000, 4))
    hist = np.zeros(cnt)
    for row in draws:
        for q in SP.pick_ranks(cnt, row, 4):
            hist[q] += 1
    expect = 4 * 20000 / cnt
    chi2 = float(((hist - expect) ** 2 / expect).sum())
    dof = cnt - 1
    quantile = dof * (1 - 2 / (9 * dof) + 3.0902 * np.sqrt(2 / (9 * dof))) ** 3
    print(f"chi-square {chi2:.1f} on {dof} degrees of freedom, 99.9 % quantile {quantile:.1f}")
    assert chi2 < quantile


def test_bitmap_rank_equals_torch_unique():
    h, w = 24, 20
    mask, anchors = SP.fixture_inputs()
    _, pos = SP.knn_pairs(anchors, mask, 8, 8)
    _, neg = SP.negative_pairs(anchors, mask, SP.make_draws(len(anchors), 4, 5), 6.0, None, 4)
    coords = np.concatenate([anchors, pos, neg, anchors[:5]], axis=0)
    assert len({tuple(a) for a in anchors.tolist()}) < len(anchors), "no duplicate anchor"
    assert len({tuple(p) for p in pos.tolist()}) < len(pos), "no neighbour shared between anchors"
    unique, inverse = torch.unique(torch.from_numpy(coords), dim=0, return_inverse=True)
    got_unique, got_inverse = SP.bitmap_rank(coords, h, w)
    assert np.array_equal(got_unique, unique.numpy()) and np.array_equal(got_inverse, inverse.numpy())


def _batch():
    shapes = [(24, 20), (24, 20), (24, 20)]
    masks = np.stack([SP.make_mask(*s, 30 + j, invalid=0.2) for j, s in enumerate(shapes)])
    feats = np.stack([SP.make_feat(3, *s, 40 + j) for j, s in enumerate(shapes)])
    off = [0, 12, 12, 13]
    anchors = np.concatenate([SP.make_anchors(24, 20, 12, 50), SP.make_anchors(24, 20, 1, 51)], axis=0)
    return anchors, masks, feats, off, SP.make_draws(13, 4, 52)


def test_batched_restatement_is_the_shifted_concatenation():
    anchors, masks, feats, off, draws = _batch()
    kw = dict(k=6, max_radius=2, min_distance=5.0, max_distance=11.5, n_per_anchor=4, tau=0.7, min_w=0.05)
    out = SP.build_batched(anchors, masks, feats, off, draws, **kw)
    first, last = SP.build(anchors[:12], masks[0], feats[0], draws[:12], **kw), SP.build(anchors[12:], masks[2], feats[2], draws[12:], **kw)
    u0 = first["stats"]["n_unique"]
    assert out["unique_offsets"] == [0, u0, u0, u0 + last["stats"]["n_unique"]] and out["stats"]["n_anchors"] == [12, 0, 1]
    assert np.array_equal(out["pos_pairs"], np.concatenate([first["pos_pairs"], last["pos_pairs"] + u0]))
    assert np.array_equal(out["neg_pairs"], np.concatenate([first["neg_pairs"], last["neg_pairs"] + u0]))
    assert np.array_equal(out["unique_coords"], np.concatenate([first["unique_coords"], last["unique_coords"]]))
    assert np.array_equal(out["pos_weights"], np.concatenate([first["pos_weights"], last["pos_weights"]]))
    assert out["pos_offsets"][-1] == len(out["pos_pairs"]) > 0 and out["neg_offsets"][-1] == len(out["neg_pairs"]) > 0
    coords = out["unique_coords"][out["pos_pairs"][:, 0]]                                  # a pair's first entry is its anchor
    assert {tuple(c) for c in coords[:out["pos_offsets"][1]].tolist()} <= {tuple(a) for a in anchors[:12].tolist()}


def test_package_host_logic_matches_the_restatement():
    from frl_hip.utils import spatial as S
    for k, r in ((4, 8), (6, 8), (8, 1), (64, 1), (64, 8), (12, 3), (5, 64)):
        assert S.neighbor_offsets(k, r) == SP.offsets(k, r), (k, r)
    assert SP.offsets(6, 8) == [(-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1)] and len(SP.offsets(64, 1)) == 4
    for h, w in ((24, 20), (70, 33), (256, 256)):
        for dmin, dmax in SP.FIXTURE_NEG + ((0.0, None), (0.0, 0.0), (16.0, None), (7.07, 7.08), (1e9, None), (3.0, 1e9), (0.5, 0.9)):
            lo, hi = S.distance_thresholds(dmin, dmax, h, w)
            want = SP.thresholds(dmin, dmax, h, w)
            assert (lo, hi) == want or (lo > hi and want[0] > want[1]), (h, w, dmin, dmax, (lo, hi), want)


def test_python_layer_argument_errors():
    from frl_hip import _lib
    from frl_hip.losses import build_spatial_pairs, build_spatial_pairs_batched
    from frl_hip.utils import spatial_knn_pairs, spatial_negative_pairs
    anchors, masks, feats, off, draws = (torch.from_numpy(np.asarray(x)) for x in _batch())
    a, m, f, d = anchors[:12], masks[0], feats[0], draws[:12]
    with pytest.raises(ValueError, match="k must be at least 1"):
        build_spatial_pairs(a, m, f, k=0)
    with pytest.raises(ValueError, match="k must be at least 1"):
        spatial_knn_pairs(a, m, k=0)
    with pytest.raises(ValueError, match="at most 64 neighbours"):
        spatial_knn_pairs(a, m, k=65, max_radius=8)
    with pytest.raises(ValueError, match="max_radius must be in 1..64"):
        spatial_knn_pairs(a, m, k=4, max_radius=65)
    with pytest.raises(ValueError, match="n_per_anchor must be in 1..64"):
        build_spatial_pairs(a, m, f, n_per_anchor=0)
    with pytest.raises(ValueError, match="n_per_anchor must be in 1..64"):
        spatial_negative_pairs(a, m, n_per_anchor=65)
    with pytest.raises(ValueError, match="min_distance must not be negative"):
        spatial_negative_pairs(a, m, min_distance=-1.0)
    with pytest.raises(ValueError, match="max_distance must not be below min_distance"):
        build_spatial_pairs(a, m, f, min_distance=8.0, max_distance=7.5)
    with pytest.raises(ValueError, match="tau must be positive"):
        build_spatial_pairs(a, m, f, tau=0.0)
    with pytest.raises(ValueError, match=r"anchors must be an int64 or int32 \[N, 2\]"):
        build_spatial_pairs(a.float(), m, f)
    with pytest.raises(ValueError, match=r"anchors must be an int64 or int32 \[N, 2\]"):
        spatial_knn_pairs(a[:, :1], m)
    with pytest.raises(ValueError, match="the mask must be a bool"):
        spatial_negative_pairs(a, m.to(torch.uint8))
    with pytest.raises(ValueError, match=r"expected mask \[H, W\] and feat \[C, H, W\]"):
        build_spatial_pairs(a, masks, f)
    with pytest.raises(ValueError, match="the feature maps must be a float32"):
        build_spatial_pairs(a, m, f.double())
    with pytest.raises(ValueError, match="the feature maps must be a float32"):
        build_spatial_pairs(a, m, f[:, :-1])
    with pytest.raises(ValueError, match="at most 256 feature channels"):
        build_spatial_pairs(a, m, torch.zeros(257, 24, 20))
    with pytest.raises(ValueError, match="must not exceed 1024"):
        spatial_knn_pairs(a, torch.ones(8, 1025, dtype=torch.bool))
    with pytest.raises(ValueError, match="draws must be an int64 or int32"):
        build_spatial_pairs(a, m, f, draws=d[:, :3])
    with pytest.raises(ValueError, match="draws must be an int64 or int32"):
        spatial_negative_pairs(a, m, draws=d.float())
    with pytest.raises(ValueError, match=r"draws must lie in \[0, 2\^31\)"):
        spatial_negative_pairs(a, m, draws=d - 1)
    with pytest.raises(ValueError, match=r"draws must lie in \[0, 2\^31\)"):
        build_spatial_pairs(a, m, f, draws=d + 2 ** 31 - 1)
    with pytest.raises(ValueError, match="segment_offsets must rise"):
        build_spatial_pairs_batched(anchors, masks, feats, [0, 12, 11, 13])
    with pytest.raises(ValueError, match="segment_offsets must have 4 entries"):
        build_spatial_pairs_batched(anchors, masks, feats, [0, 12, 13])
    for call in (lambda: build_spatial_pairs(a, m, f, draws=d), lambda: build_spatial_pairs_batched(anchors, masks, feats, off.tolist()),
                 lambda: spatial_knn_pairs(a, m), lambda: spatial_negative_pairs(a, m)):
        with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):   # a CPU tensor raises: there is no CPU path
            call()
