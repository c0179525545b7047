"""GPU parity of spatial pair mining (csrc/spatial_pairs.hip behind losses.build_spatial_pairs / build_spatial_pairs_batched and
utils.spatial_knn_pairs / spatial_negative_pairs) against the fixtures written by the REFERENCE (tests/golden/make_spatial_pairs_golden.py)
and against the restatement (tests/spatial_pairs_cases.py, pinned to the fixtures by tests/test_cpu_spatial_pairs.py) under the same draws.

Bounds.  Every integer output is equal, order included.  The feature maps lie on the 2^-8 grid with squared distances below 256, so the
kernel's float32 sum of squares (fused multiply-adds, channels ascending) is exact.  d is then one correctly rounded sqrtf: within 2^-24 d.
With x = d / tau (tau exactly representable here) the exponent carries the rounding of sqrtf and of the division, at most x 2^-23
relatively, expf adds about one ulp, and as in test_gpu_phase_pairs.py the bound is twice that sum: w_pos within (2 + x) 2^-22 w64 of the
float64 value before the clamp.  w_neg = 1 - e rounds once more, a value of at most 1: the same absolute bound plus 2^-24.  The clamp is
1-Lipschitz (min_w is exactly representable here too), so both bounds hold after it."""
import functools
import os

import numpy as np
import pytest
import torch

import spatial_pairs_cases as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_KEYS = ("unique_coords", "anchor_to_unique", "pos_pairs", "neg_pairs")
LIST_KEYS = ("unique_offsets", "pos_offsets", "neg_offsets")

# name -> (H, W, N, invalid fraction, parameters)
CASES = {
    "below_one_word": (24, 20, 37, 0.1, dict(k=4, max_radius=8, min_distance=6.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.0625)),
    "three_words_n64": (40, 70, 130, 0.3, dict(k=6, max_radius=8, min_distance=5.0, max_distance=5.0, n_per_anchor=64, tau=0.75, min_w=0.0625)),
    "tall_one_bit_word": (70, 33, 37, 0.1, dict(k=8, max_radius=1, min_distance=16.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.0625)),
    "beyond_diagonal_one_anchor": (70, 33, 1, 0.1, dict(k=64, max_radius=1, min_distance=100.0, max_distance=None, n_per_anchor=1, tau=1.0, min_w=0.0625)),
    "sparse_k64": (24, 20, 130, 0.99, dict(k=64, max_radius=8, min_distance=6.1, max_distance=12.3, n_per_anchor=1, tau=0.5, min_w=0.25)),
    "sparse_n4": (40, 70, 37, 0.99, dict(k=4, max_radius=8, min_distance=6.0, max_distance=9.5, n_per_anchor=4, tau=1.0, min_w=0.0625)),
    "live_size": (256, 256, 37, 0.1, dict(k=4, max_radius=8, min_distance=16.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.0625)),
    "limit_size": (1024, 1000, 9, 0.1, dict(k=4, max_radius=8, min_distance=900.0, max_distance=1300.5, n_per_anchor=4, tau=1.0, min_w=0.0625)),
}


SEED_ORDER = ["below_one_word", "beyond_diagonal_one_anchor", "live_size", "sparse_k64", "sparse_n4", "tall_one_bit_word", "three_words_n64",
              "limit_size"]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    h, w, n, invalid, kw = CASES[name]
    seed = 1000 + 10 * SEED_ORDER.index(name)
    mask, anchors, feat = SP.make_mask(h, w, seed, invalid=invalid), SP.make_anchors(h, w, n, seed + 1), SP.make_feat(8, h, w, seed + 2)
    draws = SP.make_draws(n, kw["n_per_anchor"], seed + 3)
    return mask, anchors, feat, draws, kw, SP.build(anchors, mask, feat, draws, **kw)


def _check(got, want, tau, what):
    for key in INT_KEYS:
        assert got[key].dtype == torch.int64 and got[key].is_cuda, key
        assert np.array_equal(got[key].cpu().numpy(), want[key]), f"{what}: {key} differs from the restatement's"
    for key in LIST_KEYS:
        assert list(got[key]) == list(want[key]), key
    assert got["stats"] == want["stats"]
    for sign in ("pos", "neg"):
        d64, raw64, w64 = want[f"{sign}_dist"], want[f"{sign}_raw"], want[f"{sign}_weights"]
        d, wgt = got[f"{sign}_dist"], got[f"{sign}_weights"]
        assert d.dtype == torch.float32 and wgt.dtype == torch.float32 and d.shape == d64.shape and wgt.shape == w64.shape
        ddev = np.abs(d.double().cpu().numpy() - d64)
        bound = (2.0 + d64 / tau) * 2.0 ** -22 * np.exp(-d64 / tau) + (2.0 ** -24 if sign == "neg" else 0.0)
        wdev = np.abs(wgt.double().cpu().numpy() - w64)
        if len(d64):
            print(f"{what} {sign}: {len(d64)} pairs, worst d dev / bound {float((ddev / np.maximum(2.0 ** -24 * d64, 1e-300)).max()):.3f}, "
                  f"worst w dev / bound {float((wdev / bound).max()):.3f}, clamped {int((raw64 != w64).sum())}")
        assert bool((ddev <= 2.0 ** -24 * d64).all()), f"{what}: {sign}_dist"
        assert bool((wdev <= bound).all()), f"{what}: {sign}_weights"


@pytest.mark.parametrize("name", list(CASES))
def test_single_sample_equals_the_restatement(name):
    from frl_hip.losses import build_spatial_pairs
    mask, anchors, feat, draws, kw, want = _case(name)
    got = build_spatial_pairs(_dev(anchors), _dev(mask), _dev(feat), draws=_dev(draws), **kw)
    _check(got, want, kw["tau"], name)
    again = build_spatial_pairs(_dev(anchors).to(torch.int32), _dev(mask), _dev(feat), draws=_dev(draws).to(torch.int32), **kw)
    for key in INT_KEYS + ("pos_weights", "neg_weights", "pos_dist", "neg_dist"):
        assert torch.equal(again[key], got[key]), key


def test_cases_hold_what_they_are_there_for():
    lo, hi = SP.thresholds(5.0, 5.0, 40, 70)
    mask, anchors, _, _, kw, want = _case("three_words_n64")
    counts = np.asarray([len(SP.candidates(mask, r, c, lo, hi)) for r, c in anchors.tolist()])
    assert 0 < counts.max() < 64 and want["stats"]["n_neg"] == int(counts.sum())          # n = 64 and every cnt below it
    assert _case("beyond_diagonal_one_anchor")[5]["stats"]["n_neg"] == 0 and len(SP.offsets(64, 1)) == 4
    for name, n_per in (("sparse_k64", 1), ("sparse_n4", 4)):
        mask, anchors, _, _, kw, _ = _case(name)
        lo, hi = SP.thresholds(kw["min_distance"], kw["max_distance"], *mask.shape)
        counts = np.asarray([len(SP.candidates(mask, r, c, lo, hi)) for r, c in anchors.tolist()])
        assert bool((counts == 0).any()) and bool((counts >= n_per).any()), name
        if n_per > 1:
            assert bool(((counts > 0) & (counts < n_per)).any()), name
    half = _case("sparse_k64")[5]                                                          # tau = 0.5, min_w = 0.25: clamped and not
    assert bool((half["pos_raw"] == half["pos_weights"]).any()) and bool((half["pos_raw"] != half["pos_weights"]).any())


@pytest.fixture(scope="module")
def batch():
    """40 x 70, segments [37, 0, 1, 12, 130]: a plain one, an empty one, a single anchor, one whose mask is all False, a long one."""
    h, w, lengths = 40, 70, [37, 0, 1, 12, 130]
    masks = np.stack([SP.make_mask(h, w, 300 + j, invalid=0.2) for j in range(5)])
    masks[3] = False
    feats = np.stack([SP.make_feat(8, h, w, 310 + j) for j in range(5)])
    anchors = np.concatenate([SP.make_anchors(h, w, n, 320 + j) for j, n in enumerate(lengths)], axis=0)
    off = [0] + np.cumsum(lengths).tolist()
    return anchors, masks, feats, off, SP.make_draws(off[-1], 4, 330)


@pytest.mark.parametrize("params", [dict(min_distance=6.0, min_w=0.0625), dict(k=6, max_radius=3, min_distance=5.0, max_distance=9.5, tau=0.5, min_w=0.25)],
                         ids=["defaults", "bounded"])
def test_batched_equals_single_calls_and_restatement(batch, params):
    from frl_hip.losses import build_spatial_pairs, build_spatial_pairs_batched
    anchors, masks, feats, off, draws = batch
    kw = {**SP.DEFAULTS, **params}
    ad, md, fd, dd = _dev(anchors), _dev(masks), _dev(feats), _dev(draws)
    got = build_spatial_pairs_batched(ad, md, fd, off, draws=dd, **kw)
    _check(got, SP.build_batched(anchors, masks, feats, off, draws, **kw), kw["tau"], "batched")
    assert got["stats"]["n_pos"][3] == 0 and got["stats"]["n_neg"][3] == 0 and got["stats"]["n_unique"][3] > 0 and got["stats"]["n_unique"][1] == 0
    assert got["stats"]["n_pos"][0] > 0 and got["stats"]["n_neg"][4] > 0
    singles = [build_spatial_pairs(ad[a:b], md[s], fd[s], draws=dd[a:b], **kw) for s, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    shifts = got["unique_offsets"][:-1]
    for key in INT_KEYS:
        parts = [p[key] + (sh if key in SP.SHIFTED_KEYS else 0) for p, sh in zip(singles, shifts)]
        assert torch.equal(got[key], torch.cat(parts)), f"{key}: not the shifted concatenation"
    for key in ("pos_weights", "neg_weights", "pos_dist", "neg_dist"):
        assert torch.equal(got[key], torch.cat([p[key] for p in singles])), key
    same = build_spatial_pairs_batched(ad, md, fd, torch.tensor(off), draws=dd, **kw)
    assert all(torch.equal(same[key], got[key]) for key in INT_KEYS)


@pytest.mark.parametrize("k", SP.FIXTURE_K)
def test_fixture_neighbours(golden_dir, k):
    from frl_hip.utils import spatial_knn_pairs
    fx = np.load(os.path.join(golden_dir, "spatial_knn.npz"))
    idx, rc = spatial_knn_pairs(_dev(fx["anchors"]), _dev(fx["mask"]), k=k, max_radius=int(fx["max_radius"]))
    assert idx.dtype == torch.int64 and rc.dtype == torch.int64 and rc.shape == (idx.shape[0], 2) and bool((idx[1:] >= idx[:-1]).all())
    assert np.array_equal(SP.sorted_rows(idx.cpu().numpy(), rc.cpu().numpy()), fx[f"rows_{k}"].astype(np.int64)), "not the reference's rows"
    want_idx, want_rc = SP.knn_pairs(fx["anchors"], fx["mask"], k, int(fx["max_radius"]))          # and in the documented order
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(rc.cpu().numpy(), want_rc)


@pytest.mark.parametrize("i", range(len(SP.FIXTURE_NEG)))
def test_fixture_candidate_sets(golden_dir, i):
    """n_per_anchor = 64: an anchor with at most 64 candidates must return exactly the reference's set, any other 64 distinct members."""
    from frl_hip.utils import spatial_negative_pairs
    fx = np.load(os.path.join(golden_dir, "spatial_neg.npz"))
    dmin, dmax = SP.FIXTURE_NEG[i]
    anchors, mask, keys, offs = fx["anchors"], fx["mask"], fx[f"keys_{i}"].astype(np.int64), fx[f"offs_{i}"].astype(np.int64)
    draws = SP.make_draws(len(anchors), 64, 900 + i)
    idx, rc = spatial_negative_pairs(_dev(anchors), _dev(mask), dmin, dmax, 64, draws=_dev(draws))
    idx, got = idx.cpu().numpy(), (rc[:, 0] * mask.shape[1] + rc[:, 1]).cpu().numpy()
    assert bool((np.diff(idx) >= 0).all())
    whole = 0
    for a in range(len(anchors)):
        cand, mine = keys[offs[a]:offs[a + 1]], got[idx == a]
        assert len(mine) == min(64, len(cand)) and len(set(mine.tolist())) == len(mine), (i, a)
        if len(cand) <= 64:
            whole += 1
            assert np.array_equal(np.sort(mine), cand), (i, a)
        else:
            assert set(mine.tolist()) <= set(cand.tolist()), (i, a)
    print(f"case {i}: {whole} of {len(anchors)} anchors return their whole candidate set")
    assert whole == len(anchors) or i not in (2, 3)
    want_idx, want_rc = SP.negative_pairs(anchors, mask, draws, dmin, dmax, 64)
    assert np.array_equal(idx, want_idx) and np.array_equal(rc.cpu().numpy(), want_rc)


def test_generator_draws_are_reproducible_and_valid():
    from frl_hip.losses import build_spatial_pairs
    from frl_hip.utils import spatial_negative_pairs
    mask, anchors, feat, _, kw, _ = _case("three_words_n64")
    kw = {**kw, "min_distance": 6.0, "max_distance": 9.5, "n_per_anchor": 4}
    ad, md, fd = _dev(anchors), _dev(mask), _dev(feat)
    outs = []
    for _ in range(2):
        g = torch.Generator(device=DEV)
        g.manual_seed(77)
        outs.append(build_spatial_pairs(ad, md, fd, generator=g, **kw))
    assert all(torch.equal(outs[0][key], outs[1][key]) for key in INT_KEYS + ("neg_weights",)) and outs[0]["stats"]["n_neg"] > 0
    idx, rc = spatial_negative_pairs(ad, md, 6.0, 9.5, 4)
    idx, rc = idx.cpu().numpy(), rc.cpu().numpy()
    lo, hi = SP.thresholds(6.0, 9.5, *mask.shape)
    for a, (r, c) in enumerate(anchors.tolist()):
        cand = set(SP.candidates(mask, r, c, lo, hi).tolist())
        mine = (rc[idx == a][:, 0] * mask.shape[1] + rc[idx == a][:, 1]).tolist()
        assert len(mine) == min(4, len(cand)) and len(set(mine)) == len(mine) and set(mine) <= cand, a


def test_out_of_range_anchor_and_draw_raise():
    from frl_hip.losses import build_spatial_pairs, build_spatial_pairs_batched
    from frl_hip.utils import spatial_knn_pairs, spatial_negative_pairs
    mask, anchors, feat, draws, kw, _ = _case("below_one_word")
    ad, md, fd, dd = _dev(anchors), _dev(mask), _dev(feat), _dev(draws)
    for bad in ((24, 3), (-1, 3), (3, 20), (3, -1), (2 ** 40, 3), (3, -2 ** 40)):
        moved = ad.clone()
        moved[17] = torch.tensor(bad, device=DEV)
        for call in (lambda: build_spatial_pairs(moved, md, fd, draws=dd, **kw), lambda: spatial_knn_pairs(moved, md),
                     lambda: spatial_negative_pairs(moved, md, 6.0, None, 4, draws=dd),
                     lambda: build_spatial_pairs_batched(moved, md.unsqueeze(0), fd.unsqueeze(0), [0, len(anchors)], draws=dd, **kw)):
            with pytest.raises(ValueError, match="an anchor lies outside the mask"):
                call()
    for value in (-1, 2 ** 31):
        off = dd.clone()
        off[5, 2] = value
        with pytest.raises(ValueError, match=r"draws must lie in \[0, 2\^31\)"):
            build_spatial_pairs(ad, md, fd, draws=off, **kw)
        with pytest.raises(ValueError, match=r"draws must lie in \[0, 2\^31\)"):
            spatial_negative_pairs(ad, md, 6.0, None, 4, draws=off)
    out = build_spatial_pairs(ad[:0], md, fd, **kw)                                       # no anchors: nothing is launched
    assert out["unique_coords"].shape == (0, 2) and out["pos_pairs"].shape == (0, 2) and out["stats"]["n_anchors"] == 0
