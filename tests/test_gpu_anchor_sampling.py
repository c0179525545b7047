"""GPU parity of anchor sampling (csrc/anchors.hip behind frl_hip.data.sample_anchors_batched and the reference-shaped wrappers) against
the restatement (tests/anchor_cases.py, pinned to the REFERENCE's fixtures by tests/test_cpu_anchor_sampling.py) under explicit jitter and
noise, and against those fixtures directly.  Everything compared is an integer or a correctly rounded float32 quotient: equality
throughout, order included.

The select kernel does not switch path by size: it forms the keys once and re-reads them in every pass at every size.  What changes with
the size is the number of rounds a thread makes (one below 1024 pixels: 5 x 7 and 24 x 20; several above, more than one batch of eight
from 130 x 129 on) and whether the last round is partial (every shape here).  It does switch by data: when every pixel at the cut is
taken (distinct keys: the generic cases, low_byte at some sizes) the winners claim slots in any order, and when the cut falls inside a
group of equal keys (duplicates, one_value, zeros, inf_keys) the collection walks in pixel order; both sides are named in `_special`."""
import functools
import os

import numpy as np
import pytest
import torch

import anchor_cases as AC
import spatial_pairs_cases as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name -> (H, W, invalid fraction): dense masks have more than 1024 valid pixels from 70 x 67 on, the sparse ones fewer
VARIANTS = {
    "5x7": (5, 7, 0.1), "24x20": (24, 20, 0.1), "70x67": (70, 67, 0.1), "70x67_sparse": (70, 67, 0.9), "130x129": (130, 129, 0.1),
    "130x129_sparse": (130, 129, 0.97), "260x257": (260, 257, 0.1), "260x257_sparse": (260, 257, 0.99),
}
GRID = dict(stride=3, border=2)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _data():
    from frl_hip import data
    return data


def _run(masks, jitter, noise, weights=None, radius=2, **kw):
    """One batched call on numpy inputs -> its dict."""
    return _data().sample_anchors_batched(_dev(np.stack(masks)), jitter_radius=radius, jitter=_dev(np.asarray(jitter, dtype=np.int64)),
                                          noise=None if noise is None else _dev(np.stack(noise)),
                                          weights=None if weights is None else _dev(np.stack(weights)), **kw)


def _same(got, want, what):
    assert got["anchors"].dtype == torch.int64 and got["anchors"].is_cuda and got["anchors"].shape == want["anchors"].shape, what
    assert torch.equal(got["anchors"].cpu(), torch.from_numpy(want["anchors"])), f"{what}: anchors differ from the restatement's"
    assert list(got["offsets"]) == list(want["offsets"]) and all(isinstance(o, int) for o in got["offsets"]), what
    assert got["stats"] == want["stats"], what


@functools.lru_cache(maxsize=None)
def _variant(name):
    h, w, invalid = VARIANTS[name]
    seed = 4000 + 10 * sorted(VARIANTS).index(name)
    return AC.make_mask(h, w, seed, invalid=invalid), AC.make_noise((h, w), seed + 1), AC.make_weights(h, w, seed + 2)


def _counts(eligible):
    ns = {0, 1, 104, 1024}
    if eligible + 1 <= 1024:
        ns |= {eligible - 1, eligible, eligible + 1}
    return sorted(n for n in ns if n >= 0)


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_single_sample_equals_the_restatement(name, weighted):
    mask, noise, wgt = _variant(name)
    weights = wgt if weighted else None
    eligible = int((mask & (wgt > 0)).sum()) if weighted else int(mask.sum())
    assert eligible > 1 and (("sparse" in name or mask.size < 1024) == (eligible + 1 <= 1024))
    for i, n in enumerate(_counts(eligible)):
        jitter = [((-2, 2), (2, -2), (0, 1))[i % 3]]
        got = _run([mask], jitter, [noise], None if weights is None else [weights], supplement_n=n, **GRID)
        want = AC.sample_batched([mask], jitter, [noise], supplement_n=n, weights=None if weights is None else [weights], **GRID)
        _same(got, want, f"{name} n={n}")
        assert got["stats"]["n_supplement"] == [min(n, eligible)]


def _special(name):
    """-> (mask, noise, weights or None, the supplement sizes, a check on what the case is there for)."""
    h, w = 70, 67
    rng = np.random.default_rng(4200)
    mask = AC.make_mask(h, w, 4201, invalid=0.1)
    if name == "low_byte":                      # keys that differ only in their lowest byte: every radix pass decides
        noise = (np.uint32(0x3f800000) | rng.integers(0, 256, (h, w)).astype(np.uint32)).view(np.float32)
        return mask, noise, None, (1, 104, 1000), lambda: len(np.unique(noise.view(np.uint32) >> 8)) == 1
    if name == "high_byte":                     # keys that differ only in their highest byte
        noise = (rng.integers(1, 0x7f, (h, w)).astype(np.uint32) << 24).view(np.float32)
        return mask, noise, None, (1, 104, 1000), lambda: bool(np.isfinite(noise).all() and (noise > 0).all())
    if name == "duplicates":                    # three values: the cut falls inside a tie group spread over every wave
        noise = rng.choice(np.asarray([0.5, 1.0, 2.0], dtype=np.float32), (h, w))
        return mask, noise, None, (104, 1024), lambda: int((mask & (noise == 0.5)).sum()) > 1024
    if name == "one_value":
        return mask, np.ones((h, w), dtype=np.float32), None, (1, 104, 1024), lambda: True
    if name == "zeros":                         # a third of the noise is 0, one of them -0.0
        noise = AC.make_noise((h, w), 4202)
        noise[rng.random((h, w)) < 0.33] = 0.0
        first = np.nonzero(mask & (noise == 0))
        noise[first[0][5], first[1][5]] = -0.0
        return mask, noise, AC.make_weights(h, w, 4203, zero=0.1), (104, 1024), lambda: int((mask & (noise == 0)).sum()) > 1024
    if name == "inf_keys":                      # weights so small that noise / w overflows: the cut falls among the infinite keys
        mask = AC.make_mask(h, w, 4204, invalid=0.7)
        noise = AC.make_noise((h, w), 4205) + np.float32(0.01)
        wgt = np.where(rng.random((h, w)) < 0.5, np.float32(1e-45), np.float32(1.0)).astype(np.float32)
        with np.errstate(over="ignore"):
            key = noise / wgt
        finite, positive = int((mask & np.isfinite(key)).sum()), int(mask.sum())
        return mask, noise, wgt, (1024,), lambda: finite < 1024 < positive
    if name == "zero_weights":                  # no positive weight: the draw falls back to uniform over the valid pixels
        return mask, AC.make_noise((h, w), 4206), np.zeros((h, w), dtype=np.float32), (104,), lambda: True
    if name == "nonpositive_weights":
        return mask, AC.make_noise((h, w), 4207), -np.abs(AC.make_weights(h, w, 4208)), (104,), lambda: True
    if name == "few_positive":                  # fewer pixels of positive weight than supplement_n
        wgt = np.zeros((h, w), dtype=np.float32)
        ys, xs = np.nonzero(mask)
        wgt[ys[::97], xs[::97]] = 2.0
        return mask, AC.make_noise((h, w), 4209), wgt, (104,), lambda: 1 < int((mask & (wgt > 0)).sum()) < 104
    if name == "all_false":
        return np.zeros((h, w), dtype=bool), AC.make_noise((h, w), 4210), None, (0, 8), lambda: True
    raise KeyError(name)


SPECIAL = ("low_byte", "high_byte", "duplicates", "one_value", "zeros", "inf_keys", "zero_weights", "nonpositive_weights", "few_positive",
           "all_false")


@pytest.mark.parametrize("name", SPECIAL)
def test_special_noise_masks_and_weights_equal_the_restatement(name):
    mask, noise, weights, counts, there_for = _special(name)
    assert there_for(), name
    for n in counts:
        got = _run([mask], [(0, 0)], [noise], None if weights is None else [weights], radius=0, supplement_n=n, **GRID)
        want = AC.sample_batched([mask], [(0, 0)], [noise], supplement_n=n, weights=None if weights is None else [weights], **GRID)
        _same(got, want, f"{name} n={n}")
    if name in ("zero_weights", "nonpositive_weights"):
        plain = _run([mask], [(0, 0)], [noise], None, radius=0, supplement_n=104, **GRID)
        assert torch.equal(got["anchors"], plain["anchors"])
    if name == "few_positive":
        assert got["stats"]["n_supplement"] == [int((mask & (weights > 0)).sum())]
    if name == "all_false":
        assert got["anchors"].shape == (0, 2) and got["offsets"] == [0, 0] and got["stats"]["n_valid"] == [0]


@functools.lru_cache(maxsize=None)
def _batch():
    h, w = 70, 67
    masks = [AC.make_mask(h, w, 4300 + s, invalid=0.2) for s in range(5)]
    masks[2] = np.zeros((h, w), dtype=bool)
    weights = [AC.make_weights(h, w, 4310 + s) for s in range(5)]
    weights[3] = np.zeros((h, w), dtype=np.float32)
    noise = list(AC.make_noise((5, h, w), 4320))
    jitter = [(2, 2), (-2, -2), (0, 1), (-2, 2), (1, 0)]
    kw = dict(stride=8, border=4, supplement_n=20)
    return masks, weights, noise, jitter, kw, AC.sample_batched(masks, jitter, noise, weights=weights, **kw)


def test_batched_equals_the_single_calls_and_the_restatement():
    masks, weights, noise, jitter, kw, want = _batch()
    got = _run(masks, jitter, noise, weights, **kw)
    _same(got, want, "batched")
    assert want["stats"]["n_valid"][2] == 0 and want["offsets"][2] == want["offsets"][3] and want["stats"]["n_supplement"][3] == 20
    D = _data()
    for s in range(5):
        one = D.sample_anchors_grid_plus_supplement(_dev(masks[s]), kw["stride"], kw["border"], 2, kw["supplement_n"], _dev(weights[s]),
                                                    jitter=_dev(np.asarray(jitter[s], dtype=np.int64)), noise=_dev(noise[s]))
        assert torch.equal(one, got["anchors"][got["offsets"][s]:got["offsets"][s + 1]]), s
        g = D.sample_anchors_grid(_dev(masks[s]), kw["stride"], kw["border"], 2, jitter=_dev(np.asarray(jitter[s], dtype=np.int64)))
        assert torch.equal(g, one[:want["stats"]["n_grid"][s]])


def test_batched_result_feeds_the_spatial_pair_miner():
    from frl_hip.losses import build_spatial_pairs_batched
    masks, weights, noise, jitter, kw, _ = _batch()
    got = _run(masks, jitter, noise, weights, **kw)
    n = got["anchors"].shape[0]
    feats = np.stack([SP.make_feat(4, 70, 67, 4330 + s) for s in range(5)])
    draws = SP.make_draws(n, 4, 4340)
    params = dict(k=4, max_radius=8, min_distance=16.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.0625)
    pairs = build_spatial_pairs_batched(got["anchors"], _dev(np.stack(masks)), _dev(feats), got["offsets"], draws=_dev(draws), **params)
    want = SP.build_batched(got["anchors"].cpu().numpy(), masks, feats, got["offsets"], draws, **params)
    assert pairs["stats"]["n_anchors"] == [b - a for a, b in zip(got["offsets"][:-1], got["offsets"][1:])]
    for key in ("unique_coords", "anchor_to_unique", "pos_pairs", "neg_pairs"):
        assert np.array_equal(pairs[key].cpu().numpy(), want[key]), key


# ---- the reference's fixtures ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f"anchor_{k}.npz")) for k in ("grid", "supplement", "weights")}


def test_grids_equal_the_reference(fx):
    D = _data()
    for c, (name, stride, border, radius, seeds) in enumerate(AC.GRID_CASES):
        mask = _dev(fx["grid"][f"mask_{name}"])
        for seed in seeds:
            got = D.sample_anchors_grid(mask, stride, border, radius, jitter=_dev(fx["grid"][f"jitter_{c}_{seed}"].astype(np.int64)))
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), fx["grid"][f"grid_{c}_{seed}"]), (c, seed)
    name, stride, border, radius = AC.RAISING_GRID                                # the reference raises here; no grid row is no anchor
    assert D.sample_anchors_grid(_dev(fx["grid"][f"mask_{name}"]), stride, border, radius).shape == (0, 2)


@pytest.mark.parametrize("name", ["small", "large"])
def test_supplement_candidate_sets_equal_the_reference(fx, name):
    D = _data()
    mask, wgt = fx["grid"][f"mask_{name}"], fx["supplement"][f"weights_{name}"]
    h, w = mask.shape
    kw = dict(AC.SUPPLEMENT_GRID[name], supplement_n=1024)
    n_grid = len(AC.grid(mask, **AC.SUPPLEMENT_GRID[name]))
    for key, weights in (("all", None), ("positive", wgt)):
        want = fx["supplement"][f"{key}_{name}"]
        parts = []                                                                # 1024 picks per call: cover the set with disjoint masks
        for lo in range(0, len(want), 1024):
            part = np.zeros(h * w, dtype=bool)
            part[want[lo:lo + 1024]] = True
            sub = mask & part.reshape(h, w) if weights is None else mask
            sub_w = None if weights is None else np.where(part.reshape(h, w), weights, np.float32(0))
            out = D.sample_anchors_grid_plus_supplement(_dev(sub), weights=None if sub_w is None else _dev(sub_w),
                                                        noise=_dev(AC.make_noise((h, w), 4400 + lo)), **kw)
            parts.append(AC.keys_of(out.cpu().numpy()[len(AC.grid(sub, **AC.SUPPLEMENT_GRID[name])):], w))
        got = np.concatenate(parts)
        assert len(got) == len(want) and set(got.tolist()) == set(want.tolist()), (name, key)
    if name == "small":                                                           # small enough for one call each
        for key, weights in (("all", None), ("positive", wgt)):
            out = D.sample_anchors_grid_plus_supplement(_dev(mask), weights=None if weights is None else _dev(weights),
                                                        noise=_dev(AC.make_noise((h, w), 4450)), **kw)
            assert set(AC.keys_of(out.cpu().numpy()[n_grid:], w).tolist()) == set(fx["supplement"][f"{key}_{name}"].tolist())


def test_inverse_frequency_and_resolved_weights_equal_the_reference(fx):
    D = _data()
    for name, (data, valid, listed) in AC.invfreq_cases().items():
        got = D.inverse_frequency_weights(_dev(data), _dev(valid), listed)
        assert got.dtype == torch.float32 and got.shape == data.shape
        assert np.array_equal(got.cpu().numpy(), fx["weights"][f"invfreq_{name}"]), name
    codes, valid, listed = AC.invfreq_cases()["codes_listed"]
    both = D.inverse_frequency_weights(_dev(np.stack([codes, codes])), _dev(np.stack([valid, np.zeros_like(valid)])), listed).cpu().numpy()
    assert np.array_equal(both[0], fx["weights"]["invfreq_codes_listed"]) and not both[1].any()
    sample = AC.resolve_sample()
    for name, specs in AC.RESOLVE_CASES.items():
        got = D.resolve_supplement_weights(sample, [D.WeightSpec(channel=ch, transform=tr, valid_values=vv) for ch, tr, vv in specs], device=DEV)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), fx["weights"][f"resolve_{name}"]), name


def test_inverse_frequency_distinct_value_limit():
    D = _data()
    valid = _dev(np.ones((70, 67), dtype=bool))
    ramp = np.arange(70 * 67, dtype=np.float32).reshape(70, 67)
    at_limit = D.inverse_frequency_weights(_dev(np.minimum(ramp, 4095)), valid).cpu().numpy()          # 4096 distinct values
    assert np.array_equal(at_limit, AC.inverse_frequency(np.minimum(ramp, 4095), np.ones((70, 67), dtype=bool)))
    with pytest.raises(ValueError, match="distinct"):
        D.inverse_frequency_weights(_dev(np.minimum(ramp, 4096)), valid)                                 # 4097


def test_anchor_sampler_with_weight_specs_on_the_gpu(fx):
    D = _data()
    sample = AC.resolve_sample()
    specs = [D.WeightSpec(channel=ch, transform=tr, valid_values=vv) for ch, tr, vv in AC.RESOLVE_CASES["mask_x_invfreq"]]
    sampler = D.AnchorSampler("grid-plus-supplement-ysfc", stride=4, border=4, jitter_radius=2, supplement_n=30, weight_specs=specs)
    mask = AC.make_mask(24, 20, 4500)
    noise = AC.make_noise((24, 20), 4501)
    got = sampler(_dev(mask), training=True, sample=sample, jitter=_dev(np.asarray([-2, 1])), noise=_dev(noise))
    want = AC.sample_batched([mask], [(-2, 1)], [noise], stride=4, border=4, supplement_n=30, weights=[fx["weights"]["resolve_mask_x_invfreq"]])
    assert torch.equal(got.cpu(), torch.from_numpy(want["anchors"]))
    both = sampler.batched(_dev(np.stack([mask, mask])), training=False, samples=[sample, sample], noise=_dev(np.stack([noise, noise])))
    want = AC.sample_batched([mask], [(0, 0)], [noise], stride=4, border=4, supplement_n=30, weights=[fx["weights"]["resolve_mask_x_invfreq"]])
    half = both["offsets"][1]
    assert both["offsets"] == [0, half, 2 * half] and torch.equal(both["anchors"][:half].cpu(), torch.from_numpy(want["anchors"]))
    assert torch.equal(both["anchors"][:half], both["anchors"][half:])


# ---- the default random path and the errors at the host read ---------------------------------------------------------------------------

def test_default_random_inputs():
    D = _data()
    mask = AC.make_mask(70, 67, 4600, invalid=0.3)
    masks = _dev(np.stack([mask, mask]))
    kw = dict(stride=8, border=8, jitter_radius=4, supplement_n=50)

    def draw(seed):
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        return D.sample_anchors_batched(masks, generator=g, **kw)

    a, b, c = draw(7), draw(7), draw(8)
    assert torch.equal(a["anchors"], b["anchors"]) and a["offsets"] == b["offsets"]
    rc = a["anchors"].cpu().numpy()
    assert mask[rc[:, 0], rc[:, 1]].all()
    for s in range(2):
        lo, hi = a["offsets"][s] + a["stats"]["n_grid"][s], a["offsets"][s + 1]
        sup = AC.keys_of(rc[lo:hi], 67)
        assert len(sup) == 50 and len(set(sup.tolist())) == 50
        lo_c = c["offsets"][s] + c["stats"]["n_grid"][s]
        assert set(sup.tolist()) != set(AC.keys_of(c["anchors"].cpu().numpy()[lo_c:c["offsets"][s + 1]], 67).tolist())
    first = [set(AC.keys_of(rc[a["offsets"][s] + a["stats"]["n_grid"][s]:a["offsets"][s + 1]], 67).tolist()) for s in range(2)]
    assert first[0] != first[1]                                                   # the two samples get noise of their own
    assert a["stats"]["n_valid"] == [int(mask.sum())] * 2


def test_errors_at_the_host_read():
    mask = AC.make_mask(24, 20, 4700)
    mask[0, 0], mask[0, 1] = True, False
    noise = AC.make_noise((24, 20), 4701)
    wgt = np.abs(AC.make_weights(24, 20, 4702)) + np.float32(0.5)
    kw = dict(supplement_n=8, **GRID)
    for bad in (np.nan, np.inf):
        inside, outside = wgt.copy(), wgt.copy()
        inside[0, 0], outside[0, 1] = bad, bad
        with pytest.raises(ValueError, match="not finite"):
            _run([mask], [(0, 0)], [noise], [inside], **kw)
        _same(_run([mask], [(0, 0)], [noise], [outside], **kw), AC.sample_batched([mask], [(0, 0)], [noise], weights=[outside], **kw), "outside")
    for jitter in ((3, 0), (0, -3), (2 ** 40, 0)):
        with pytest.raises(ValueError, match=r"jitter must lie in \[-2, 2\]"):
            _run([mask], [jitter], [noise], **kw)
    for bad in (-1.0, np.nan):
        inside, outside = noise.copy(), noise.copy()
        inside[0, 0], outside[0, 1] = bad, bad
        with pytest.raises(ValueError, match="noise"):
            _run([mask], [(0, 0)], [inside], **kw)
        _run([mask], [(0, 0)], [outside], **kw)
