"""The restatement of anchor sampling (tests/anchor_cases.py) against the fixtures written by the REFERENCE's anchor_sampling.py
(tests/golden/make_anchor_golden.py): grids equal under the recorded jitter, supplement candidate sets equal as sets, inverse-frequency and
resolved weights array_equal; the law of the exponential race (first-pick frequencies, distinct picks, m = min(n, eligible), no
zero-weight pick, ties at the cut by pixel index); and the plain-Python layer of frl_hip.data.anchor_sampling, which needs no GPU:
resolve_supplement_weights on plain masks, AnchorSampler and build_anchor_sampler on SimpleNamespace configs and legacy dicts, and every
argument error, raised on CPU tensors before the library is called."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import anchor_cases as AC
from frl_hip import _lib
from frl_hip.data import anchor_sampling as A


@pytest.fixture(scope="module")
def grid_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anchor_grid.npz"))


@pytest.fixture(scope="module")
def sup_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anchor_supplement.npz"))


@pytest.fixture(scope="module")
def weight_fx(golden_dir):
    return np.load(os.path.join(golden_dir, "anchor_weights.npz"))


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------

def test_fixture_inputs_come_from_the_seeded_makers(grid_fx, sup_fx):
    for name, mask in AC.fixture_masks().items():
        assert np.array_equal(grid_fx[f"mask_{name}"], mask)
        assert np.array_equal(sup_fx[f"weights_{name}"], AC.fixture_weights()[name])
    assert grid_fx["mask_small"].shape == (24, 20) and grid_fx["mask_large"].shape == (70, 67)
    assert not grid_fx["mask_small"][6:13, 5:12].any()


@pytest.mark.parametrize("c", range(len(AC.GRID_CASES)))
def test_restatement_reproduces_the_reference_grids(grid_fx, c):
    name, stride, border, radius, seeds = AC.GRID_CASES[c]
    mask = grid_fx[f"mask_{name}"]
    seen = set()
    for seed in seeds:
        jr, jc = grid_fx[f"jitter_{c}_{seed}"].tolist()
        assert abs(jr) <= radius and abs(jc) <= radius
        seen |= {jr, jc}
        got = AC.grid(mask, stride, border, jr, jc)
        assert got.dtype == np.int64 and np.array_equal(got, grid_fx[f"grid_{c}_{seed}"].astype(np.int64)), (c, seed)
        assert A.grid_capacity(*mask.shape, stride, border, radius) >= len(got)
    assert {-radius, radius} <= seen
    if c == 2:
        assert A.grid_capacity(*mask.shape, stride, border, radius) == 4158 and 256 < len(grid_fx["grid_2_0"]) < 4158
    if c == 3:
        assert len(grid_fx["grid_3_0"]) == 0


def test_grid_without_a_row_is_empty_where_the_reference_raises():
    name, stride, border, radius = AC.RAISING_GRID
    mask = AC.fixture_masks()[name]
    assert len(AC.grid(mask, stride, border)) == 0 and A.grid_capacity(*mask.shape, stride, border, radius) == 0


@pytest.mark.parametrize("name", ["small", "large"])
def test_restatement_reproduces_the_reference_candidate_sets(grid_fx, sup_fx, name):
    mask, wgt = grid_fx[f"mask_{name}"], sup_fx[f"weights_{name}"]
    h, w = mask.shape
    n_valid = int(mask.sum())
    noise = AC.make_noise((h, w), 41)
    got = AC.keys_of(AC.supplement(mask, noise, n_valid + 5), w)
    assert len(got) == n_valid and set(got.tolist()) == set(sup_fx[f"all_{name}"].tolist())
    positive = sup_fx[f"positive_{name}"]
    for n in (len(positive), len(positive) + 7):                               # asked for more, the race still stops at the positive ones
        got = AC.keys_of(AC.supplement(mask, noise, n, wgt), w)
        assert len(got) == len(positive) and set(got.tolist()) == set(positive.tolist())
    got = AC.keys_of(AC.supplement(mask, noise, 10, np.zeros_like(wgt)), w)     # all-zero weights: uniform over the valid pixels
    ref = sup_fx[f"zero_{name}"]
    assert len(got) == len(ref) == 10 and len(set(got.tolist())) == 10 and mask.reshape(-1)[got].all() and mask.reshape(-1)[ref].all()
    assert np.array_equal(got, AC.keys_of(AC.supplement(mask, noise, 10), w))


@pytest.mark.parametrize("name", sorted(AC.invfreq_cases()))
def test_restatement_reproduces_the_reference_inverse_frequency(weight_fx, name):
    data, valid, listed = AC.invfreq_cases()[name]
    got = AC.inverse_frequency(data, valid, listed)
    assert got.dtype == np.float32 and np.array_equal(got, weight_fx[f"invfreq_{name}"])


def test_inverse_frequency_fixture_holds_what_it_is_there_for(weight_fx):
    codes, valid, listed = AC.invfreq_cases()["codes_listed"]
    out, out_listed = weight_fx["invfreq_codes"], weight_fx["invfreq_codes_listed"]
    zeros = valid & (codes == 0)
    assert np.signbit(codes[zeros]).any() and len(np.unique(out[zeros])) == 1 and out[zeros][0] == np.float32(1) / np.float32(zeros.sum())
    assert out[0, 4] > 0 and out[0, 4] == out[1, 0] and out[0, 4] != out[1, 2]                    # 2.5 is its own value ...
    assert out_listed[0, 4] > 0 and out_listed[0, 5] > 0 and out_listed[2, 2] > 0                 # ... listed as 2; 3.5 as 4; -2.5 as -2
    assert out_listed[2, 3] == 0 and 5 not in listed and (out_listed[valid & (codes == 5)] == 0).all()   # -3.5 as -4: not listed
    assert (out[1, 4:6] == 0).all() and (out[2, :2] == 0).all()                                  # NaN and inf
    many, large, _ = AC.invfreq_cases()["many"]
    assert len(np.unique(many[large & np.isfinite(many)])) > 550
    assert np.array_equal(weight_fx["invfreq_nothing_listed"], valid.astype(np.float32))
    assert not weight_fx["invfreq_nothing_valid"].any()


@pytest.mark.parametrize("name", sorted(AC.RESOLVE_CASES))
def test_restatement_reproduces_the_reference_resolved_weights(weight_fx, name):
    got = AC.resolve(AC.resolve_sample(), AC.RESOLVE_CASES[name])
    assert got.dtype == np.float32 and np.array_equal(got, weight_fx[f"resolve_{name}"])


# ---- the race -------------------------------------------------------------------------------------------------------------------------

def test_race_first_pick_follows_the_weights():
    wgt = np.asarray([[1, 2, 3, 0, 4, 0.5]], dtype=np.float32)
    noise = np.random.default_rng(1).standard_exponential((4096, 6)).astype(np.float32)
    mask = np.ones((1, 6), dtype=bool)
    first = np.asarray([AC.supplement(mask, noise[t:t + 1], 1, wgt)[0, 1] for t in range(4096)])
    p = wgt[0] / wgt.sum()
    freq = np.bincount(first, minlength=6) / 4096.0
    sd = np.sqrt(p * (1 - p) / 4096.0)
    worst = float(np.max(np.abs(freq - p)[p > 0] / sd[p > 0]))
    print(f"first-pick frequencies {freq}, expected {p}, worst deviation {worst:.2f} standard deviations")
    assert freq[3] == 0 and worst < 4.0


def test_race_picks_are_distinct_and_never_of_zero_weight():
    mask = AC.make_mask(24, 20, 51, invalid=0.3)
    wgt = AC.make_weights(24, 20, 52)
    noise = AC.make_noise((24, 20), 53)
    positive = int((mask & (wgt > 0)).sum())
    for n, weights, eligible in ((7, None, int(mask.sum())), (10 ** 4, None, int(mask.sum())), (7, wgt, positive), (positive + 3, wgt, positive),
                                 (0, wgt, positive)):
        rc = AC.supplement(mask, noise, n, weights)
        keys = AC.keys_of(rc, 20)
        assert len(rc) == min(n, eligible) and len(set(keys.tolist())) == len(keys) and mask[rc[:, 0], rc[:, 1]].all()
        if weights is not None:
            assert (weights[rc[:, 0], rc[:, 1]] > 0).all()
        _, key = AC.race_keys(mask, noise, weights)
        assert (np.diff(key[rc[:, 0], rc[:, 1]]) >= 0).all()
    assert len(AC.supplement(np.zeros((5, 7), dtype=bool), AC.make_noise((5, 7), 1), 4)) == 0


def test_race_ties_at_the_cut_resolve_by_pixel_index():
    mask = np.ones((4, 8), dtype=bool)
    mask[0, 1] = False
    noise = np.full((4, 8), 2.0, dtype=np.float32)
    noise[3, 7] = 0.5                                                           # one key below the tie group
    noise[0, 1] = 0.0                                                           # not valid: never picked
    rc = AC.supplement(mask, noise, 5)
    assert rc.tolist() == [[3, 7], [0, 0], [0, 2], [0, 3], [0, 4]]
    wgt = np.full((4, 8), 4.0, dtype=np.float32)
    wgt[1, 0] = 8.0                                                             # 2 / 8 beats 2 / 4 and loses to 0.5 / 4
    assert AC.supplement(mask, noise, 4, wgt).tolist() == [[3, 7], [1, 0], [0, 0], [0, 2]]


def test_batched_restatement_is_the_concatenation():
    masks = [AC.make_mask(24, 20, 61), np.zeros((24, 20), dtype=bool), AC.make_mask(24, 20, 62, invalid=0.5)]
    noise = AC.make_noise((3, 24, 20), 63)
    out = AC.sample_batched(masks, [(0, 0), (1, -1), (-2, 2)], noise, stride=4, border=4, supplement_n=6)
    assert out["offsets"][0] == 0 and out["offsets"][-1] == len(out["anchors"]) and out["stats"]["n_valid"][1] == 0
    assert out["offsets"][2] == out["offsets"][1] and out["stats"]["n_supplement"] == [6, 0, 6]
    a, b = out["offsets"][2], out["offsets"][3]
    assert np.array_equal(out["anchors"][a:b], np.concatenate([AC.grid(masks[2], 4, 4, -2, 2), AC.supplement(masks[2], noise[2], 6)]))


# ---- the package's plain-Python layer --------------------------------------------------------------------------------------------------

def test_resolve_supplement_weights_plain_masks_and_errors(weight_fx):
    sample = AC.resolve_sample()
    specs = [A.WeightSpec(channel=ch, transform=tr, valid_values=vv) for ch, tr, vv in AC.RESOLVE_CASES["masks_only"]]
    got = A.resolve_supplement_weights(sample, specs)                            # numpy planes, no transform: no kernel is needed
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), weight_fx["resolve_masks_only"])
    temporal = A.resolve_supplement_weights(sample, [A.WeightSpec("annual.cover")])
    assert np.array_equal(temporal.numpy(), sample["static_mask"][1])            # [T, H, W]: slice 0
    as_torch = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in sample.items()}
    assert torch.equal(A.resolve_supplement_weights(as_torch, specs), got)
    assert A.resolve_supplement_weights(sample, []) is None
    with pytest.raises(ValueError, match="unknown weight transform"):
        A.resolve_supplement_weights(sample, [A.WeightSpec("static_mask.aoi"), A.WeightSpec("static.ysfc_min", transform="inverse")])
    with pytest.raises(ValueError, match="group.channel"):
        A.resolve_supplement_weights(sample, [A.WeightSpec("aoi")])
    with pytest.raises(ValueError, match="no channel"):
        A.resolve_supplement_weights(sample, [A.WeightSpec("static_mask.water")])


def _parsed_config():
    grid = NS(stride=8, exclude_border=12, jitter=NS(radius=3))
    weighted = NS(grid=grid, supplement=NS(n=50, weight_by=[NS(mask_ref="static_mask.aoi", channel=None, transform=None),
                                                            NS(mask_ref=None, channel="static.ysfc_min", transform="inverse-frequency")]))
    bare = NS(grid=None, supplement=None)
    return NS(sampling_strategies={"grid": NS(grid=grid, supplement=None), "grid-plus-supplement": NS(grid=grid, supplement=NS(n=50, weight_by=None)),
                                   "grid-plus-supplement-ysfc": weighted, "grid-plus-supplement-bare": bare,
                                   "grid-plus-supplement-nojitter": NS(grid=NS(stride=8, exclude_border=12, jitter=None), supplement=None)})


def _params(s):
    return s.strategy, s.stride, s.border, s.jitter_radius, s.supplement_n


def test_build_anchor_sampler_parsed_config():
    cfg = _parsed_config()
    assert _params(A.build_anchor_sampler(cfg, "grid")) == ("grid", 8, 12, 3, 0)
    assert _params(A.build_anchor_sampler(cfg, "grid-plus-supplement")) == ("grid-plus-supplement", 8, 12, 3, 50)
    s = A.build_anchor_sampler(cfg, "grid-plus-supplement-ysfc")
    assert _params(s) == ("grid-plus-supplement-ysfc", 8, 12, 3, 50)
    assert s.weight_specs == [A.WeightSpec("static_mask.aoi"), A.WeightSpec("static.ysfc_min", transform="inverse-frequency")]
    assert _params(A.build_anchor_sampler(cfg, "grid-plus-supplement-bare")) == ("grid-plus-supplement-bare", 16, 16, 4, 104)
    assert _params(A.build_anchor_sampler(cfg, "grid-plus-supplement-nojitter")) == ("grid-plus-supplement-nojitter", 8, 12, 4, 104)
    assert _params(A.build_anchor_sampler(cfg, "grid-plus-supplement-absent")) == ("grid-plus-supplement-absent", 16, 16, 4, 104)
    assert A.build_anchor_sampler(cfg, "grid-plus-supplement-absent").weight_specs == []


def test_build_anchor_sampler_legacy_dict_and_defaults():
    legacy = NS(sampling_strategy={
        "grid": {"stride": 32, "exclude_border": 8, "jitter": {"radius": 2}},
        "grid-plus-supplement": {"grid": {"stride": 24}, "supplement": {"n": 12, "sampling": {
            "weight_by": ["static_mask.aoi", {"channel": "static.ysfc_min", "transform": "inverse-frequency"}]}}},
        "grid-plus-supplement-plain": {}})
    assert _params(A.build_anchor_sampler(legacy, "grid")) == ("grid", 32, 8, 2, 0)
    s = A.build_anchor_sampler(legacy, "grid-plus-supplement")
    assert _params(s) == ("grid-plus-supplement", 24, 16, 4, 12)
    assert s.weight_specs == [A.WeightSpec("static_mask.aoi"), A.WeightSpec("static.ysfc_min", transform="inverse-frequency")]
    assert _params(A.build_anchor_sampler(legacy, "grid-plus-supplement-plain")) == ("grid-plus-supplement-plain", 16, 16, 4, 104)
    with pytest.raises(ValueError, match="unknown sampling strategy"):
        A.build_anchor_sampler(legacy, "poisson")
    bad = NS(sampling_strategy={"grid-plus-supplement": {"supplement": {"sampling": {"weight_by": [{"transform": "inverse-frequency"}]}}}})
    with pytest.raises(ValueError, match="channel"):
        A.build_anchor_sampler(bad, "grid-plus-supplement")
    with pytest.raises(ValueError, match="weight_by entry"):
        A.build_anchor_sampler(NS(sampling_strategy={"grid-plus-supplement": {"supplement": {"sampling": {"weight_by": [3]}}}}),
                               "grid-plus-supplement")
    assert _params(A.build_anchor_sampler(NS(), "grid-plus-supplement")) == ("grid-plus-supplement", 16, 16, 4, 104)
    assert _params(A.build_anchor_sampler(None, "grid")) == ("grid", 16, 16, 4, 104)


def test_anchor_sampler_plumbing(monkeypatch):
    calls = []

    def fake(masks, **kw):
        calls.append((tuple(masks.shape), kw))
        return {"anchors": torch.zeros((0, 2), dtype=torch.long), "offsets": [0] * (masks.shape[0] + 1), "stats": {}}

    monkeypatch.setattr(A, "sample_anchors_batched", fake)
    mask = torch.ones(24, 20, dtype=torch.bool)
    s = A.AnchorSampler("grid-plus-supplement-x", stride=8, border=12, jitter_radius=3, supplement_n=50)
    assert s(mask).shape == (0, 2)
    assert calls[-1][0] == (1, 24, 20)
    assert {k: calls[-1][1][k] for k in ("stride", "border", "jitter_radius", "supplement_n", "weights")} == \
        dict(stride=8, border=12, jitter_radius=3, supplement_n=50, weights=None)
    s(mask, training=False)
    assert calls[-1][1]["jitter_radius"] == 0 and calls[-1][1]["supplement_n"] == 50
    A.AnchorSampler("grid", stride=8, border=12, jitter_radius=3, supplement_n=50)(mask)
    assert calls[-1][1]["supplement_n"] == 0 and calls[-1][1]["jitter_radius"] == 3
    out = s.batched(torch.ones(3, 24, 20, dtype=torch.bool), training=False, weights=torch.ones(3, 24, 20))
    assert calls[-1][0] == (3, 24, 20) and calls[-1][1]["jitter_radius"] == 0 and calls[-1][1]["weights"].shape == (3, 24, 20)
    assert out["offsets"] == [0, 0, 0, 0]
    # weight specs and a sample: the plain-mask product reaches the call as [1, H, W]
    sample = AC.resolve_sample()
    w = A.AnchorSampler("grid-plus-supplement", weight_specs=[A.WeightSpec("static_mask.aoi"), A.WeightSpec("static_mask.forest")])
    w(mask, sample=sample)
    assert np.array_equal(calls[-1][1]["weights"].numpy()[0], sample["static_mask"][0] * sample["static_mask"][1])
    w(mask)                                                                      # no sample: unweighted, as the reference
    assert calls[-1][1]["weights"] is None
    w.batched(torch.ones(2, 24, 20, dtype=torch.bool), samples=[sample, sample])
    assert calls[-1][1]["weights"].shape == (2, 24, 20)
    with pytest.raises(ValueError, match="2 masks but 1 samples"):
        w.batched(torch.ones(2, 24, 20, dtype=torch.bool), samples=[sample])
    n = len(calls)
    for call in (lambda: A.AnchorSampler("poisson")(mask), lambda: A.AnchorSampler("poisson").batched(mask.unsqueeze(0))):
        with pytest.raises(ValueError, match="unknown sampling strategy"):
            call()
    assert len(calls) == n


def test_argument_errors_are_raised_on_cpu_tensors_without_a_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "load", boom)
    masks = torch.ones(2, 24, 20, dtype=torch.bool)
    ok = dict(stride=4, border=4, jitter_radius=2, supplement_n=8)
    bad = [
        (dict(masks=masks.float()), "bool"), (dict(masks=masks[0]), "bool"), (dict(masks=masks[:0]), "bool"),
        (dict(masks=torch.ones(1, 1025, 4, dtype=torch.bool)), "must not exceed 1024"),
        (dict(stride=0), "stride"), (dict(jitter_radius=-1), "jitter_radius"), (dict(border=1), "border - jitter_radius"),
        (dict(border=1025), "border must not exceed"), (dict(supplement_n=-1), "supplement_n"), (dict(supplement_n=1025), "supplement_n"),
        (dict(masks=torch.ones(1, 400, 400, dtype=torch.bool), stride=1, border=2), "at most 16384 grid points"),
        (dict(weights=torch.ones(2, 24, 21)), "weights"), (dict(weights=torch.ones(2, 24, 20, dtype=torch.bool)), "weights"),
        (dict(jitter=torch.zeros(2, 3, dtype=torch.int64)), "jitter"), (dict(jitter=torch.zeros(2, 2)), "jitter"),
        (dict(jitter=torch.tensor([[0, 0], [3, 0]])), r"jitter must lie in \[-2, 2\]"),
        (dict(noise=torch.ones(2, 24, 20, dtype=torch.float64)), "noise"), (dict(noise=torch.ones(1, 24, 20)), "noise"),
    ]
    for change, match in bad:
        kw = dict(ok, **change)
        m = kw.pop("masks", masks)
        with pytest.raises(ValueError, match=match):
            A.sample_anchors_batched(m, **kw)
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):             # valid arguments, CPU tensors: no fallback
        A.sample_anchors_batched(masks, **ok)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        A.sample_anchors_grid(masks)
    with pytest.raises(ValueError, match="stride"):
        A.sample_anchors_grid(masks[0], stride=0)
    with pytest.raises(ValueError, match="supplement_n"):
        A.sample_anchors_grid_plus_supplement(masks[0], supplement_n=2000)
    with pytest.raises(_lib.FrlHipError):
        A.sample_anchors_grid_plus_supplement(masks[0], weights=torch.ones(24, 20), jitter=torch.tensor([0, 0]), noise=torch.ones(24, 20))
    data = torch.zeros(24, 20)
    for args, match in (((data.double(), masks[0]), "float32"), ((data, masks[0].float()), "valid_mask"), ((data, masks[0, :5]), "valid_mask"),
                        ((torch.zeros(1025, 4), torch.ones(1025, 4, dtype=torch.bool)), "at most"),
                        ((data, masks[0], range(5000)), "valid_values"), ((data, masks[0], [2 ** 31]), "valid_values")):
        with pytest.raises(ValueError, match=match):
            A.inverse_frequency_weights(*args)
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        A.inverse_frequency_weights(data, masks[0], {1, 2})
