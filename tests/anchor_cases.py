"""Seeded inputs and a numpy restatement of anchor sampling (frl/data/sampling/anchor_sampling.py), written from the definitions:

  grid        the points (border + jr + i stride, border + jc + j stride) with row < H - border and col < W - border, row-major, kept
              where the mask is True.
  supplement  eligible = valid pixels, with weights the valid pixels of positive weight (all valid pixels again when there is none, and
              the weights are then ignored); key = noise, or float32(noise / weight) with weights in use, its sign dropped; the picks are
              the m = min(n, eligible) eligible pixels of smallest (key, row * W + col), ascending.
  inverse     eligible = valid, finite and (with a whitelist) rint(value) listed; weight = float32(1) / float32(count of eligible pixels
  frequency   with an equal value), 0 elsewhere; no eligible pixel: 1 at the valid pixels.
  resolve     the product of the plain masks, then each transform on the pixels where that product is positive (finite pixels when there
              is no plain mask), then the product of both.
"""
import numpy as np

GRID_CASES = (  # (mask name, stride, border, jitter_radius, seeds)
    ("small", 4, 4, 0, (0,)),
    ("small", 4, 4, 2, tuple(range(16))),
    ("large", 1, 2, 0, (0,)),
    ("small", 16, 10, 0, (0,)),
)
# (16, 16, 0) on 24 x 20 has no grid row either, but the reference cannot say so: torch.arange refuses a start beyond its end
RAISING_GRID = ("small", 16, 16, 0)
SUPPLEMENT_GRID = {"small": dict(stride=16, border=10), "large": dict(stride=16, border=16)}    # the grid the supplement fixtures came with


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def make_mask(h, w, seed, invalid=0.1, hole=None):
    """bool [h, w]; `invalid` of the pixels are False at random, `hole` = (r0, r1, c0, c1) is False throughout."""
    mask = np.random.default_rng(seed).random((h, w)) >= invalid
    if hole is not None:
        mask[hole[0]:hole[1], hole[2]:hole[3]] = False
    return mask


def fixture_masks():
    """The masks of tests/golden/anchor_*.npz: 24 x 20 with a hole, and 70 x 67."""
    return {"small": make_mask(24, 20, 3101, invalid=0.2, hole=(6, 13, 5, 12)), "large": make_mask(70, 67, 3102, invalid=0.15)}


def make_noise(shape, seed):
    """float32 Exp(1) variates."""
    return np.random.default_rng(seed).standard_exponential(shape).astype(np.float32)


def make_weights(h, w, seed, zero=0.3):
    """float32 [h, w]: positive values over three decades, `zero` of them exactly 0 and a few negative."""
    rng = np.random.default_rng(seed)
    wgt = np.exp(rng.uniform(-3.0, 3.0, (h, w))).astype(np.float32)
    wgt[rng.random((h, w)) < zero] = 0.0
    wgt[rng.random((h, w)) < 0.05] = -1.5
    return wgt


def fixture_weights():
    return {name: make_weights(*m.shape, seed) for (name, m), seed in zip(fixture_masks().items(), (3111, 3112))}


def invfreq_cases():
    """name -> (data float32 [H, W], valid bool [H, W], valid_values or None)."""
    masks = fixture_masks()
    rng = np.random.default_rng(3121)
    small, large = masks["small"], masks["large"]
    codes = rng.integers(-3, 9, small.shape).astype(np.float32)
    codes[0, :6] = [0.0, -0.0, 0.0, -0.0, 2.5, 3.5]
    codes[1, :6] = [2.5, 3.5, 2.0, 4.0, np.nan, np.inf]
    codes[2, :4] = [-np.inf, np.nan, -2.5, -3.5]
    valid = small.copy()
    valid[:3, :6] = True
    many = (rng.integers(0, 600, large.shape) / 8.0).astype(np.float32)
    many[5, 5] = np.nan
    listed = {-3, -2, 0, 2, 4, 7}
    return {"codes_listed": (codes, valid, listed), "codes": (codes, valid, None), "many": (many, large, None),
            "nothing_listed": (codes, valid, {99}), "empty_list": (codes, valid, set()), "nothing_valid": (codes, np.zeros_like(valid), None)}


def resolve_sample():
    """A sample dict as the dataset returns it (numpy planes): static_mask [2, H, W] (aoi, forest), static [2, H, W] (ysfc_min, evt) and a
    temporal group [1, T, H, W]."""
    rng = np.random.default_rng(3131)
    h, w = 24, 20
    aoi = (rng.random((h, w)) < 0.8).astype(np.float32)
    forest = (rng.random((h, w)) < 0.7).astype(np.float32)
    ysfc = rng.integers(0, 12, (h, w)).astype(np.float32)
    ysfc[rng.random((h, w)) < 0.05] = np.nan
    evt = rng.integers(7000, 7012, (h, w)).astype(np.float32)
    return {"static_mask": np.stack([aoi, forest]), "static": np.stack([ysfc, evt]), "annual": np.stack([np.stack([forest, aoi])]),
            "metadata": {"channel_names": {"static_mask": ["aoi", "forest"], "static": ["ysfc_min", "evt"], "annual": ["cover"]}}}


RESOLVE_CASES = {  # name -> [(channel, transform, valid_values)]
    "masks_only": [("static_mask.aoi", None, None), ("static_mask.forest", None, None)],
    "mask_x_invfreq": [("static_mask.aoi", None, None), ("static.ysfc_min", "inverse-frequency", None)],
    "invfreq_only": [("static.ysfc_min", "inverse-frequency", None)],
    "masks_x_listed": [("static.evt", "inverse-frequency", {7001, 7002, 7005, 7011}), ("static_mask.aoi", None, None),
                       ("static_mask.forest", None, None)],
    "temporal_mask": [("annual.cover", None, None), ("static.ysfc_min", "inverse-frequency", None)],
}


# ---- restatement ----------------------------------------------------------------------------------------------------------------------

def grid(mask, stride, border, jr=0, jc=0):
    """-> int64 [G, 2]."""
    h, w = mask.shape
    pts = [(r, c) for r in range(border + jr, h - border, stride) for c in range(border + jc, w - border, stride) if mask[r, c]]
    return np.asarray(pts, dtype=np.int64).reshape(-1, 2)


def race_keys(mask, noise, weights=None):
    """-> (eligible bool [H, W], key float32 [H, W])."""
    noise = np.asarray(noise, dtype=np.float32)
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float32)
        positive = mask & (weights > 0)
        if positive.any():
            with np.errstate(all="ignore"):
                return positive, np.abs(noise / np.where(positive, weights, np.float32(1)))
    return mask.copy(), np.abs(noise)


def supplement(mask, noise, n, weights=None):
    """-> int64 [m, 2], the picks in ascending (key, pixel index)."""
    eligible, key = race_keys(mask, noise, weights)
    idx = np.nonzero(eligible.reshape(-1))[0]
    order = np.lexsort((idx, key.reshape(-1)[idx]))[:max(int(n), 0)]
    pick = idx[order]
    return np.stack([pick // mask.shape[1], pick % mask.shape[1]], axis=1).astype(np.int64).reshape(-1, 2)


def sample_batched(masks, jitter, noise, stride=16, border=16, supplement_n=104, weights=None):
    """-> the dict of frl_hip.data.sample_anchors_batched with a numpy `anchors`."""
    parts, offsets, stats = [], [0], {"n_grid": [], "n_supplement": [], "n_valid": []}
    for s, mask in enumerate(masks):
        g = grid(mask, stride, border, int(jitter[s][0]), int(jitter[s][1]))
        p = supplement(mask, noise[s], supplement_n, None if weights is None else weights[s]) if supplement_n else np.zeros((0, 2), np.int64)
        parts += [g, p]
        offsets.append(offsets[-1] + len(g) + len(p))
        stats["n_grid"].append(len(g))
        stats["n_supplement"].append(len(p))
        stats["n_valid"].append(int(mask.sum()))
    return {"anchors": np.concatenate(parts, axis=0).reshape(-1, 2), "offsets": offsets, "stats": stats}


def inverse_frequency(data, valid, valid_values=None):
    """-> float32 [H, W]."""
    data = np.asarray(data, dtype=np.float32)
    eligible = valid & np.isfinite(data)
    if valid_values is not None:
        with np.errstate(invalid="ignore"):
            r = np.rint(data)                                                        # half to even
        inside = np.isfinite(r) & (np.abs(r) < 2.0 ** 31)
        code = np.where(inside, r, 0).astype(np.int64)
        eligible &= inside & np.isin(code, np.asarray(sorted(int(v) for v in valid_values), dtype=np.int64))
    if not eligible.any():
        return valid.astype(np.float32)
    vals = data[eligible]
    vals = np.where(vals == 0, np.float32(0), vals)                                  # -0.0 and 0.0 are one value
    _, inverse, counts = np.unique(vals, return_inverse=True, return_counts=True)
    out = np.zeros(data.shape, dtype=np.float32)
    out[eligible] = np.float32(1) / counts[inverse.reshape(-1)].astype(np.float32)
    return out


def channel(sample, ref):
    group, name = ref.split(".")
    plane = np.asarray(sample[group][sample["metadata"]["channel_names"][group].index(name)], dtype=np.float32)
    return plane[0] if plane.ndim == 3 else plane


def resolve(sample, specs):
    """specs: [(channel, transform, valid_values)] -> float32 [H, W]."""
    product = None
    for ch, transform, _ in specs:
        if transform is None:
            product = channel(sample, ch) if product is None else product * channel(sample, ch)
    for ch, transform, listed in specs:
        if transform is None:
            continue
        plane = channel(sample, ch)
        w = inverse_frequency(plane, product > 0 if product is not None else np.isfinite(plane), listed)
        product = w if product is None else product * w
    return product


def keys_of(coords, w):
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    return coords[:, 0] * w + coords[:, 1]
