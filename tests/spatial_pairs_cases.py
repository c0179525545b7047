"""Seeded inputs and a numpy / torch-CPU restatement of spatial InfoNCE pair mining (frl/training/representation/step.py:325-401 with
spatial_knn_pairs and spatial_negative_pairs of frl/utils/spatial.py), written from the formulas:

  neighbours  the first min(k, count) offsets (dr, dc) in [-R, R]^2 with 0 < dr^2 + dc^2 <= R^2, ordered by (dr^2 + dc^2, (dr + R)(2R + 1)
              + dc + R); a pair per offset whose pixel is inside the mask and valid; anchor-major, offset order.
  candidates  the valid pixels whose float32 distance sqrt(float32(d2)) to the anchor is >= float32(min_distance) and <=
              float32(max_distance), in row-major order.  `thresholds` turns that into integer bounds lo <= d2 <= hi by a table of
              float32 square roots of every possible d2 (not by the package's bisection).
  picks       m = min(n, cnt); draw j has the rank q = (draw_j * (cnt - j)) >> 31 among the remaining candidates; going through the earlier
              picks in ascending order, q += 1 while q >= the pick; pick j is the candidate of that rank.  Draw order.
  mapping     torch.unique(cat([anchors, neighbours, negatives]), dim=0, return_inverse=True), as step.py forms it; `bitmap_rank` is the
              kernel's route to the same thing (set bits of an H x W bitmap, rank = set bits below the key).
  weights     d = |f_a - f_b|_2 over the channels of the map, exp(-d / tau) and 1 - exp(-d / tau) clamped to [min_w, 1], in float64.
"""
import numpy as np
import torch

DEFAULTS = dict(k=4, max_radius=8, min_distance=16.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.05)
FIXTURE_SHAPE, FIXTURE_ANCHORS, FIXTURE_RADIUS = (24, 20), 40, 8
FIXTURE_K = (4, 8, 12)
FIXTURE_NEG = ((6.0, None), (6.0, 9.5), (5.0, 5.0), (40.0, None), (6.1, 12.3))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def make_mask(h, w, seed, invalid=0.1, hole=None):
    """bool [h, w]; `invalid` of the pixels are False at random, `hole` = (r0, r1, c0, c1) is False throughout."""
    mask = np.random.default_rng(seed).random((h, w)) >= invalid
    if hole is not None:
        mask[hole[0]:hole[1], hole[2]:hole[3]] = False
    return mask


def make_anchors(h, w, n, seed):
    """int64 [n, 2]: the four corners and the four edge midpoints first, then random pixels (valid or not); from ten anchors on the last
    one repeats the first random one (a duplicate anchor)."""
    fixed = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    rng = np.random.default_rng(seed)
    rows = fixed[:n] + [(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(max(0, n - len(fixed)))]
    if n >= 10:
        rows[-1] = rows[8]
    return np.asarray(rows, dtype=np.int64).reshape(n, 2)


def make_feat(c, h, w, seed, span=96):
    """float32 [c, h, w] on the 2^-8 grid, values within span * 2^-8 of zero, every squared distance between two pixels below 256: float32
    sums of the squares are exact.  The default span keeps most distances below 2, where the weights are not clamped."""
    b = min(int(span), int(2047 / np.sqrt(c)) - 1)
    assert c * (2 * b / 256.0) ** 2 < 256.0
    return (np.random.default_rng(seed).integers(-b, b + 1, (c, h, w)) / 256.0).astype(np.float32)


def make_draws(n, n_per, seed):
    """int64 [n, n_per] in [0, 2^31), with the two extremes planted in the first rows."""
    d = np.random.default_rng(seed).integers(0, 2 ** 31, (n, n_per)).astype(np.int64)
    d[0, :] = 0
    if n > 1:
        d[1, :] = 2 ** 31 - 1
    if n > 2:
        d[2, ::2] = 0
        d[2, 1::2] = 2 ** 31 - 1
    return d


def fixture_inputs():
    """The inputs of tests/golden/spatial_*.npz: a 24 x 20 mask, a quarter invalid and with a hole, and 40 anchors."""
    h, w = FIXTURE_SHAPE
    return make_mask(h, w, 2401, invalid=0.25, hole=(3, 12, 2, 14)), make_anchors(h, w, FIXTURE_ANCHORS, 2402)


# ---- restatement ----------------------------------------------------------------------------------------------------------------------

def offsets(k, max_radius):
    r = max_radius
    cells = [(dr, dc) for dr in range(-r, r + 1) for dc in range(-r, r + 1) if 0 < dr * dr + dc * dc <= r * r]
    cells.sort(key=lambda o: (o[0] ** 2 + o[1] ** 2, (o[0] + r) * (2 * r + 1) + o[1] + r))
    return cells[:k]


def thresholds(min_distance, max_distance, h, w):
    """-> (lo, hi), lo > hi when no squared distance qualifies; from the table of float32 roots of 0..(h - 1)^2 + (w - 1)^2."""
    top = (h - 1) ** 2 + (w - 1) ** 2
    root = np.sqrt(np.arange(top + 1).astype(np.float32))
    above = np.nonzero(root >= np.float32(min_distance))[0]
    lo = int(above[0]) if len(above) else top + 1
    if max_distance is None:
        return lo, top
    below = np.nonzero(root <= np.float32(max_distance))[0]
    return lo, int(below[-1]) if len(below) else -1


def candidates(mask, r, c, lo, hi):
    """Keys y * W + x of the candidates of anchor (r, c), row-major (ascending)."""
    ys, xs = np.nonzero(mask)
    d2 = (ys - r) ** 2 + (xs - c) ** 2
    sel = (d2 >= lo) & (d2 <= hi)
    return (ys * mask.shape[1] + xs)[sel].astype(np.int64)


def pick_ranks(cnt, draws, n):
    picks = []
    for j in range(min(n, cnt)):
        q = (int(draws[j]) * (cnt - j)) >> 31
        for p in sorted(picks):
            if q >= p:
                q += 1
            else:
                break
        picks.append(q)
    return picks


def knn_pairs(anchors, mask, k=4, max_radius=8):
    """-> (anchor_indices [M] int64, neighbor_coords [M, 2] int64)."""
    h, w = mask.shape
    idx, rc = [], []
    for i, (r, c) in enumerate(np.asarray(anchors).tolist()):
        for dr, dc in offsets(k, max_radius):
            y, x = r + dr, c + dc
            if 0 <= y < h and 0 <= x < w and mask[y, x]:
                idx.append(i)
                rc.append((y, x))
    return np.asarray(idx, dtype=np.int64), np.asarray(rc, dtype=np.int64).reshape(-1, 2)


def negative_pairs(anchors, mask, draws, min_distance=16.0, max_distance=None, n_per_anchor=4):
    h, w = mask.shape
    lo, hi = thresholds(min_distance, max_distance, h, w)
    idx, rc = [], []
    for i, (r, c) in enumerate(np.asarray(anchors).tolist()):
        cand = candidates(mask, r, c, lo, hi)
        for q in pick_ranks(len(cand), draws[i], n_per_anchor):
            idx.append(i)
            rc.append((int(cand[q]) // w, int(cand[q]) % w))
    return np.asarray(idx, dtype=np.int64), np.asarray(rc, dtype=np.int64).reshape(-1, 2)


def bitmap_rank(coords, h, w):
    """coords [M, 2] -> (sorted unique coords [U, 2], inverse [M]) by the bitmap route."""
    keys = coords[:, 0] * w + coords[:, 1]
    bitmap = np.zeros(h * w, dtype=np.int64)
    bitmap[keys] = 1
    below = np.cumsum(bitmap) - bitmap
    set_keys = np.nonzero(bitmap)[0]
    return np.stack([set_keys // w, set_keys % w], axis=1).astype(np.int64), below[keys].astype(np.int64)


def build(anchors, mask, feat, draws, k=4, max_radius=8, min_distance=16.0, max_distance=None, n_per_anchor=4, tau=1.0, min_w=0.05):
    """One sample -> the dict of losses.build_spatial_pairs with numpy arrays, weights and distances in float64."""
    anchors = np.asarray(anchors, dtype=np.int64).reshape(-1, 2)
    n = anchors.shape[0]
    pos_a, pos_rc = knn_pairs(anchors, mask, k, max_radius)
    neg_a, neg_rc = negative_pairs(anchors, mask, draws, min_distance, max_distance, n_per_anchor)
    parts = [torch.from_numpy(anchors)]
    if pos_rc.size:
        parts.append(torch.from_numpy(pos_rc))
    if neg_rc.size:
        parts.append(torch.from_numpy(neg_rc))
    unique, inverse = torch.unique(torch.cat(parts, dim=0), dim=0, return_inverse=True)
    unique, inverse = unique.numpy().reshape(-1, 2), inverse.numpy()
    a2u = inverse[:n]
    n_pos, n_neg = pos_rc.shape[0], neg_rc.shape[0]
    pos_pairs = np.stack([a2u[pos_a], inverse[n:n + n_pos]], axis=1).reshape(-1, 2)
    neg_pairs = np.stack([a2u[neg_a], inverse[n + n_pos:]], axis=1).reshape(-1, 2)
    f = np.asarray(feat, dtype=np.float64)[:, unique[:, 0], unique[:, 1]].T if len(unique) else np.zeros((0, feat.shape[0]))
    dpos = np.sqrt(((f[pos_pairs[:, 0]] - f[pos_pairs[:, 1]]) ** 2).sum(axis=1))
    dneg = np.sqrt(((f[neg_pairs[:, 0]] - f[neg_pairs[:, 1]]) ** 2).sum(axis=1))
    return {"unique_coords": unique, "unique_offsets": [0, len(unique)], "anchor_to_unique": a2u, "pos_pairs": pos_pairs, "neg_pairs": neg_pairs,
            "pos_offsets": [0, n_pos], "neg_offsets": [0, n_neg], "pos_dist": dpos, "neg_dist": dneg,
            "pos_raw": np.exp(-dpos / tau), "neg_raw": 1.0 - np.exp(-dneg / tau),
            "pos_weights": np.clip(np.exp(-dpos / tau), min_w, 1.0), "neg_weights": np.clip(1.0 - np.exp(-dneg / tau), min_w, 1.0),
            "stats": {"n_anchors": n, "n_pos": n_pos, "n_neg": n_neg, "n_unique": len(unique)}}


ARRAY_KEYS = ("unique_coords", "anchor_to_unique", "pos_pairs", "neg_pairs", "pos_dist", "neg_dist", "pos_raw", "neg_raw", "pos_weights",
              "neg_weights")
SHIFTED_KEYS = ("anchor_to_unique", "pos_pairs", "neg_pairs")


def build_batched(anchors_all, masks, feats, offsets_, draws, **kw):
    """The shifted concatenation of `build` over the segments."""
    parts = [build(anchors_all[a:b], masks[s], feats[s], draws[a:b], **kw) for s, (a, b) in enumerate(zip(offsets_[:-1], offsets_[1:]))]
    out = {"stats": {key: [p["stats"][key] for p in parts] for key in ("n_anchors", "n_pos", "n_neg", "n_unique")}}
    for key, count in (("unique_offsets", "n_unique"), ("pos_offsets", "n_pos"), ("neg_offsets", "n_neg")):
        out[key] = [0] + np.cumsum(out["stats"][count]).tolist()
    for key in ARRAY_KEYS:
        out[key] = np.concatenate([p[key] + (shift if key in SHIFTED_KEYS else 0) for p, shift in zip(parts, out["unique_offsets"][:-1])], axis=0)
    return out


def sorted_rows(anchor_idx, coords):
    """[M, 3] rows (anchor, row, col) in ascending order: what the fixtures and the tests compare."""
    rows = np.concatenate([np.asarray(anchor_idx, dtype=np.int64).reshape(-1, 1), np.asarray(coords, dtype=np.int64).reshape(-1, 2)], axis=1)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
