"""Plain-torch float64 restatement of phase pair mining (losses.build_phase_pairs and its batched form), checked against the
reference-written fixtures (tests/test_cpu_phase_pairs.py) and used where no fixture is committed (tests/test_gpu_phase_pairs.py); and the
seeded input makers the fixtures were drawn with, on top of those of tests/soft_neighborhood_cases.py.

    per anchor i of N >= 2:  its min(k, N - 1) nearest other anchors by squared L2 in spectral space, ascending by (distance, index)
    overlap(i, j) = number of distinct trunc(ysfc) values that both pixels carry anywhere in T
    a neighbour passes iff overlap >= min_overlap;  an anchor survives iff at least min_pairs of its neighbours pass
    result: the passing neighbours of the surviving anchors, by anchor and then by rank, weight exp(-|spec_i - spec_j|_2 / sigma);
            then (i, i) with weight self_pair_weight for the surviving anchors in ascending i (include_self);  empty without a cross pair
"""
import torch

import soft_neighborhood_cases as SC

COUNT_KEYS = ("n_anchors", "n_anchors_surviving", "n_candidates", "n_after_overlap", "n_self_pairs", "n_total_pairs", "overlap_min")
FLOAT_KEYS = ("overlap_mean", "weight_mean", "weight_std", "dist_mean", "dist_std", "dist_q25", "dist_q50", "dist_q75", "dist_min", "dist_max")
WEIGHT_KEYS, DIST_KEYS = FLOAT_KEYS[1:3], FLOAT_KEYS[3:]
EMPTY_KEYS = COUNT_KEYS + FLOAT_KEYS[:3]                                # the ten keys of an empty result

# name -> (N, C, T, seed, scale, reset, parameters, added to ysfc).  g and h reuse the inputs of a.
CASES = {
    "a": (37, 7, 5, 501, 1.0, 0.2, {}, 0),
    "b": (203, 16, 15, 511, 1.0, 0.2, dict(min_overlap=6, min_pairs=8), 0),
    "c": (8, 12, 15, 521, 1.0, 0.2, dict(k=16, min_pairs=2), 0),
    "d": (64, 64, 32, 531, 0.25, 0.2, dict(min_overlap=40), 0),
    "e": (300, 20, 15, 541, 1.0, 0.2, dict(k=8, min_overlap=6, min_pairs=1, include_self=False), 0),
    "f": (130, 12, 39, 561, 1.0, 0.1, dict(min_overlap=12), 0),
    "g": (37, 7, 5, 501, 1.0, 0.2, {}, 60),
    "h": (37, 7, 5, 501, 1.0, 0.2, dict(min_pairs=17), 0),
    "k1": (70, 16, 5, 571, 1.0, 0.2, dict(k=1, min_overlap=2, min_pairs=1), 0),
}
DEFAULTS = dict(k=16, min_overlap=3, min_pairs=5, include_self=True, sigma=5.0, self_pair_weight=1.0)


def make_inputs(n, c, t, seed, scale=1.0, reset=0.2, shift=0):
    """-> (spec [N, C] float32 on the 2^-8 grid, ysfc [N, T] integer-valued float32 ramps with resets, plus `shift`)."""
    return SC.make_points(1, n, c, seed, scale)[0], SC.make_ysfc(n, t, seed + 1, reset) + float(shift)


def case_inputs(name):
    """-> (spec, ysfc, the full parameter dict) of a fixture case."""
    n, c, t, seed, scale, reset, params, shift = CASES[name]
    spec, ysfc = make_inputs(n, c, t, seed, scale, reset, shift)
    return spec, ysfc, {**DEFAULTS, **params}


def make_tied_inputs(n=130, c=3, t=5, seed=581):
    """Points on a half-integer grid in three dimensions: exactly equal distances (and coincident points) are frequent."""
    spec, ysfc = make_inputs(n, c, t, seed)
    return torch.round(spec * 2.0) / 2.0, ysfc


def squared_distances_f64(spec):
    x = spec.detach().to("cpu", torch.float64)
    return ((x.unsqueeze(1) - x.unsqueeze(0)) ** 2).sum(dim=2)


def empty_stats(n, n_candidates=0):
    return {**{key: 0 for key in COUNT_KEYS}, **{key: 0.0 for key in FLOAT_KEYS[:3]}, "n_anchors": n, "n_candidates": n_candidates}


def phase_pairs_f64(spec, ysfc, k=16, min_overlap=3, min_pairs=5, include_self=True, sigma=5.0, self_pair_weight=1.0):
    """-> (pairs int64 [P, 2], weights float64 [P], stats, raw) with raw = {"knn" [N, k] (-1 = none), "overlap", "keep_overlap", "keep"
    [N, k], "anchor_ok" [N], "d2" [N, k]}."""
    n = spec.shape[0]
    none = (torch.zeros((0, 2), dtype=torch.int64), torch.zeros(0, dtype=torch.float64))
    raw = {"knn": torch.full((n, k), -1, dtype=torch.int64), "overlap": torch.zeros((n, k), dtype=torch.int64),
           "keep_overlap": torch.zeros((n, k), dtype=torch.bool), "keep": torch.zeros((n, k), dtype=torch.bool),
           "anchor_ok": torch.zeros(n, dtype=torch.bool), "d2": torch.zeros((n, k), dtype=torch.float64)}
    if n < 2:
        return (*none, empty_stats(n), raw)
    kk = min(k, n - 1)
    d2 = squared_distances_f64(spec)
    d2.fill_diagonal_(float("inf"))
    knn = torch.argsort(d2, dim=1, stable=True)[:, :kk]                  # stable: equal distances keep ascending index
    nd2 = torch.gather(d2, 1, knn)
    values = ysfc.detach().to("cpu").long()                              # truncation
    present = torch.zeros((n, int(values.max()) + 1), dtype=torch.bool)
    present[torch.arange(n).unsqueeze(1), values] = True
    overlap = (present.unsqueeze(1) & present[knn]).sum(dim=2)           # [N, kk]
    passed = overlap >= min_overlap
    anchor_ok = passed.sum(dim=1) >= min_pairs
    keep = passed & anchor_ok.unsqueeze(1)
    raw["knn"][:, :kk], raw["overlap"][:, :kk], raw["keep_overlap"][:, :kk], raw["keep"][:, :kk], raw["d2"][:, :kk] = knn, overlap, passed, keep, nd2
    raw["anchor_ok"] = anchor_ok
    n_cross = int(keep.sum())
    if n_cross == 0:
        raw["anchor_ok"] = torch.zeros(n, dtype=torch.bool)
        return (*none, empty_stats(n, n * kk), raw)
    rows = torch.arange(n).unsqueeze(1).expand(n, kk)
    cross = torch.stack([rows[keep], knn[keep]], dim=1)
    dist = torch.sqrt(nd2[keep])
    w = torch.exp(-dist / sigma)
    ov = overlap[keep]
    survivors = anchor_ok.nonzero().flatten() if include_self else torch.zeros(0, dtype=torch.int64)
    pairs = torch.cat([cross, torch.stack([survivors, survivors], dim=1)], dim=0)
    weights = torch.cat([w, torch.full((survivors.numel(),), float(self_pair_weight), dtype=torch.float64)])
    q = torch.quantile(dist, torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64))
    many = n_cross > 1
    stats = {"n_anchors": n, "n_anchors_surviving": int(anchor_ok.sum()), "n_candidates": n * kk, "n_after_overlap": int(passed.sum()),
             "n_self_pairs": int(survivors.numel()), "n_total_pairs": int(pairs.shape[0]),
             "overlap_mean": float(ov.float().mean()),                   # the reference averages float32 overlaps
             "overlap_min": int(ov.min()), "weight_mean": float(w.mean()), "weight_std": float(w.std()) if many else 0.0,
             "dist_mean": float(dist.mean()), "dist_std": float(dist.std()) if many else 0.0, "dist_q25": float(q[0]), "dist_q50": float(q[1]),
             "dist_q75": float(q[2]), "dist_min": float(dist.min()), "dist_max": float(dist.max())}
    return pairs, weights, stats, raw


def phase_pairs_batched_f64(spec, ysfc, segment_offsets, **kw):
    """A loop over the segments: -> (pairs, weights, stats with the integer counts summed and "per_segment")."""
    off = [int(o) for o in segment_offsets]
    pairs, weights, per_segment = [], [], []
    for lo, hi in zip(off[:-1], off[1:]):
        p, w, st, _ = phase_pairs_f64(spec[lo:hi], ysfc[lo:hi], **kw)
        pairs.append(p + lo)
        weights.append(w)
        per_segment.append(st)
    stats = {key: sum(st[key] for st in per_segment) for key in COUNT_KEYS if key != "overlap_min"}
    stats["per_segment"] = per_segment
    return torch.cat(pairs, dim=0), torch.cat(weights), stats


def weight_bound(d2, sigma, w64):
    """The float32 kernel's weight against float64: the squared distance is exact on grid inputs, sqrtf and the division are correctly
    rounded (the exponent carries at most x 2^-23, x = d / sigma), expf adds about one ulp; the bound is twice that sum."""
    x = torch.sqrt(d2.double()) / sigma
    return (2.0 + x) * 2.0 ** -22 * w64.double()
