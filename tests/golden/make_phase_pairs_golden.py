"""Writes tests/golden/phase_pairs_{a..h,k1}.npz by running the REFERENCE's build_phase_pairs (frl/losses/phase_pairs.py:74-253) in float64,
torch.cdist held on the exact-difference route.  The reference does not travel; only these arrays do.  Inputs come from the seeded makers of
tests/phase_pairs_cases.py (spectral points on the 2^-8 grid, ysfc ramps with resets).

phase_pairs_*: spec [N, C] float32, ysfc [N, T] float32, k, min_overlap, min_pairs, include_self, sigma, self_pair_weight, pairs [P, 2]
int32, weights64 [P], and one stat_* value per key of the reference's stats dict (ten keys for an empty result, seventeen otherwise).

Before a case is written the maker asserts the property the case is there for (so a reseed cannot quietly empty it), that every squared
distance is below 256 (float32 sums of 2^-16-grid squares are then exact and the float32 ranking is the float64 one), and that no two of
an anchor's k + 1 smallest distances are equal (the reference's tie order, which torch.topk leaves unspecified, cannot show).

    python tests/golden/make_phase_pairs_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl"))
sys.path.insert(0, os.path.dirname(HERE))
from losses.phase_pairs import build_phase_pairs  # noqa: E402

import phase_pairs_cases as PP  # noqa: E402

_cdist = torch.cdist
torch.cdist = lambda a, b, *args, **kw: _cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist")   # exact differences at any size


def run(name):
    spec, ysfc, kw = PP.case_inputs(name)
    pairs, weights, stats = build_phase_pairs(spec.double(), ysfc.double(), **kw)
    return spec, ysfc, kw, pairs, weights, stats


def write(name, results):
    spec, ysfc, kw, pairs, weights, stats = results[name]
    n, c = spec.shape
    k = kw["k"]
    d2 = PP.squared_distances_f64(spec)
    assert float(d2.max()) < 256.0, "a squared distance of 256 or more: the float32 sum is no longer exact"
    d2.fill_diagonal_(float("inf"))
    head = torch.sort(d2, dim=1).values[:, :min(k + 1, n - 1)]
    assert bool((head[:, 1:] > head[:, :-1]).all()), "two of an anchor's k + 1 smallest distances are equal"
    n_cross = stats["n_total_pairs"] - stats["n_self_pairs"]
    _, _, _, raw = PP.phase_pairs_f64(spec, ysfc, **kw)
    passed = int(raw["keep_overlap"].sum())
    if name == "a":
        assert c % 16 != 0 and 0 < stats["n_anchors_surviving"] < n and 0 < stats["n_after_overlap"] < stats["n_candidates"]
    if name == "b":
        assert n > 128 and n % 4 != 0 and 0 < stats["n_anchors_surviving"] < n and n_cross < stats["n_after_overlap"] < stats["n_candidates"]
    if name == "c":
        assert k > n - 1 and stats["n_candidates"] == n * (n - 1) and n_cross > 0
    if name == "d":
        assert pairs.shape == (0, 2) and stats["n_candidates"] == n * k and passed == 0 and len(stats) == 10
    if name == "e":
        assert not kw["include_self"] and stats["n_self_pairs"] == 0 and n_cross > 0 and bool((pairs[:, 0] != pairs[:, 1]).all()) and n > 256
    if name == "f":
        assert float(ysfc.max()) > 40 and 0 < stats["n_anchors_surviving"] < n
    if name == "g":
        assert float(ysfc.min()) < 64 <= float(ysfc.max()) and torch.equal(pairs, results["a"][3]) and pairs.shape[0] > 0
    if name == "h":
        assert pairs.shape == (0, 2) and passed > 0 and stats["n_after_overlap"] == 0 and stats["n_candidates"] == n * k
    if name == "k1":
        assert k == 1 and 0 < stats["n_self_pairs"] == n_cross < n
    arrays = dict(spec=spec.numpy(), ysfc=ysfc.numpy(), k=np.int64(k), min_overlap=np.int64(kw["min_overlap"]), min_pairs=np.int64(kw["min_pairs"]),
                  include_self=np.bool_(kw["include_self"]), sigma=np.float64(kw["sigma"]), self_pair_weight=np.float64(kw["self_pair_weight"]),
                  pairs=pairs.numpy().astype(np.int32), weights64=weights.double().numpy())
    for key, value in stats.items():
        arrays["stat_" + key] = np.float64(value)
    path = os.path.join(HERE, f"phase_pairs_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"phase_pairs_{name}", tuple(spec.shape), tuple(ysfc.shape), "candidates", stats["n_candidates"], "pass the overlap", passed,
          "anchors surviving", stats["n_anchors_surviving"], "pairs", int(pairs.shape[0]), "self", stats["n_self_pairs"], "ysfc max",
          float(ysfc.max()), os.path.getsize(path), "bytes")


def main():
    results = {name: run(name) for name in PP.CASES}
    for name in PP.CASES:
        write(name, results)


if __name__ == "__main__":
    main()
