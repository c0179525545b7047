"""Writes tests/golden/spatial_knn.npz and tests/golden/spatial_neg.npz by running the REFERENCE's spatial_knn_pairs and
spatial_negative_pairs (frl/utils/spatial.py:176-332).  The reference does not travel; only these arrays do.  Inputs come from the seeded
makers of tests/spatial_pairs_cases.py (a 24 x 20 mask with a hole, 40 anchors with corners, edges and a duplicate).

spatial_knn: mask, anchors, and per k in {4, 8, 12} (max_radius 8) rows_k [M, 3] = (anchor, row, col) sorted ascending.  These k end on
a distance boundary (4, 8 and 12 offsets lie within distances 1, sqrt 2 and 2), so the reference's unstable argsort cannot change the
set; the maker asserts that.
spatial_neg: torch.randperm cannot be matched, so the candidate sets are pinned: the reference is called with n_per_anchor at the number
of valid pixels and then returns every candidate of every anchor.  Per case i: min_i, max_i (NaN for None), keys_i (row * W + col,
ascending per anchor, concatenated) and offs_i [N + 1].  The maker asserts what each case is there for: an anchor without a candidate,
an anchor with fewer than four, a non-integer threshold, max_distance == min_distance.

    python tests/golden/make_spatial_pairs_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
_spec = importlib.util.spec_from_file_location(
    "reference_spatial", os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl", "utils", "spatial.py"))
REF = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(REF)

import spatial_pairs_cases as SP  # noqa: E402


def main():
    mask, anchors = SP.fixture_inputs()
    h, w = mask.shape
    n = anchors.shape[0]
    mask_t, anchors_t = torch.from_numpy(mask), torch.from_numpy(anchors)
    assert len({tuple(a) for a in anchors.tolist()}) < n, "no duplicate anchor"

    knn = dict(mask=mask, anchors=anchors, max_radius=np.int64(SP.FIXTURE_RADIUS))
    for k in SP.FIXTURE_K:
        d2 = sorted(dr * dr + dc * dc for dr in range(-8, 9) for dc in range(-8, 9) if 0 < dr * dr + dc * dc <= 64)
        assert d2[k - 1] < d2[k], f"k = {k} does not end on a distance boundary"
        idx, rc = REF.spatial_knn_pairs(anchors_t, mask_t, k=k, max_radius=SP.FIXTURE_RADIUS)
        rows = SP.sorted_rows(idx.numpy(), rc.numpy())
        assert 0 < len(rows) < n * k, "every slot valid or none: the case checks nothing"
        knn[f"rows_{k}"] = rows.astype(np.int32)
        print(f"spatial_knn k={k}: {len(rows)} of {n * k} slots valid")
    path = os.path.join(HERE, "spatial_knn.npz")
    np.savez_compressed(path, **knn)
    print("spatial_knn", os.path.getsize(path), "bytes")

    neg = dict(mask=mask, anchors=anchors)
    n_valid = int(mask.sum())
    seen = set()
    for i, (dmin, dmax) in enumerate(SP.FIXTURE_NEG):
        torch.manual_seed(i)
        idx, rc = REF.spatial_negative_pairs(anchors_t, mask_t, min_distance=dmin, max_distance=dmax, n_per_anchor=n_valid)
        idx, keys = idx.numpy(), (rc[:, 0] * w + rc[:, 1]).numpy()
        per_anchor = [np.sort(keys[idx == a]) for a in range(n)]
        counts = np.asarray([len(p) for p in per_anchor])
        if (counts == 0).any():
            seen.add("an anchor without a candidate")
        if ((counts > 0) & (counts < 4)).any():
            seen.add("an anchor with fewer than four")
        if dmin != int(dmin) or (dmax is not None and dmax != int(dmax)):
            seen.add("a non-integer threshold")
        if dmax is not None and dmax == dmin:
            seen.add("max == min")
            assert counts.sum() > 0
        if (dmin, dmax) == (40.0, None):
            assert counts.sum() == 0, "min_distance beyond the diagonal still has candidates"
        neg[f"min_{i}"] = np.float64(dmin)
        neg[f"max_{i}"] = np.float64(np.nan if dmax is None else dmax)
        neg[f"keys_{i}"] = np.concatenate(per_anchor).astype(np.int32)
        neg[f"offs_{i}"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        print(f"spatial_neg case {i} ({dmin}, {dmax}): {int(counts.sum())} candidates, {int((counts == 0).sum())} anchors empty, "
              f"{int(((counts > 0) & (counts < 4)).sum())} with 1..3")
    assert seen == {"an anchor without a candidate", "an anchor with fewer than four", "a non-integer threshold", "max == min"}, seen
    path = os.path.join(HERE, "spatial_neg.npz")
    np.savez_compressed(path, **neg)
    print("spatial_neg", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
