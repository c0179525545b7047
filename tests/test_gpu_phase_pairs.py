"""GPU parity of phase pair mining (csrc/phase_pairs.hip behind losses.build_phase_pairs / build_phase_pairs_batched) against the fixtures
written by the REFERENCE's build_phase_pairs (tests/golden/make_phase_pairs_golden.py) and, where no fixture is committed, against the
float64 restatement (tests/phase_pairs_cases.py, pinned to the fixtures by tests/test_cpu_phase_pairs.py).

Bounds.  pair_indices and the integer statistics are equal, order included.  A weight is within (2 + x) 2^-22 w64 of the float64 value,
x = d / sigma: the squared distance is exact on these inputs (2^-8 grid, below 256), sqrtf and the division are correctly rounded, so the
exponent carries at most x 2^-23, expf adds about one ulp, and the bound is twice that sum.  A distance is a correctly rounded sqrtf of
an exact value: within 2^-24 d.  The float statistics are float64 reductions of those entries (means, unbiased standard deviations,
interpolated quantiles, extremes): within twice the largest entry bound of their kind, absolutely.  overlap_mean is the reference's
float32 quotient of an exact integer sum: equal."""
import os

import numpy as np
import pytest
import torch

import phase_pairs_cases as PP
import soft_neighborhood_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(PP.CASES)
B_PARAMS = dict(min_overlap=6, min_pairs=8)


def _fx(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, f"phase_pairs_{name}.npz"))
    kw = dict(k=int(fx["k"]), min_overlap=int(fx["min_overlap"]), min_pairs=int(fx["min_pairs"]), include_self=bool(fx["include_self"]),
              sigma=float(fx["sigma"]), self_pair_weight=float(fx["self_pair_weight"]))
    return fx, kw


def _pair_d2(spec, pairs):
    x = spec.detach().to("cpu", torch.float64)
    p = pairs.to("cpu", torch.int64)
    return ((x[p[:, 0]] - x[p[:, 1]]) ** 2).sum(dim=1)


def _check_weights(weights, w64, spec, pairs, sigma, what):
    """-> (largest weight bound, largest distance bound) over the cross pairs."""
    assert weights.dtype == torch.float32 and weights.shape == w64.shape
    d2 = _pair_d2(spec, pairs)
    bound = PP.weight_bound(d2, sigma, w64)
    dev = (weights.double().cpu() - w64).abs()
    cross = pairs[:, 0].cpu() != pairs[:, 1].cpu()
    print(f"{what}: {int(cross.sum())} cross weights, worst dev / bound {float((dev / bound).max()) if len(dev) else 0.0:.3f}")
    assert bool((dev <= bound).all()), what
    if not bool(cross.any()):
        return 0.0, 0.0
    return float(bound[cross].max()), float(2.0 ** -24 * torch.sqrt(d2[cross]).max())


@pytest.mark.parametrize("name", CASES)
def test_fixture(golden_dir, name):
    from frl_hip.losses import build_phase_pairs
    fx, kw = _fx(golden_dir, name)
    spec, ysfc = torch.from_numpy(fx["spec"]), torch.from_numpy(fx["ysfc"])
    pairs, weights, stats = build_phase_pairs(spec.to(DEV), ysfc.to(DEV), **kw)
    assert pairs.dtype == torch.int64 and pairs.is_cuda and pairs.dim() == 2 and pairs.shape[1] == 2
    assert np.array_equal(pairs.cpu().numpy(), fx["pairs"].astype(np.int64)), "pair_indices differ from the reference's"
    wb, db = _check_weights(weights, torch.from_numpy(fx["weights64"]), spec, pairs, kw["sigma"], name)
    want = {key[5:]: float(fx[key]) for key in fx.files if key.startswith("stat_")}
    assert set(stats) == set(want)
    for key in stats:
        if key in PP.COUNT_KEYS:
            assert stats[key] == int(want[key]) and isinstance(stats[key], int), key
        elif key == "overlap_mean":
            assert stats[key] == want[key], key
        else:
            bound = 2.0 * (wb if key in PP.WEIGHT_KEYS else db)
            print(f"{name} {key}: got {stats[key]!r} want {want[key]!r} dev {abs(stats[key] - want[key]):.3e} bound {bound:.3e}")
            assert abs(stats[key] - want[key]) <= bound, key
    p2, w2, none = build_phase_pairs(spec.to(DEV), ysfc.to(DEV), **kw, stats=False)
    assert none == {} and torch.equal(p2, pairs) and torch.equal(w2, weights)


@pytest.fixture(scope="module")
def batch():
    """Segments [37, 1, 203, 0, 64]: the inputs of case a, one lone anchor, the inputs of case b, an empty segment, the inputs of case d."""
    a, b, d = PP.case_inputs("a"), PP.case_inputs("b"), PP.case_inputs("d")
    lone = PP.make_inputs(1, 16, 15, 591)
    width, t = 64, 32

    def rows(spec, ysfc):                                               # one width and one T for the pooled rows: zero columns add
        s = torch.nn.functional.pad(spec, (0, width - spec.shape[1]))   # nothing to a distance, a repeated last year no new ysfc value
        y = torch.cat([ysfc, ysfc[:, -1:].expand(-1, t - ysfc.shape[1])], dim=1)
        return s, y

    parts = [rows(*a[:2]), rows(*lone), rows(*b[:2]), rows(*d[:2])]
    spec, ysfc = torch.cat([p[0] for p in parts]).contiguous(), torch.cat([p[1] for p in parts]).contiguous()
    return spec, ysfc, [0, 37, 38, 241, 241, 305]


@pytest.mark.parametrize("params", [{}, B_PARAMS, dict(k=5, min_overlap=2, min_pairs=0, include_self=True)], ids=["defaults", "b", "min_pairs0"])
def test_batched_equals_single_calls_and_restatement(batch, params):
    from frl_hip.losses import build_phase_pairs, build_phase_pairs_batched
    spec, ysfc, off = batch
    sd, yd = spec.to(DEV), ysfc.to(DEV)
    pairs, weights, stats = build_phase_pairs_batched(sd, yd, off, **params)
    singles = [build_phase_pairs(sd[lo:hi].contiguous(), yd[lo:hi].contiguous(), **params) for lo, hi in zip(off[:-1], off[1:])]
    assert torch.equal(pairs, torch.cat([p + lo for (p, _, _), lo in zip(singles, off[:-1])])), "not the shifted concatenation"
    assert torch.equal(weights, torch.cat([w for _, w, _ in singles]))
    for got, (_, _, want) in zip(stats["per_segment"], singles):         # the same entries reduced from another address: counts equal,
        assert set(got) == set(want)                                    # float64 reductions to their last few bits
        for key in got:
            assert got[key] == want[key] if key in PP.COUNT_KEYS else abs(got[key] - want[key]) <= 1e-12 * max(1.0, abs(want[key])), key
    p_list, w_tensor, none = build_phase_pairs_batched(sd, yd, torch.tensor(off), **params, stats=False)
    assert none == {} and torch.equal(p_list, pairs) and torch.equal(w_tensor, weights)
    p64, w64, st64 = PP.phase_pairs_batched_f64(spec, ysfc, off, **params)
    assert torch.equal(pairs.cpu(), p64), "pair_indices differ from the restatement's"
    kw = {**PP.DEFAULTS, **params}
    _check_weights(weights, w64, spec, pairs, kw["sigma"], "batched")
    for key in PP.COUNT_KEYS:
        if key != "overlap_min":
            assert stats[key] == st64[key], key
        assert [s[key] for s in stats["per_segment"]] == [s[key] for s in st64["per_segment"]], key
    assert set(stats) == set(st64) and "weight_mean" not in stats
    assert pairs.shape[0] > 0 and stats["per_segment"][1] == PP.empty_stats(1) and stats["per_segment"][3] == PP.empty_stats(0)


def test_raw_outputs(batch):
    from frl_hip import ops
    spec, ysfc, off = batch
    spec = torch.cat([spec, spec[:8]])                                  # a sixth segment of 8 anchors: fewer neighbours than k
    ysfc = torch.cat([ysfc, ysfc[:8]])
    off = off + [313]
    k, min_overlap, min_pairs, sigma = 16, 3, 5, 5.0
    seg_host = torch.tensor(off, dtype=torch.int32)
    out = ops.phase_pairs(spec.to(DEV), ysfc.to(DEV), seg_host.to(DEV), seg_host, k, min_overlap, min_pairs, sigma)
    out = {key: value.cpu() for key, value in out.items()}
    assert out["knn_idx"].dtype == torch.int32 and out["keep"].dtype == torch.uint8 and out["meta"][-1] == 0
    counters = out["meta"][:-1].reshape(-1, 4)
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        n = hi - lo
        if n == 0:
            assert not counters[s].any()
            continue
        _, _, _, raw = PP.phase_pairs_f64(spec[lo:hi], ysfc[lo:hi], k=k, min_overlap=min_overlap, min_pairs=min_pairs, sigma=sigma)
        kk = min(k, n - 1)
        knn = out["knn_idx"][lo:hi].long()
        assert bool((knn[:, kk:] == -1).all()) and not out["keep"][lo:hi, kk:].any() and not out["keep_overlap"][lo:hi, kk:].any()
        assert not out["weight"][lo:hi, kk:].any() and not out["dist"][lo:hi, kk:].any() and not out["overlap"][lo:hi, kk:].any()
        assert torch.equal(knn[:, :kk], raw["knn"][:, :kk] + lo) and bool(((knn[:, :kk] >= lo) & (knn[:, :kk] < hi)).all())
        assert torch.equal(out["overlap"][lo:hi].long(), raw["overlap"])
        passed = raw["overlap"][:, :kk] >= min_overlap
        assert torch.equal(out["keep_overlap"][lo:hi, :kk].bool(), passed)
        ok = passed.sum(dim=1) >= min_pairs
        assert torch.equal(out["anchor_ok"][lo:hi].bool(), ok) and torch.equal(out["keep"][lo:hi, :kk].bool(), passed & ok.unsqueeze(1))
        d64 = raw["d2"][:, :kk].sqrt()
        assert bool(((out["dist"][lo:hi, :kk].double() - d64).abs() <= 2.0 ** -24 * d64).all())
        assert counters[s].tolist() == [n * kk, int(passed.sum()), int((passed & ok.unsqueeze(1)).sum()), int(ok.sum())]


def test_tied_distances_follow_distance_then_index():
    from frl_hip.losses import build_phase_pairs
    spec, ysfc = PP.make_tied_inputs()
    kw = dict(k=16, min_overlap=2, min_pairs=3)
    pairs, weights, stats = build_phase_pairs(spec.to(DEV), ysfc.to(DEV), **kw)
    p64, w64, st64, _ = PP.phase_pairs_f64(spec, ysfc, **kw)
    assert pairs.shape[0] > 500 and torch.equal(pairs.cpu(), p64)
    _check_weights(weights, w64, spec, pairs, 5.0, "tied")               # distances on the half-integer grid are exact as well
    assert all(stats[key] == st64[key] for key in PP.COUNT_KEYS)


def test_long_segment_uses_more_than_64k_of_lds():
    """4100 anchors on a line at spacing 2^-4 (the distance rows of four anchors pass 64 KB of LDS), all with the same ysfc: every
    distance is tied between the two sides of an anchor, so by (distance, index) its neighbours are i - 1, i + 1, i - 2, i + 2, ... as
    far as they exist; everything passes the overlap filter."""
    from frl_hip.losses import build_phase_pairs_batched
    n, k, sigma = 4100, 4, 5.0
    spec = torch.zeros(n, 3)
    spec[:, 1] = torch.arange(n) / 16.0
    ysfc = torch.arange(5.0).repeat(n, 1)
    step = torch.tensor([-1, 1, -2, 2, -3, 3, -4, 4])
    cand = torch.arange(n).unsqueeze(1) + step
    valid = (cand >= 0) & (cand < n)
    first = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)[:, :k]      # the existing ones, in order
    knn = torch.gather(cand, 1, first)
    rows = torch.arange(n).unsqueeze(1).expand(n, k)
    want = torch.cat([torch.stack([rows.reshape(-1), knn.reshape(-1)], dim=1), torch.arange(n).unsqueeze(1).expand(n, 2)])
    w64 = torch.exp(-torch.sqrt(_pair_d2(spec, want)) / sigma)
    pairs, weights, stats = build_phase_pairs_batched(torch.cat([spec[:5], spec]).to(DEV), torch.cat([ysfc[:5], ysfc]).to(DEV), [0, 5, n + 5],
                                                      k=k, min_overlap=5, min_pairs=k, sigma=sigma)
    assert stats["per_segment"][1]["n_total_pairs"] == n * (k + 1) and stats["per_segment"][0]["n_total_pairs"] == 25
    assert torch.equal(pairs[25:].cpu(), want + 5)
    _check_weights(weights[25:], w64, spec, want, sigma, "long segment")


def test_limits_and_argument_errors():
    from frl_hip import _lib
    from frl_hip.losses import build_phase_pairs, build_phase_pairs_batched
    nmax = _lib.load().frl_phase_pairs_max_points(16)
    assert nmax == (160 * 1024 - (4 * 16 + 64 * 20) * 4) // 16
    big_spec, big_ysfc = torch.zeros(nmax + 1, 16, device=DEV), torch.zeros(nmax + 1, 3, device=DEV)
    with pytest.raises(_lib.FrlHipError, match="do not fit the LDS"):
        build_phase_pairs(big_spec, big_ysfc)
    with pytest.raises(_lib.FrlHipError, match="do not fit the LDS"):
        build_phase_pairs_batched(big_spec, big_ysfc, [0, 0, nmax + 1])
    spec, ysfc, _ = PP.case_inputs("a")
    sd, yd = spec.to(DEV), ysfc.to(DEV)
    with pytest.raises(ValueError, match="k must be in 1..64"):
        build_phase_pairs(sd, yd, k=65)
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):
        build_phase_pairs(spec, yd)
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):
        build_phase_pairs(sd, ysfc)
    for bad in (float("nan"), float("inf"), -1.0, 256.0):
        y = yd.clone()
        y[20, 3] = bad
        with pytest.raises(ValueError, match="ysfc must hold finite values in 0..255"):
            build_phase_pairs(sd, y)
    y = yd.clone()
    y[20, 3] = 255.75                                                   # truncated to 255: the largest value the masks hold
    pairs, _, _ = build_phase_pairs(sd, y)
    p64, _, _, _ = PP.phase_pairs_f64(spec, y.cpu())
    assert torch.equal(pairs.cpu(), p64)


def test_k64_and_wide_features():
    from frl_hip.losses import build_phase_pairs
    spec, ysfc = PP.make_inputs(150, 100, 15, 601, scale=0.5)           # C = 100 is padded to 128, the next width with a kernel
    kw = dict(k=64, min_overlap=4, min_pairs=20)
    pairs, weights, stats = build_phase_pairs(spec.to(DEV), ysfc.to(DEV), **kw)
    p64, w64, st64, _ = PP.phase_pairs_f64(spec, ysfc, **kw)
    assert float(PP.squared_distances_f64(spec).max()) < 256.0
    assert pairs.shape[0] > 0 and torch.equal(pairs.cpu(), p64)
    _check_weights(weights, w64, spec, pairs, 5.0, "k = 64")
    assert all(stats[key] == st64[key] for key in PP.COUNT_KEYS)


def test_pairs_feed_phase_neighborhood_loss(batch):
    """The hand-over of dtype, device and layout: the batched call's pairs and weights against the restatement's, through the loss."""
    from frl_hip.losses import build_phase_pairs_batched, phase_neighborhood_loss
    spec, ysfc, off = batch
    n, t = ysfc.shape
    pairs, weights, _ = build_phase_pairs_batched(spec.to(DEV), ysfc.to(DEV), off, stats=False)
    p64, w64, _ = PP.phase_pairs_batched_f64(spec, ysfc, off)
    spectral, phase = SC.make_points(n, t, 6, 611).to(DEV), SC.make_points(n, t, 12, 612, 0.25).to(DEV)
    got, st_got = phase_neighborhood_loss(spectral, phase, ysfc.to(DEV), pairs, pair_weights=weights, tau_ref=1.0, tau_learned=1.0)
    want, st_want = phase_neighborhood_loss(spectral, phase, ysfc.to(DEV), p64.to(DEV), pair_weights=w64.float().to(DEV), tau_ref=1.0, tau_learned=1.0)
    # the loss is a weighted mean of non-negative per-pair terms: a relative change eps of every weight moves it by at most 2 eps
    # relatively; eps is the largest relative weight bound, and 2^-20 covers the float32 sums rounding differently under other weights
    cross = p64[:, 0] != p64[:, 1]
    eps = float((PP.weight_bound(_pair_d2(spec, p64), 5.0, w64) / w64)[cross].max()) + 2.0 ** -24
    bound = (2.0 * eps + 2.0 ** -20) * abs(float(want))
    print(f"loss {float(got)!r} against {float(want)!r}: dev {abs(float(got) - float(want)):.3e} bound {bound:.3e}")
    assert float(want) > 0 and st_got["n_pairs_sufficient_overlap"] == st_want["n_pairs_sufficient_overlap"] > 0
    assert abs(float(got) - float(want)) <= bound
