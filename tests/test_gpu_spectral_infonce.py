"""GPU checks of the global spectral InfoNCE block (csrc/spectral_negatives.hip, frl_hip.losses.spectral_infonce) against the restatement
of tests/spectral_infonce_cases.py and the fixtures the reference wrote (tests/golden/make_spectral_infonce_golden.py).

Tolerances.  Distances: every term of the float32 sum of squares passes through at most C / 16 + 8 roundings at C <= 256 and the square
root halves the relative error: 2e-6 relative against float64, the bound of tests/test_gpu_contrastive.py.  Weights: the distance error
passes through x e^-x <= 0.37, plus a couple of ulp of expf on values <= 1: 2e-6 absolute.  Similarities: 2e-6 relative, as the
distances without the root.  Their mean and standard deviation are sums kept in double, so they carry the per-pair bound only; the
deviation moves by at most the largest per-pair error: 5e-6 * max(1, |v|) (2.5 x margin).  Loss and gradient: the tolerances of
test_contrastive_loss_matches_reference."""
import os

import numpy as np
import pytest
import torch

import spectral_infonce_cases as SC
from frl_hip.losses import spectral_infonce  # noqa: F401  (the module under test: nothing here can run without it)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_NAMES = ["a", "b", "c", "d"]


def _fx(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"spectral_infonce_{case}.npz"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_case(case, **kw):
    from frl_hip.losses import cross_patch_negatives
    c, inp = SC.CASES[case], SC.make_inputs(case)
    out = cross_patch_negatives(_dev(inp["spec"]), inp["offsets"], c["neg_per_anchor"], SC.TAU, SC.MIN_W, draws=_dev(inp["draws"]), **kw)
    return inp, out


def _check_dist_and_weights(out, dist64, w64):
    d, w = out["neg_dist"].cpu().numpy().astype(np.float64), out["neg_weights"].cpu().numpy().astype(np.float64)
    assert out["neg_dist"].dtype == torch.float32 and out["neg_weights"].dtype == torch.float32
    err_d, err_w = np.abs(d - dist64) / np.maximum(dist64, 1e-30), np.abs(w - w64)
    print(f"neg_dist relative error {err_d.max():.2e}, neg_weights absolute error {err_w.max():.2e}")
    assert err_d.max() <= 2e-6
    assert err_w.max() <= 2e-6


# ---- negatives: indices ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASE_NAMES)
def test_negatives_match_fixture(golden_dir, case):
    """Cases a-d (C = 7, 33, 1, 16: scalar rows with lane tails, one channel, 16-byte rows): pairs integer-exact, distances and weights
    against the reference's float64."""
    fx = _fx(golden_dir, case)
    inp, out = _run_case(case)
    assert out["n_per"] == inp["n_per"] and out["neg_pairs"].dtype == torch.int64
    pairs = out["neg_pairs"].cpu().numpy()
    assert np.array_equal(pairs, SC.negative_pairs(inp["offsets"], inp["n_per"], inp["draws"]))
    assert np.array_equal(pairs, fx["neg"])
    _check_dist_and_weights(out, fx["neg_dist"], fx["neg_w"])
    if case == "c":                                                       # the lower clamp: exactly min_w where the reference clamps
        below = 1.0 - np.exp(-fx["neg_dist"] / SC.TAU) < SC.MIN_W - 1e-6
        assert below.sum() > 0 and (fx["neg_w"][below] == SC.MIN_W).all()
        assert (out["neg_weights"].cpu().numpy()[below] == np.float32(SC.MIN_W)).all()


def test_negatives_extreme_draws_hit_first_and_last_anchor():
    from frl_hip.losses import cross_patch_negatives
    c, inp = SC.CASES["a"], SC.make_inputs("a")
    draws = np.where(np.random.default_rng(7).random(inp["draws"].shape) < 0.5, 0, SC.DRAW_TOP).astype(np.int64)
    for dtype in (np.int64, np.int32):
        out = cross_patch_negatives(_dev(inp["spec"]), torch.tensor(inp["offsets"]), c["neg_per_anchor"], draws=_dev(draws.astype(dtype)))
        pairs = out["neg_pairs"].cpu().numpy()
        assert np.array_equal(pairs, SC.negative_pairs(inp["offsets"], inp["n_per"], draws))
        offs = np.asarray(inp["offsets"])
        assert np.isin(pairs, np.concatenate([offs[:-1], offs[1:] - 1])).all()


# ---- negatives: distances and weights -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("aligned", [True, False])
def test_negatives_256_channels_upper_clamp(aligned):
    """C = 256 (four 16-byte loads per lane) with unit-variance rows: d ~ 22, 1 - exp(-d) rounds to 1.0 exactly.  The same rows at an
    address that is no multiple of 16 bytes take the scalar route."""
    from frl_hip.losses import cross_patch_negatives
    patches = (5, 9, 4)
    offsets = SC.offsets_of(patches)
    spec = SC.make_rows(offsets[-1], 256, 77)
    n_per = SC.n_per_of(20, offsets[-1], 3)
    draws = SC.make_draws(n_per * 6, 78)
    t = _dev(spec)
    if not aligned:
        buf = torch.empty(spec.size + 1, dtype=torch.float32, device=DEV)
        t = buf[1:].view(spec.shape).copy_(t)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    out = cross_patch_negatives(t, offsets, 20, SC.TAU, SC.MIN_W, draws=_dev(draws))
    pairs, dist64, w64 = SC.negatives(spec, offsets, n_per, draws)
    assert np.array_equal(out["neg_pairs"].cpu().numpy(), pairs)
    _check_dist_and_weights(out, dist64, w64)
    assert dist64.min() > 18.0 and (out["neg_weights"] == 1.0).all()


# ---- negatives: scale, with the similarity statistics of as many pairs ------------------------------------------------------------------

def test_negatives_and_similarities_beyond_one_grid_pass():
    """4 x 750 anchors, 20 per anchor: Q = 60000 pairs, more than the 2048 x 16 of one pass of the grid; no kNN."""
    from frl_hip.losses import cross_patch_negatives, pair_similarity, pair_similarity_stats
    offsets = SC.offsets_of((750,) * 4)
    n = offsets[-1]
    spec, z = SC.make_rows(n, 16, 91), SC.make_rows(n, 64, 92)
    n_per = SC.n_per_of(20, n, 4)
    draws = SC.make_draws(n_per * 12, 93)
    assert draws.shape[0] == 60000
    out = cross_patch_negatives(_dev(spec), offsets, 20, SC.TAU, SC.MIN_W, draws=_dev(draws))
    pairs, dist64, w64 = SC.negatives(spec, offsets, n_per, draws)
    assert np.array_equal(out["neg_pairs"].cpu().numpy(), pairs)
    _check_dist_and_weights(out, dist64, w64)
    zt = _dev(z)
    sims64 = SC.sims(z, pairs)
    got = pair_similarity(zt, out["neg_pairs"]).cpu().numpy().astype(np.float64)
    assert (np.abs(got - sims64) <= 2e-6 * np.abs(sims64)).all()
    few = pairs[:5000:7]
    st = pair_similarity_stats(zt, _dev(few), out["neg_pairs"], 0.07)
    want = SC.sim_stats(z, few) + SC.sim_stats(z, pairs)
    for key, v in zip(("pos_mean", "pos_std", "neg_mean", "neg_std"), want):
        assert abs(st[key] - v) <= 5e-6 * max(1.0, abs(v)), (key, st[key], v)


# ---- negatives: misuse and reproducibility --------------------------------------------------------------------------------------------

def test_out_of_range_device_draws_are_clamped_and_flagged():
    from frl_hip import ops
    from frl_hip.losses import cross_patch_negatives
    c, inp = SC.CASES["a"], SC.make_inputs("a")
    offs = np.asarray(inp["offsets"])
    spec = _dev(inp["spec"])
    ops.index_errors()
    out = cross_patch_negatives(spec, inp["offsets"], c["neg_per_anchor"], draws=_dev(inp["draws"]))
    assert not ops.index_errors()
    for dtype, bad in ((np.int64, (-5, 2 ** 31, 2 ** 40, -2 ** 40)), (np.int32, (-1, -2 ** 31))):
        draws = inp["draws"].astype(dtype)
        rows = [3, 700, 1001, 1337][:len(bad)]
        for r, v in zip(rows, bad):
            draws[r, r % 2] = v
        got = cross_patch_negatives(spec, inp["offsets"], c["neg_per_anchor"], draws=_dev(draws))
        pairs = got["neg_pairs"].cpu().numpy()
        blocks = np.repeat(np.asarray(SC.blocks(3)), inp["n_per"], axis=0)
        assert (pairs >= offs[blocks]).all() and (pairs < offs[blocks + 1]).all()                       # inside their patches
        assert torch.isfinite(got["neg_dist"]).all() and torch.isfinite(got["neg_weights"]).all()
        keep = np.ones(len(pairs), dtype=bool)
        keep[rows] = False
        assert np.array_equal(pairs[keep], out["neg_pairs"].cpu().numpy()[keep])                        # the other negatives are untouched
        assert ops.index_errors() and not ops.index_errors()                                            # set, then cleared


def test_negatives_are_reproducible():
    from frl_hip.losses import cross_patch_negatives
    _, a = _run_case("d")
    _, b = _run_case("d")
    for key in ("neg_pairs", "neg_dist", "neg_weights"):
        assert torch.equal(a[key], b[key])
    inp = SC.make_inputs("a")
    spec = _dev(inp["spec"])
    outs = []
    for seed in (5, 5, 6):
        g = torch.Generator(device=DEV).manual_seed(seed)
        outs.append(cross_patch_negatives(spec, inp["offsets"], 20, generator=g))
    assert torch.equal(outs[0]["neg_pairs"], outs[1]["neg_pairs"]) and torch.equal(outs[0]["neg_weights"], outs[1]["neg_weights"])
    assert not torch.equal(outs[0]["neg_pairs"], outs[2]["neg_pairs"])
    pairs = outs[0]["neg_pairs"].cpu().numpy()                                                          # drawn pairs obey the block structure
    offs, blocks = np.asarray(inp["offsets"]), np.repeat(np.asarray(SC.blocks(3)), inp["n_per"], axis=0)
    assert (pairs >= offs[blocks]).all() and (pairs < offs[blocks + 1]).all()
    one = cross_patch_negatives(spec, [0, spec.shape[0]], 20)                                           # one patch: no negatives
    assert one["neg_pairs"].shape == (0, 2) and one["n_per"] == 0 and one["neg_weights"].shape == (0,)


# ---- similarities ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASE_NAMES)
def test_similarities_and_statistics_match_fixture(golden_dir, case):
    from frl_hip.losses import pair_similarity, pair_similarity_stats
    fx, inp = _fx(golden_dir, case), SC.make_inputs(case)
    z = _dev(inp["z"])
    pos, neg = _dev(fx["pos"].astype(np.int64)), _dev(fx["neg"].astype(np.int64))
    for pairs in (pos, neg):
        want = SC.sims(inp["z"], pairs.cpu().numpy())
        got = pair_similarity(z, pairs)
        assert got.dtype == torch.float32 and got.shape == (pairs.shape[0],)
        assert (np.abs(got.cpu().numpy() - want) <= 2e-6 * np.abs(want)).all()
        assert torch.equal(got, pair_similarity(z, pairs))
    st = pair_similarity_stats(z, pos, neg, SC.TEMPERATURE)
    assert st["temperature"] == SC.TEMPERATURE and set(st) == {"pos_mean", "pos_std", "neg_mean", "neg_std", "temperature"}
    for key, v in zip(("pos_mean", "pos_std", "neg_mean", "neg_std"), fx["stats"]):
        print(f"{case} {key}: {st[key]!r} against {v!r}")
        assert abs(st[key] - v) <= 5e-6 * max(1.0, abs(v)), key
    assert st == pair_similarity_stats(z, pos, neg, SC.TEMPERATURE)                                     # identical bits


@pytest.mark.parametrize("d", [1, 7, 33, 256])
def test_similarities_other_widths(d):
    """Widths the cases do not have: one column, lane tails on the scalar route, four 16-byte loads per lane."""
    from frl_hip.losses import pair_similarity
    z = SC.make_rows(50, d, 300 + d)
    pairs = np.random.default_rng(d).integers(0, 50, (333, 2))
    pairs[0] = (4, 4)                                                                                   # a pair with itself: exactly 0
    got = pair_similarity(_dev(z), _dev(pairs)).cpu().numpy()
    want = SC.sims(z, pairs)
    assert got[0] == 0.0 and (np.abs(got - want) <= 2e-6 * np.abs(want)).all()


def test_similarity_edge_cases():
    from frl_hip import ops
    from frl_hip.losses import pair_similarity, pair_similarity_stats
    z = SC.make_rows(20, 16, 400)
    zt = _dev(z)
    one, three = _dev(np.asarray([[2, 9]])), _dev(np.asarray([[0, 1], [5, 6], [7, 19]]))
    empty = torch.zeros((0, 2), dtype=torch.long, device=DEV)
    st = pair_similarity_stats(zt, one, three, 0.1)
    assert np.isnan(st["pos_std"]) and abs(st["pos_mean"] - SC.sims(z, np.asarray([[2, 9]]))[0]) <= 2e-6 * abs(st["pos_mean"])     # torch.std of one value
    assert np.isfinite(st["neg_std"])
    assert pair_similarity_stats(zt, empty, three, 0.1) is None and pair_similarity_stats(zt, three, empty, 0.1) is None
    assert pair_similarity(zt, empty).shape == (0,)
    # bfloat16 rows are converted: the float32 call on the converted rows, bit for bit
    zb = zt.to(torch.bfloat16)
    assert torch.equal(pair_similarity(zb, three), pair_similarity(zb.float(), three))
    assert pair_similarity_stats(zb, three, three, 0.1) == pair_similarity_stats(zb.float(), three, three, 0.1)
    # rows out of range: negative ones wrap as torch indexing does, the rest is clamped and flagged
    ops.index_errors()
    assert torch.equal(pair_similarity(zt, _dev(np.asarray([[-1, 0], [3, -20]]))), pair_similarity(zt, _dev(np.asarray([[19, 0], [3, 0]]))))
    assert not ops.index_errors()
    got = pair_similarity(zt, _dev(np.asarray([[0, 20], [-21, 3], [1 << 40, 2]])))
    assert torch.equal(got, pair_similarity(zt, _dev(np.asarray([[0, 19], [0, 3], [19, 2]]))))
    assert ops.index_errors() and not ops.index_errors()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASE_NAMES)
def test_global_spectral_infonce_matches_reference(golden_dir, case):
    from frl_hip.losses import global_spectral_infonce
    fx, c, inp = _fx(golden_dir, case), SC.CASES[case], SC.make_inputs(case)
    z = _dev(inp["z"]).requires_grad_(True)
    spec = _dev(inp["spec"]).requires_grad_(True)
    coords = [_dev(x) for x in inp["coords"]]
    loss, info = global_spectral_infonce(z, spec, coords, inp["offsets"], positive_k=c["k"], positive_min_spatial=SC.MIN_SPATIAL,
                                         neg_per_anchor=c["neg_per_anchor"], neg_tau=SC.TAU, neg_min_weight=SC.MIN_W,
                                         temperature=SC.TEMPERATURE, draws=_dev(inp["draws"]))
    assert loss.dim() == 0
    assert np.array_equal(info["pos_pairs"].cpu().numpy(), fx["pos"]) and np.array_equal(info["neg_pairs"].cpu().numpy(), fx["neg"])
    assert info["n_pos"] == len(fx["pos"]) and info["n_neg"] == len(fx["neg"])
    assert np.abs(info["neg_weights"].cpu().numpy() - fx["neg_w"]).max() <= 2e-6
    want = float(fx["loss"])
    print(f"{case}: loss {loss.item()!r} against {want!r}")
    assert abs(loss.item() - want) <= 2e-6 * max(1.0, abs(want))
    loss.backward()
    scale = max(1e-6, np.abs(fx["grad"]).max())
    err = np.abs(z.grad.cpu().numpy() - fx["grad"]).max()
    print(f"{case}: gradient error {err / scale:.2e} of the largest entry")
    assert err <= 1e-5 * scale
    assert spec.grad is None                                                                            # the spectral rows are data
    for key, v in zip(("pos_mean", "pos_std", "neg_mean", "neg_std"), fx["stats"]):
        assert abs(info["sim_stats"][key] - v) <= 5e-6 * max(1.0, abs(v)), key
    assert info["sim_stats"]["temperature"] == SC.TEMPERATURE
    _, quiet = global_spectral_infonce(z.detach(), spec.detach(), coords, inp["offsets"], positive_k=c["k"], neg_per_anchor=c["neg_per_anchor"],
                                       draws=_dev(inp["draws"]), stats=False)
    assert quiet["sim_stats"] is None


def test_global_spectral_infonce_one_and_zero_patches():
    from frl_hip.losses import contrastive_loss, global_spectral_infonce
    inp = SC.make_inputs("c")
    z, spec = _dev(inp["z"][:40]).requires_grad_(True), _dev(inp["spec"][:40])
    loss, info = global_spectral_infonce(z, spec, [_dev(inp["coords"][0])], [0, 40], positive_k=8)
    assert info["n_neg"] == 0 and info["neg_pairs"].shape == (0, 2) and info["n_pos"] > 0 and info["sim_stats"] is None
    assert torch.isfinite(loss) and loss.dim() == 0
    assert loss.item() == contrastive_loss(z, info["pos_pairs"], info["neg_pairs"]).item()              # InfoNCE without negatives
    loss.backward()
    assert torch.isfinite(z.grad).all()
    zero, info = global_spectral_infonce(torch.zeros(0, 8, device=DEV), torch.zeros(0, 1, device=DEV), [], [0])
    assert zero.dim() == 0 and zero.item() == 0.0 and info["n_pos"] == 0 and info["n_neg"] == 0 and info["sim_stats"] is None
