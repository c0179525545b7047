"""GPU parity of the phase margin losses (csrc/phase_margin.hip: recovery discrimination and spread ranking) against the fixtures written by
the REFERENCE's functions (tests/golden/make_phase_margin_golden.py) and, where a fixture holds part of a gradient or no fixture is
committed, against the float64 restatement (tests/phase_margin_cases.py, pinned to the fixtures by tests/test_cpu_phase_margin.py).
Bounds: those of the soft-neighbourhood parity tests for a float32 kernel against a float64 reference: 2e-6 * max(1, |loss64|) on losses
and on the mean statistics, 1e-5 * max|grad64| on gradients; counts are equal.  bfloat16 embeddings: the restatement on the rounded
values, the same loss bound, 2^-8 |g64| + 1e-5 max|g64| per gradient element (the gradient is rounded to bfloat16 once)."""
import os

import numpy as np
import pytest
import torch

import phase_margin_cases as PC
import soft_neighborhood_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["a", "b", "c", "d", "e"]


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


def _check_loss(got, want, what):
    got, want = float(got.detach()) if torch.is_tensor(got) else float(got), float(want)
    print(f"{what}: got {got!r} want {want!r} dev {abs(got - want):.3e} bound {2e-6 * max(1.0, abs(want)):.3e}")
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), what


def _check_grad(g, g64, what, scale=None):
    g64 = np.asarray(g64, dtype=np.float64)
    scale = np.abs(g64).max(initial=0.0) if scale is None else float(scale)
    g = g.detach().double().cpu().numpy() if torch.is_tensor(g) else np.asarray(g, dtype=np.float64)
    dev = np.abs(g.reshape(g64.shape) - g64).max(initial=0.0)
    print(f"{what} grad: dev {dev:.3e} max|g64| {scale:.3e} bound {1e-5 * scale:.3e}")
    assert np.isfinite(dev) and dev <= 1e-5 * scale, what


def _check_grad_bf16(g, g64, what):
    g64 = g64.numpy() if torch.is_tensor(g64) else np.asarray(g64, dtype=np.float64)
    dev = np.abs(g.double().cpu().numpy().reshape(g64.shape) - g64)
    bound = 2.0 ** -8 * np.abs(g64) + 1e-5 * np.abs(g64).max()
    print(f"{what} bf16 grad: worst dev / bound {(dev / bound).max():.3f}")
    assert (dev <= bound).all(), what


def _check_spread_stats(stats, want, what):
    for key in PC.SPREAD_COUNTS:
        assert stats[key] == int(want[key]), f"{what} {key}: {stats[key]} != {want[key]}"
    for key in PC.SPREAD_MEANS:
        _check_loss(stats[key], want[key], f"{what} {key}")


def _fx_stats(fx):
    return {k[5:]: float(fx[k]) for k in fx.files if k.startswith("stat_")}


# ---------------------------------------------------------------------------------------------------------------------------
# recovery discrimination
# ---------------------------------------------------------------------------------------------------------------------------
def _recovery_kw(fx):
    return dict(margin=float(fx["margin"]), low_ysfc_max=float(fx["low_ysfc_max"]), high_ysfc_min=float(fx["high_ysfc_min"]))


def _run_recovery(z, ysfc, factor=1.0, **kw):
    from frl_hip.losses import phase_recovery_discrimination_loss
    zz = z.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = phase_recovery_discrimination_loss(zz, ysfc.to(DEV), **kw)
    (factor * loss).backward()
    return loss.detach(), stats, zz.grad


@pytest.fixture(scope="module")
def recovery_b(golden_dir):
    fx = _fx(golden_dir, "recovery_disc_b")
    z, ysfc, kw = torch.from_numpy(fx["z"]), torch.from_numpy(fx["ysfc"]), _recovery_kw(fx)
    return fx, z, ysfc, kw, PC.recovery_f64(z, ysfc, **kw)


@pytest.mark.parametrize("case", CASES)
def test_recovery_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"recovery_disc_{case}")
    z, ysfc, kw = torch.from_numpy(fx["z"]), torch.from_numpy(fx["ysfc"]), _recovery_kw(fx)
    loss, stats, g = _run_recovery(z, ysfc, **kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype == torch.float32 and g.shape == z.shape
    _check_loss(loss, fx["loss64"], case)
    assert stats == {"n_pairs": int(fx["stat_n_pairs"]), "n_active_pixels": int(fx["stat_n_active_pixels"])}
    assert torch.isfinite(g).all()
    _check_grad(g[torch.from_numpy(fx["grad_pixels"]).to(DEV)], fx["grad64"], case, scale=fx["grad_max"])
    _, _, g64 = PC.recovery_f64(z, ysfc, **kw)                            # every row, where the fixture holds some
    _check_grad(g, g64.numpy(), case + " all rows", scale=fx["grad_max"])
    low, high = PC.recovery_classes(ysfc, kw["low_ysfc_max"], kw["high_ysfc_min"])
    inactive = ~(low.any(dim=1) & high.any(dim=1))
    assert not g[inactive.to(DEV)].any()                                 # zeros written, not left over
    if case == "d":
        assert float(loss) == 0.0 and not g.any()
    loss2, _, g2 = _run_recovery(z, ysfc, **kw)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)              # identical bits from run to run


@pytest.mark.parametrize("n,t,d,margin", [(5, 1, 1, 0.5), (7, 2, 3, 0.5), (9, 32, 100, 0.5), (6, 32, 128, 0.5), (5, 32, 256, 0.5), (3, 17, 255, 0.5),
                                          (260, 15, 12, 25.0), (1030, 2, 3, 0.5)])
def test_recovery_shapes_match_the_restatement(n, t, d, margin):
    # the widths at which four, three, two and one pixel share a workgroup, forward and backward; margin 25: softplus past its threshold;
    # N = 1030: more pixels than the 1024 threads of the final reduction
    z = SC.make_points(n, t, d, seed=n + t + d, scale=0.05)
    ysfc = PC.plant_invalid(SC.make_ysfc(n, t, seed=n * t + d), seed=d, nan_frac=0.1, neg_frac=0.05)
    ysfc[0, :] = float("nan")
    if t > 1:
        ysfc[1, 0], ysfc[1, 1:] = 0.0, 7.0                              # one low against all the others high, whatever the draw
    kw = dict(margin=margin, low_ysfc_max=2.0, high_ysfc_min=2.0 if t == 1 else 3.0)
    want_loss, want_stats, g64 = PC.recovery_f64(z, ysfc, upstream=3.0, **kw)
    loss, stats, g = _run_recovery(z, ysfc, factor=3.0, **kw)
    what = f"N={n} T={t} D={d}"
    _check_loss(loss, want_loss, what)
    assert stats == want_stats and (t == 1 or stats["n_pairs"] > 0)
    _check_grad(g, g64.numpy(), what)


def test_recovery_bfloat16_embeddings(recovery_b):
    fx, z, ysfc, kw, _ = recovery_b
    z16 = z.to(torch.bfloat16)
    want_loss, want_stats, g64 = PC.recovery_f64(z16, ysfc, **kw)      # on the bf16-rounded values
    loss, stats, g = _run_recovery(z16, ysfc, **kw)
    assert loss.dtype == torch.float32 and g.dtype == torch.bfloat16
    _check_loss(loss, want_loss, "recovery b bf16")
    assert stats == want_stats
    _check_grad_bf16(g, g64, "recovery b")


def test_recovery_upstream_stats_off_frozen_and_strided(recovery_b):
    from frl_hip.losses import phase_recovery_discrimination_loss
    fx, z, ysfc, kw, (_, _, g64) = recovery_b
    loss, stats, g = _run_recovery(z, ysfc, **kw)
    _, _, g3 = _run_recovery(z, ysfc, factor=3.0, **kw)                 # (3 * loss).backward()
    _check_grad(g3, 3.0 * g64.numpy(), "recovery b, upstream 3")
    zd, yd = z.to(DEV), ysfc.to(DEV)
    l0, s0 = phase_recovery_discrimination_loss(zd, yd, stats=False, **kw)
    assert s0 == {} and torch.equal(l0, loss) and not l0.requires_grad  # frozen input: nothing to differentiate, no backward launch
    # a permuted view: accepted, the result of its contiguous copy, the gradient back in the view's layout
    base = z.permute(1, 0, 2).contiguous().to(DEV).requires_grad_(True)  # [T, N, D]
    lp, sp = phase_recovery_discrimination_loss(base.permute(1, 0, 2), yd.double(), **kw)
    lp.backward()
    assert not base.permute(1, 0, 2).is_contiguous() and torch.equal(lp.detach(), loss) and sp == stats
    assert torch.equal(base.grad.permute(1, 0, 2), g)


# ---------------------------------------------------------------------------------------------------------------------------
# spread ranking
# ---------------------------------------------------------------------------------------------------------------------------
def _spread(golden_dir, case):
    from frl_hip.losses import phase_alignment
    fx = _fx(golden_dir, f"spread_rank_{case}")
    t = {k: torch.from_numpy(fx[k]) for k in ("phase", "ysfc", "pairs", "dynamism")}
    kw = dict(margin=float(fx["margin"]), delta=float(fx["delta"]))
    valid, rows_i, rows_j, lengths = phase_alignment(t["ysfc"], t["pairs"], int(fx["min_overlap"]))
    pairs = t["pairs"][valid]
    ref_diff = t["dynamism"][pairs[:, 0]] - t["dynamism"][pairs[:, 1]]
    return fx, t, kw, (valid, rows_i, rows_j, lengths), pairs, ref_diff


def _blocks32(fx):
    """The fixture's float64 blocks rounded to float32 (what a float32 caller holds), zero where masked, and the mask."""
    mask = fx["mask_self"]
    out = []
    for key in ("d_self_i", "d_self_j"):
        full = np.zeros(mask.shape, dtype=np.float64)
        full[mask] = fx[key]
        out.append(torch.from_numpy(full).float())
    return out[0], out[1], torch.from_numpy(mask)


def _run_matrix(d_i, d_j, mask, pairs, dynamism, factor=1.0, **kw):
    from frl_hip.losses import compute_phase_spread_ranking
    di, dj = d_i.to(DEV).clone().requires_grad_(True), d_j.to(DEV).clone().requires_grad_(True)
    batch = {"d_learned_self": di, "d_learned_self_j": dj, "mask_self": mask.to(DEV)}
    loss, stats = compute_phase_spread_ranking(batch, pairs[:, 0].to(DEV), pairs[:, 1].to(DEV), dynamism.to(DEV), **kw)
    (factor * loss).backward()
    return loss.detach(), stats, di.grad, dj.grad


def _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, factor=1.0, **kw):
    from frl_hip.losses import phase_spread_ranking_gathered
    e = emb.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = phase_spread_ranking_gathered(e, rows_i.to(DEV), rows_j.to(DEV), lengths.to(DEV), ref_diff.to(DEV), **kw)
    (factor * loss).backward()
    return loss.detach(), stats, e.grad


def _run_convenience(t, min_overlap, factor=1.0, **kw):
    from frl_hip.losses import phase_spread_ranking_loss
    z = t["phase"].to(DEV).clone().requires_grad_(True)
    loss, stats = phase_spread_ranking_loss(z, t["ysfc"].to(DEV), t["pairs"].to(DEV), t["dynamism"].to(DEV), min_overlap=min_overlap, **kw)
    (factor * loss).backward()
    return loss.detach(), stats, z.grad


@pytest.mark.parametrize("case", ["a", "b", "c", "e"])
def test_spread_forms_match_reference_fixture(golden_dir, case):
    fx, t, kw, (_, rows_i, rows_j, lengths), pairs, ref_diff = _spread(golden_dir, case)
    want = _fx_stats(fx)
    n, tt, d = t["phase"].shape
    # matrix form on the reference's blocks
    d_i, d_j, mask = _blocks32(fx)
    loss_m, stats_m, gi, gj = _run_matrix(d_i, d_j, mask, pairs, t["dynamism"], **kw)
    assert loss_m.dtype == torch.float32 and loss_m.dim() == 0 and gi.dtype == torch.float32 and gi.shape == d_i.shape == gj.shape
    _check_loss(loss_m, fx["loss64"], case + " matrix")
    _check_spread_stats(stats_m, want, case + " matrix")
    want_gi = fx["grad64_pair"].reshape(-1, 1, 1) * fx["mask_self"]
    _check_grad(gi, want_gi, case + " matrix d_i")
    _check_grad(gj, -want_gi, case + " matrix d_j")
    # gathered form on the rows of phase_alignment
    emb = t["phase"].reshape(n * tt, d)
    loss_g, stats_g, ge = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, **kw)
    assert loss_g.dtype == torch.float32 and ge.dtype == torch.float32 and ge.shape == emb.shape and torch.isfinite(ge).all()
    _check_loss(loss_g, fx["loss64"], case + " gathered")
    _check_spread_stats(stats_g, want, case + " gathered")
    _check_grad(ge, fx["grad64"].reshape(n * tt, d), case + " gathered")
    # convenience form on the raw inputs
    loss_c, stats_c, gc = _run_convenience(t, int(fx["min_overlap"]), **kw)
    _check_loss(loss_c, fx["loss64"], case + " convenience")
    _check_spread_stats(stats_c, want, case + " convenience")
    _check_grad(gc, fx["grad64"], case + " convenience")
    assert torch.equal(loss_c, loss_g) and torch.equal(gc.reshape(ge.shape), ge)
    if case == "c":
        assert float(loss_g) == 0.0 and float(loss_m) == 0.0 and not ge.any() and not gi.any() and not gj.any()
    # identical bits from run to run
    loss2, _, ge2 = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, **kw)
    loss3, _, gi3, gj3 = _run_matrix(d_i, d_j, mask, pairs, t["dynamism"], **kw)
    assert torch.equal(loss_g, loss2) and torch.equal(ge, ge2) and torch.equal(loss_m, loss3) and torch.equal(gi, gi3) and torch.equal(gj, gj3)


def test_spread_without_valid_pairs_launches_nothing(golden_dir, monkeypatch):
    from frl_hip import ops
    from frl_hip.losses import compute_phase_spread_ranking, phase_spread_ranking_gathered
    fx, t, kw, (valid, rows_i, rows_j, lengths), pairs, ref_diff = _spread(golden_dir, "d")

    def refuse(*a, **k):
        raise AssertionError("a kernel wrapper was called")
    for name in ("spread_rank_fwd", "spread_rank_gathered_fwd", "spread_rank_bwd", "spread_rank_gathered_bwd"):
        monkeypatch.setattr(ops, name, refuse)
    empty = _fx_stats(fx)
    loss, stats, g = _run_convenience(t, int(fx["min_overlap"]), **kw)
    assert not valid.any() and float(loss) == 0.0 == float(fx["loss64"]) and stats == {k: (int(v) if k in PC.SPREAD_COUNTS else v) for k, v in empty.items()}
    assert g is None or not g.any()
    e = t["phase"].reshape(-1, 12).to(DEV).requires_grad_(True)
    loss, stats = phase_spread_ranking_gathered(e, rows_i.to(DEV), rows_j.to(DEV), lengths.to(DEV), ref_diff.to(DEV), **kw)
    assert float(loss.detach()) == 0.0 and loss.requires_grad and stats["n_pairs"] == 0 and stats["frac_satisfied"] == 1.0
    batch = {"d_learned_self": torch.zeros(0, 5, 5, device=DEV), "d_learned_self_j": torch.zeros(0, 5, 5, device=DEV),
             "mask_self": torch.zeros(0, 5, 5, dtype=torch.bool, device=DEV)}
    loss, stats = compute_phase_spread_ranking(batch, pairs[:, 0].to(DEV), pairs[:, 1].to(DEV), t["dynamism"].to(DEV), **kw)
    assert float(loss.detach()) == 0.0 and loss.requires_grad and stats["n_pairs"] == 0


@pytest.fixture(scope="module")
def spread_b(golden_dir):
    return _spread(golden_dir, "b")


def test_spread_bfloat16_embeddings(spread_b):
    fx, t, kw, (_, rows_i, rows_j, lengths), pairs, ref_diff = spread_b
    emb16 = t["phase"].reshape(-1, 12).to(torch.bfloat16)
    want_loss, want_stats, g64 = PC.spread_gathered_f64(emb16, rows_i, rows_j, lengths, ref_diff, **kw)   # on the bf16-rounded values
    (d_i, mask), (d_j, _) = PC.self_distance_blocks(emb16, rows_i, lengths), PC.self_distance_blocks(emb16, rows_j, lengths)
    _, _, _, (si, sj) = PC.spread_matrix_f64(d_i, d_j, mask, ref_diff, **kw)
    con = ref_diff.abs() > kw["delta"]
    assert bool((((si - sj).abs() - kw["margin"]).abs()[con] > 1e-4).all())            # no constrained pair on the margin after rounding either
    loss, stats, g = _run_gathered(emb16, rows_i, rows_j, lengths, ref_diff, **kw)
    assert loss.dtype == torch.float32 and g.dtype == torch.bfloat16
    _check_loss(loss, want_loss, "spread b bf16")
    _check_spread_stats(stats, want_stats, "spread b bf16")
    _check_grad_bf16(g, g64, "spread b")


def test_spread_upstream_stats_off_frozen_and_strided(spread_b):
    from frl_hip.losses import compute_phase_spread_ranking, phase_spread_ranking_gathered, phase_spread_ranking_loss
    fx, t, kw, (valid, rows_i, rows_j, lengths), pairs, ref_diff = spread_b
    n, tt, d = t["phase"].shape
    emb = t["phase"].reshape(n * tt, d)
    loss, stats, g = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, **kw)
    _, _, g3 = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, factor=3.0, **kw)
    _check_grad(g3, 3.0 * fx["grad64"].reshape(n * tt, d), "spread b gathered, upstream 3")
    d_i, d_j, mask = _blocks32(fx)
    loss_m, _, gi, gj = _run_matrix(d_i, d_j, mask, pairs, t["dynamism"], **kw)
    _, _, gi3, gj3 = _run_matrix(d_i, d_j, mask, pairs, t["dynamism"], factor=3.0, **kw)
    _check_grad(gi3, 3.0 * fx["grad64_pair"].reshape(-1, 1, 1) * fx["mask_self"], "spread b matrix, upstream 3")
    assert torch.equal(gj3, -gi3)
    # stats=False: an empty dict, the same loss bits; frozen inputs: nothing to differentiate
    args = [x.to(DEV) for x in (emb, rows_i, rows_j, lengths, ref_diff)]
    l0, s0 = phase_spread_ranking_gathered(*args, stats=False, **kw)
    assert s0 == {} and torch.equal(l0, loss) and not l0.requires_grad
    raw = [t[k].to(DEV) for k in ("phase", "ysfc", "pairs", "dynamism")]
    l0, s0 = phase_spread_ranking_loss(*raw, min_overlap=int(fx["min_overlap"]), stats=False, **kw)
    assert s0 == {} and torch.equal(l0, loss) and not l0.requires_grad
    batch = {"d_learned_self": d_i.to(DEV), "d_learned_self_j": d_j.to(DEV).requires_grad_(True), "mask_self": mask.to(DEV)}
    l0, s0 = compute_phase_spread_ranking(batch, pairs[:, 0].to(DEV), pairs[:, 1].to(DEV), raw[3], stats=False, **kw)
    l0.backward()                                                        # one block frozen: the other still gets its gradient
    assert s0 == {} and torch.equal(l0.detach(), loss_m) and torch.equal(batch["d_learned_self_j"].grad, gj) and batch["d_learned_self"].grad is None
    batch["d_learned_self_j"] = d_j.to(DEV)
    assert not compute_phase_spread_ranking(batch, pairs[:, 0].to(DEV), pairs[:, 1].to(DEV), raw[3], **kw)[0].requires_grad
    # an alignment made once is taken as given; a permuted embedding tensor gives the result of its contiguous copy
    base = t["phase"].permute(1, 0, 2).contiguous().to(DEV).requires_grad_(True)     # [T, N, D]
    align = tuple(x.to(DEV) for x in (valid, rows_i, rows_j, lengths))
    lp, sp = phase_spread_ranking_loss(base.permute(1, 0, 2), raw[1], raw[2], raw[3], min_overlap=99, alignment=align, **kw)
    lp.backward()
    assert torch.equal(lp.detach(), loss) and sp == stats and torch.equal(base.grad.permute(1, 0, 2).reshape(n * tt, d), g)


def test_spread_gathered_and_matrix_forms_agree(spread_b):
    fx, t, kw, (_, rows_i, rows_j, lengths), pairs, ref_diff = spread_b
    emb = t["phase"].reshape(-1, 12)
    d_i, mask = PC.self_distance_blocks(emb, rows_i, lengths)           # float64 distances of the gathered rows, rounded to float32
    d_j, _ = PC.self_distance_blocks(emb, rows_j, lengths)
    loss_m, stats_m, _, _ = _run_matrix(d_i.float(), d_j.float(), mask, pairs, t["dynamism"], **kw)
    loss_g, stats_g, _ = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, **kw)
    _check_loss(loss_g, float(loss_m), "gathered vs matrix")
    assert all(stats_g[k] == stats_m[k] for k in PC.SPREAD_COUNTS) and stats_g["frac_satisfied"] == stats_m["frac_satisfied"]


@pytest.mark.parametrize("m,d", [(1, 12), (2, 1), (3, 12), (32, 12), (32, 100), (32, 128), (32, 256), (17, 255)])
def test_spread_gathered_shapes_match_the_restatement(m, d):
    b, r = 11, 40                                                        # 40 rows shared by 11 * m * 2 positions: repeated rows across pairs
    emb = SC.make_points(1, r, d, seed=m + d, scale=0.25)[0]
    g = torch.Generator().manual_seed(m * 1000 + d)
    rows_i, rows_j = (torch.randint(0, r, (b, m), generator=g, dtype=torch.int64) for _ in range(2))
    if m > 1:
        rows_i[0, 1] = rows_i[0, 0]                                      # a repeated row inside a pair: a zero distance off the diagonal
    rows_j[1] = rows_i[1]                                                # an (i, i) pair
    lengths = SC.make_lengths(b, 0, m, seed=m + d)
    lengths[0], lengths[1], lengths[2], lengths[3] = m, m, 0, 1          # full pairs, an empty one, a single position
    ref_diff = SC.grid(torch.tensor([1.0, 1.0, -1.0, 1.0, 0.5, -0.5, 0.75, -0.75, 2.0, -2.0, 0.0]))
    kw = dict(margin=0.1, delta=0.5)
    want_loss, want_stats, g64 = PC.spread_gathered_f64(emb, rows_i, rows_j, lengths, ref_diff, upstream=3.0, **kw)
    loss, stats, ge = _run_gathered(emb, rows_i, rows_j, lengths, ref_diff, factor=3.0, **kw)
    what = f"M={m} D={d}"
    _check_loss(loss, want_loss, what)
    _check_spread_stats(stats, want_stats, what)
    assert torch.isfinite(ge).all()
    _check_grad(ge, g64.numpy(), what)


@pytest.mark.parametrize("b,m", [(1, 1), (5, 2), (7, 33), (3, 70), (1030, 5)])
def test_spread_matrix_shapes_match_the_restatement(b, m):
    d_i, d_j = SC.make_distances(b, m, seed=2000 + 7 * b + m)
    mask = SC.make_random_mask(b, m, seed=b * m, keep=0.7, lengths=SC.make_lengths(b, 0, m, seed=b + m))
    ref_diff = PC.make_dynamism(b, seed=b + 3 * m)
    kw = dict(margin=0.1, delta=0.5)
    want_loss, want_stats, (gi64, gj64), _ = PC.spread_matrix_f64(d_i, d_j, mask, ref_diff, upstream=3.0, **kw)
    dyn = torch.cat([ref_diff, torch.zeros(1)])                          # pair b = (b, the zero entry): r_b = ref_diff[b]
    pairs = torch.stack([torch.arange(b), torch.full((b,), b)], dim=1)
    loss, stats, gi, gj = _run_matrix(d_i, d_j, mask, pairs, dyn, factor=3.0, **kw)
    what = f"B={b} M={m}"
    _check_loss(loss, want_loss, what)
    for key in PC.SPREAD_COUNTS:
        assert stats[key] == want_stats[key], key
    for key in ("mean_spread_i", "mean_spread_j", "mean_ref_diff"):
        _check_loss(stats[key], want_stats[key], f"{what} {key}")
    _check_grad(gi, gi64.numpy(), what + " d_i")
    _check_grad(gj, gj64.numpy(), what + " d_j")
