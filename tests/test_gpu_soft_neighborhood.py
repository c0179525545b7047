"""GPU parity of the fused soft-neighbourhood matching loss (csrc/soft_neighborhood.hip) against the fixtures written by the REFERENCE's
functions (tests/golden/make_soft_neighborhood_golden.py) and, for shapes not committed, against the float64 restatement
(tests/soft_neighborhood_cases.py).  Bounds: those of the InfoNCE and VICReg parity tests for the same kind of comparison:
2e-6 * max(1, |loss64|) on losses (and on the mean statistics), 1e-5 * max|grad64| on gradients; counts are equal."""
import os

import numpy as np
import pytest
import torch

import soft_neighborhood_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = ("n_pairs", "n_pairs_active", "n_rows_total", "n_rows_valid")
MEANS = ("mean_kl", "mean_overlap", "mean_entropy_p", "mean_entropy_q")


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


def _kw(fx, dev=DEV):
    return dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), min_valid_per_row=int(fx["min_valid_per_row"]),
                pair_weights=torch.from_numpy(fx["pair_weights"]).to(dev) if "pair_weights" in fx.files else None)


def _check_loss(got, want, what):
    got, want = float(got.detach()) if torch.is_tensor(got) else float(got), float(want)
    print(f"{what}: got {got!r} want {want!r} dev {abs(got - want):.3e} bound {2e-6 * max(1.0, abs(want)):.3e}")
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), what


def _check_grad(g, g64, what):
    g64 = np.asarray(g64, dtype=np.float64)
    scale = np.abs(g64).max(initial=0.0)
    dev = np.abs(g.detach().double().cpu().numpy().reshape(g64.shape) - g64).max(initial=0.0)
    print(f"{what} grad: dev {dev:.3e} max|g64| {scale:.3e} bound {1e-5 * scale:.3e}")
    assert np.isfinite(dev) and dev <= 1e-5 * scale, what


def _check_stats(stats, want, what):
    for key in COUNTS:
        if key in want:
            assert stats[key] == int(want[key]), f"{what} {key}: {stats[key]} != {want[key]}"
    for key in MEANS:
        if key in want:
            _check_loss(stats[key], want[key], f"{what} {key}")


def _fx_stats(fx):
    return {k[5:]: float(fx[k]) for k in fx.files if k.startswith("stat_")}


def _matrices(fx):
    return torch.from_numpy(fx["d_reference"]), torch.from_numpy(fx["d_learned"])


def _run_matrix(d_ref, d_learned, mask, factor=1.0, **kw):
    from frl_hip.losses import soft_neighborhood_matching_loss
    dl = d_learned.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = soft_neighborhood_matching_loss(d_ref.to(DEV), dl, mask.to(DEV), **kw)
    (factor * loss).backward()
    return loss.detach(), stats, dl.grad


def _point_rows(fx):
    """The fixture's points as rows of one matrix: (ref [2BM, C], emb [2BM, D], rows a [B, M], rows b [B, M])."""
    b, m, d = fx["emb_a"].shape
    ref = torch.cat([torch.from_numpy(fx["ref_a"]).reshape(b * m, -1), torch.from_numpy(fx["ref_b"]).reshape(b * m, -1)])
    emb = torch.cat([torch.from_numpy(fx["emb_a"]).reshape(b * m, d), torch.from_numpy(fx["emb_b"]).reshape(b * m, d)])
    ra = torch.arange(b * m).reshape(b, m)
    return ref, emb, ra, (ra if bool(fx["shared"]) else ra + b * m)


def _run_gathered(ref, emb, ra, rb, ea, eb, lengths, excl, factor=1.0, **kw):
    from frl_hip.losses import soft_neighborhood_loss_gathered
    e = emb.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = soft_neighborhood_loss_gathered(ref.to(DEV), e, ra.to(DEV), rb.to(DEV), ea.to(DEV), eb.to(DEV), lengths.to(DEV), excl, **kw)
    (factor * loss).backward()
    return loss.detach(), stats, e.grad


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e", "f"])
def test_matrix_form_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"soft_nbr_{case}")
    d_ref, d_learned = _matrices(fx)
    want_loss, want_stats, want_grad = float(fx["loss64"]), _fx_stats(fx), fx["grad64"]
    loss, stats, g = _run_matrix(d_ref, d_learned, torch.from_numpy(fx["mask"]), **_kw(fx))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype == torch.float32 and g.shape == d_learned.shape
    _check_loss(loss, want_loss, case)
    _check_stats(stats, want_stats, case)
    _check_grad(g, want_grad, case)
    if case == "e":
        assert float(loss) == 0.0 and not g.any()
    loss2, _, g2 = _run_matrix(d_ref, d_learned, torch.from_numpy(fx["mask"]), **_kw(fx))
    assert torch.equal(loss, loss2) and torch.equal(g, g2)              # identical bits from run to run


@pytest.mark.parametrize("case", ["b", "c", "f"])
def test_gathered_form_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, f"soft_nbr_{case}")
    ref, emb, ra, rb = _point_rows(fx)
    lengths, excl = torch.from_numpy(fx["lengths"]), bool(fx["exclude_diagonal"])
    loss, stats, g = _run_gathered(ref, emb, ra, rb, ra, rb, lengths, excl, **_kw(fx))
    assert loss.dtype == torch.float32 and g.dtype == torch.float32 and g.shape == emb.shape
    _check_loss(loss, fx["loss64_points"], case)
    _check_stats(stats, {k: v for k, v in _fx_stats(fx).items() if k != "mean_kl"}, case)
    want = np.concatenate([fx["grad64_emb_a"].reshape(-1, emb.shape[1]), fx["grad64_emb_b"].reshape(-1, emb.shape[1])])
    _check_grad(g, want, case)
    loss2, _, g2 = _run_gathered(ref, emb, ra, rb, ra, rb, lengths, excl, **_kw(fx))
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    # the matrix form on the same data, within the bounds
    d_ref, d_learned = _matrices(fx)
    loss_m, stats_m, _ = _run_matrix(d_ref, d_learned, torch.from_numpy(fx["mask"]), **_kw(fx))
    _check_loss(loss, float(loss_m), case + " gathered vs matrix")
    assert all(stats[k] == stats_m[k] for k in COUNTS)


@pytest.fixture(scope="module")
def phase(golden_dir):
    fx = _fx(golden_dir, "phase_nbr_a")
    kw = dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), min_overlap=int(fx["min_overlap"]),
              min_valid_per_row=int(fx["min_valid_per_row"]), self_similarity_weight=float(fx["self_similarity_weight"]),
              cross_pixel_weight=float(fx["cross_pixel_weight"]))
    t = {k: torch.from_numpy(fx[k]).to(DEV) for k in ("spectral", "phase", "ysfc", "pairs", "weights")}
    return fx, kw, t


def _run_phase(t, kw, factor=1.0, **extra):
    from frl_hip.losses import phase_neighborhood_loss
    z = t["phase"].clone().requires_grad_(True)
    loss, stats = phase_neighborhood_loss(t["spectral"], z, t["ysfc"], t["pairs"], pair_weights=t["weights"], **{**kw, **extra})
    (factor * loss).backward()
    return loss.detach(), stats, z.grad


def test_phase_neighborhood_loss_matches_reference_fixture(phase):
    fx, kw, t = phase
    loss, stats, g = _run_phase(t, kw)
    _check_loss(loss, fx["loss64"], "phase loss")
    want = _fx_stats(fx)
    for key in ("loss_self", "loss_cross"):
        _check_loss(stats[key], want[key], key)
    assert stats["n_pairs_input"] == 200 and stats["n_pairs_sufficient_overlap"] == int(fx["valid_pair_mask"].sum()) == int(want["n_pairs_sufficient_overlap"])
    for prefix in ("self_", "cross_"):
        _check_stats({k[len(prefix):]: v for k, v in stats.items() if k.startswith(prefix)},
                     {k[len(prefix):]: v for k, v in want.items() if k.startswith(prefix)}, prefix)
    assert not any(k.startswith("d_ref_") for k in stats)
    assert g.shape == t["phase"].shape and torch.isfinite(g).all()      # finite despite the self-pairs' zero distances
    _check_grad(g, fx["grad64"], "phase")
    loss2, _, g2 = _run_phase(t, kw)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


def test_phase_batch_path_and_upstream_factor(phase):
    from frl_hip.losses import phase_neighborhood_loss
    fx, kw, t = phase
    bv, m = fx["mask_self"].shape[:2]
    batch = {"valid_pair_mask": torch.from_numpy(fx["valid_pair_mask"]).to(DEV), "M": m}
    for key, mk in (("d_ref_self", "mask_self"), ("d_learned_self", "mask_self"), ("d_ref_cross", "mask_cross"), ("d_learned_cross", "mask_cross")):
        full = np.zeros((bv, m, m), dtype=np.float64)
        full[fx[mk]] = fx[key]
        batch[key] = torch.from_numpy(full).float().to(DEV)
        batch[mk] = torch.from_numpy(fx[mk]).to(DEV)
    loss, stats = phase_neighborhood_loss(t["spectral"], t["phase"], t["ysfc"], t["pairs"], pair_weights=t["weights"], _batch=batch, **kw)
    _check_loss(loss, fx["loss64"], "phase loss from the reference batch")
    assert stats["n_pairs_sufficient_overlap"] == bv
    _, _, g3 = _run_phase(t, kw, factor=3.0)                             # (3 * loss).backward()
    _check_grad(g3, 3.0 * fx["grad64"], "phase, upstream 3")
    loss0, stats0, g0 = _run_phase(t, kw, self_similarity_weight=0.0)
    _check_loss(loss0, float(fx["cross_pixel_weight"]) * float(fx["stat_loss_cross"]), "self_similarity_weight = 0")
    spec = t["spectral"].reshape(-1, t["spectral"].shape[2])
    from frl_hip.losses import phase_alignment
    _, ri, rj, lengths = phase_alignment(t["ysfc"], t["pairs"], kw["min_overlap"])
    _, _, gc = SC.gathered_f64(spec, t["phase"].reshape(-1, 12), ri, rj, ri, rj, lengths, False, kw["tau_ref"], kw["tau_learned"],
                               t["weights"][torch.from_numpy(fx["valid_pair_mask"]).to(DEV)], kw["min_valid_per_row"], upstream=kw["cross_pixel_weight"])
    _check_grad(g0, gc.reshape(g0.shape).numpy(), "self_similarity_weight = 0")


@pytest.mark.parametrize("b,m", [(5, 1), (5, 2), (5, 3), (5, 17), (5, 64), (5, 65), (5, 70), (1, 15), (4096, 15)])
def test_matrix_form_shapes_match_the_restatement(b, m):
    d_ref, d_learned = SC.make_distances(b, m, seed=1000 + 7 * b + m)
    lengths = SC.make_lengths(b, 0, m, seed=b + m)
    mask = SC.make_random_mask(b, m, seed=b * m, keep=0.7, lengths=lengths, exclude_diagonal=(m % 2 == 1))
    if b > 1:
        mask[0] = SC.length_mask(torch.tensor([m]), m, True)[0]         # one full pair whatever the draw (all rows skipped when M <= 2)
    w = SC.make_weights(b, seed=m, zero_at=b - 1 if b > 1 else None)
    kw = dict(tau_ref=0.5, tau_learned=0.25, min_valid_per_row=2)
    want_loss, want_stats, want_grad = SC.soft_nbr_f64(d_ref, d_learned, mask, pair_weights=w, upstream=3.0, **kw)
    loss, stats, g = _run_matrix(d_ref, d_learned, mask, factor=3.0, pair_weights=w.to(DEV), **kw)
    _check_loss(loss, want_loss, f"B={b} M={m}")
    _check_stats(stats, want_stats, f"B={b} M={m}")
    _check_grad(g, want_grad, f"B={b} M={m}")
    if m <= 2 and b > 1:
        assert float(loss) == 0.0 and not g.any() and stats["n_rows_valid"] == 0
    if b == 4096:                                                        # the cross-pair reduction: identical bits from run to run
        loss2, _, g2 = _run_matrix(d_ref, d_learned, mask, factor=3.0, pair_weights=w.to(DEV), **kw)
        assert torch.equal(loss, loss2) and torch.equal(g, g2)


@pytest.mark.parametrize("c,d", [(1, 1), (6, 12), (64, 64), (256, 256)])
@pytest.mark.parametrize("m", [2, 3, 16, 32])
def test_gathered_form_shapes_match_the_restatement(m, c, d):
    b, r = 9, 40                                                         # 40 rows shared by 9 * m * 2 positions: repeated rows across pairs
    ref, emb = SC.make_points(1, r, c, seed=m + c)[0], SC.make_points(1, r, d, seed=m + d + 1)[0]
    g = torch.Generator().manual_seed(m * 1000 + c + d)
    rows = [torch.randint(0, r, (b, m), generator=g, dtype=torch.int64) for _ in range(4)]
    rows[2][0] = rows[3][0]                                              # a pair whose two roles are the same rows: zero distances on its diagonal
    lengths = SC.make_lengths(b, 0, m, seed=m + c + d)
    lengths[0], lengths[1], lengths[2] = m, 0, 1                         # a full pair, an empty one, a single position
    w = SC.make_weights(b, seed=c + 3, zero_at=4)
    for excl in (False, True):
        kw = dict(tau_ref=0.5, tau_learned=2.0, min_valid_per_row=2)
        want_loss, want_stats, want_grad = SC.gathered_f64(ref, emb, *rows, lengths, excl, pair_weights=w, upstream=3.0, **kw)
        loss, stats, ge = _run_gathered(ref, emb, *rows, lengths, excl, factor=3.0, pair_weights=w.to(DEV), **kw)
        what = f"M={m} C={c} D={d} excl={excl}"
        _check_loss(loss, want_loss, what)
        _check_stats(stats, want_stats, what)
        assert torch.isfinite(ge).all()
        _check_grad(ge, want_grad.numpy(), what)


def test_degenerate_weights_and_stats_off(golden_dir):
    from frl_hip.losses import soft_neighborhood_loss_gathered, soft_neighborhood_matching_loss
    fx = _fx(golden_dir, "soft_nbr_c")
    d_ref, d_learned = _matrices(fx)
    mask = torch.from_numpy(fx["mask"])
    kw = {k: v for k, v in _kw(fx).items() if k != "pair_weights"}
    loss, stats, g = _run_matrix(d_ref, d_learned, mask, pair_weights=torch.zeros(d_ref.shape[0], device=DEV), **kw)
    assert float(loss) == 0.0 and not g.any() and stats["mean_kl"] == 0.0 and stats["n_pairs_active"] == int(fx["stat_n_pairs_active"])
    one = torch.zeros(d_ref.shape[0])
    one[3] = 0.75                                                        # a single active pair: its own mean KL, whatever the weight
    want_loss, _, want_grad = SC.soft_nbr_f64(d_ref, d_learned, mask, pair_weights=one, **kw)
    loss, _, g = _run_matrix(d_ref, d_learned, mask, pair_weights=one.to(DEV), **kw)
    _check_loss(loss, want_loss, "single active pair")
    _check_grad(g, want_grad, "single active pair")
    assert not g[:3].any() and not g[4:].any()
    # stats=False: an empty dict and the same loss bits, both forms
    w = _kw(fx)["pair_weights"]
    l1, s1 = soft_neighborhood_matching_loss(d_ref.to(DEV), d_learned.to(DEV), mask.to(DEV), pair_weights=w, **kw)
    l0, s0 = soft_neighborhood_matching_loss(d_ref.to(DEV), d_learned.to(DEV), mask.to(DEV), pair_weights=w, stats=False, **kw)
    assert s0 == {} and len(s1) == 8 and torch.equal(l0, l1)
    ref, emb, ra, rb = (x.to(DEV) for x in _point_rows(fx))
    args = (ref, emb, ra, rb, ra, rb, torch.from_numpy(fx["lengths"]).to(DEV), bool(fx["exclude_diagonal"]))
    l1, s1 = soft_neighborhood_loss_gathered(*args, pair_weights=w, **kw)
    l0, s0 = soft_neighborhood_loss_gathered(*args, pair_weights=w, stats=False, **kw)
    assert s0 == {} and len(s1) == 8 and torch.equal(l0, l1)
    zero = torch.zeros(ra.shape[0], device=DEV)
    e = emb.clone().requires_grad_(True)
    lz, _ = soft_neighborhood_loss_gathered(args[0], e, *args[2:], pair_weights=zero, **kw)
    lz.backward()
    assert float(lz) == 0.0 and not e.grad.any()


@pytest.mark.parametrize("case", ["b", "c"])
def test_bfloat16_embeddings(golden_dir, case):
    fx = _fx(golden_dir, f"soft_nbr_{case}")
    ref, emb, ra, rb = _point_rows(fx)
    emb16 = emb.to(torch.bfloat16)
    lengths, excl = torch.from_numpy(fx["lengths"]), bool(fx["exclude_diagonal"])
    want_loss, want_stats, g64 = SC.gathered_f64(ref, emb16, ra, rb, ra, rb, lengths, excl, **_kw(fx, "cpu"))   # on the bf16-rounded values
    loss, stats, g = _run_gathered(ref, emb16, ra, rb, ra, rb, lengths, excl, **_kw(fx))
    assert loss.dtype == torch.float32 and g.dtype == torch.bfloat16
    _check_loss(loss, want_loss, case + " bf16")
    _check_stats(stats, want_stats, case + " bf16")
    g64 = g64.numpy()
    dev = np.abs(g.double().cpu().numpy() - g64)
    bound = 2.0 ** -8 * np.abs(g64) + 1e-5 * np.abs(g64).max()
    print(f"{case} bf16 grad: worst dev / bound {(dev / bound).max():.3f}")
    assert (dev <= bound).all()
