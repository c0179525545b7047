"""GPU parity of the fused VICReg variance-covariance loss (csrc/vicreg.hip) against the fixtures written by the REFERENCE's function
(tests/golden/make_vicreg_golden.py) and, for shapes too large to commit, against the float64 restatement (tests/vicreg_cases.py); and
of the VQ-VAE's lambda_vcr term.  Bounds: those of the InfoNCE parity test for the same kind of comparison
(tests/test_gpu_contrastive.py): 2e-6 * max(1, |loss|) on losses, 1e-5 * max|grad64| on gradients."""
import os

import numpy as np
import pytest
import torch

from vicreg_cases import make_rows, vicreg_f64, vicreg_torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fx(golden_dir, case):
    return np.load(os.path.join(golden_dir, f"vicreg_{case}.npz"))


def _kw(fx):
    return dict(variance_weight=float(fx["variance_weight"]), covariance_weight=float(fx["covariance_weight"]),
                variance_target=float(fx["variance_target"]), eps=float(fx["eps"]))


def _check_losses(out, want, what):
    for name, o, w in zip(("total", "variance", "covariance"), out, want):
        got = float(o.detach())
        print(f"{what} {name}: got {got!r} want {float(w)!r} dev {abs(got - float(w)):.3e} bound {2e-6 * max(1.0, abs(float(w))):.3e}")
    for o, w in zip(out, want):
        assert abs(float(o.detach()) - float(w)) <= 2e-6 * max(1.0, abs(float(w))), what


def _check_grad(g, g64, what):
    g64 = np.asarray(g64, dtype=np.float64)
    scale = max(1e-6, np.abs(g64).max())
    dev = np.abs(g.detach().double().cpu().numpy() - g64).max()
    print(f"{what} grad: dev / max {dev / scale:.3e} bound 1e-5")
    assert dev <= 1e-5 * scale, what


def _run(x, kw, upstream=(1.0, 0.0, 0.0)):
    from frl_hip.losses import variance_covariance_loss
    x = x.detach().clone().requires_grad_(True)
    out = variance_covariance_loss(x, **kw)
    (upstream[0] * out[0] + upstream[1] * out[1] + upstream[2] * out[2]).backward()
    return out, x.grad


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_f32_matches_reference_fixture(golden_dir, case):
    fx = _fx(golden_dir, case)
    x = torch.from_numpy(fx["x"]).to(DEV)
    out, g = _run(x, _kw(fx))
    assert all(o.dtype == torch.float32 and o.dim() == 0 for o in out) and g.dtype == torch.float32
    _check_losses(out, fx["loss64"], case)
    _check_grad(g, fx["grad64"], case)
    out2, g2 = _run(x, _kw(fx))                                          # bit-reproducible: identical bits, loss and gradient
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and torch.equal(g, g2)


@pytest.mark.parametrize("upstream", [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (3.0, 0.0, 0.0), (0.5, -2.0, 0.25)])
def test_gradients_of_each_output_and_upstream_factor(golden_dir, upstream):
    fx = _fx(golden_dir, "b")
    x = torch.from_numpy(fx["x"]).to(DEV)
    _, g = _run(x, _kw(fx), upstream)
    _, g64 = vicreg_f64(x, **_kw(fx), upstream=upstream)
    _check_grad(g, g64, f"b upstream {upstream}")
    if upstream == (3.0, 0.0, 0.0):
        _check_grad(g, 3.0 * fx["grad64"], "b (3 total).backward() vs fixture")


def test_variance_and_covariance_helpers(golden_dir):
    from frl_hip.losses import covariance_loss, variance_loss
    fx = _fx(golden_dir, "b")
    x = torch.from_numpy(fx["x"]).to(DEV)
    for fn, idx, up in ((variance_loss, 1, (0.0, 1.0, 0.0)), (covariance_loss, 2, (0.0, 0.0, 1.0))):
        xx = x.clone().requires_grad_(True)
        l = fn(xx)
        l.backward()
        assert abs(float(l.detach()) - float(fx["loss64"][idx])) <= 2e-6 * max(1.0, abs(float(fx["loss64"][idx])))
        _check_grad(xx.grad, vicreg_f64(x, 1.0, 1.0, 1.0, 1e-4, upstream=up)[1], fn.__name__)


@pytest.mark.parametrize("n,d,offset", [(262144, 64, 3.0), (65536, 12, 0.0), (1000, 40, 0.0), (777, 7, 1.0)])
def test_large_and_odd_shapes_match_the_float64_restatement(n, d, offset):
    x = make_rows(n, d, seed=n + d, offset=offset)
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.5, eps=1e-4)
    want, g64 = vicreg_f64(x, **kw)
    out, g = _run(x.to(DEV), kw)
    _check_losses(out, want, f"{n}x{d}")
    _check_grad(g, g64, f"{n}x{d}")
    out2, g2 = _run(x.to(DEV), kw)
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and torch.equal(g, g2)


@pytest.mark.parametrize("n,d,offset", [(4096, 64, 0.5), (8192, 12, 0.0), (3000, 128, 2.0)])
def test_bf16_rows(n, d, offset):
    """Expected values: the restatement in float64 on the bf16-ROUNDED input, which the kernel reads exactly.  Losses: the f32 bound.
    Gradient, elementwise: |g - g64| <= 2^-8 |g64| + 1e-5 max|g64| (one bf16 rounding of the output + the f32 bound)."""
    xb = make_rows(n, d, seed=7 * n + d, offset=offset).to(torch.bfloat16)
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.5, eps=1e-4)
    want, g64 = vicreg_f64(xb, **kw)
    out, g = _run(xb.to(DEV), kw)
    assert g.dtype == torch.bfloat16 and all(o.dtype == torch.float32 for o in out)
    _check_losses(out, want, f"bf16 {n}x{d}")
    g64 = g64.numpy()
    err = np.abs(g.double().cpu().numpy() - g64)
    bound = 2.0 ** -8 * np.abs(g64) + 1e-5 * np.abs(g64).max()
    print(f"bf16 {n}x{d} grad: worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    out2, g2 = _run(xb.to(DEV), kw)
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and torch.equal(g, g2)


def test_outlying_first_row_does_not_bring_the_cancellation_back():
    """Row 0 sits 200 (about 150 std) from the rest, as a masked or constant-input pixel at (0, 0) of the first tile may: a pivot taken
    from that row alone would put (|mu - p| / std)^2 ~ 2e4 in front of the f32 rounding of G - S S^T / N.  Same bounds as everywhere."""
    x = make_rows(65536, 64, seed=11, offset=0.5)
    x[0] = 200.0
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.5, eps=1e-4)
    want, g64 = vicreg_f64(x, **kw)
    out, g = _run(x.to(DEV), kw)
    _check_losses(out, want, "outlying row 0")
    _check_grad(g, g64, "outlying row 0")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_at_an_odd_storage_offset(dtype):
    """A contiguous view that starts 2 elements into its buffer: row starts are not 16-byte aligned, the kernels must not use their
    vector accesses.  Same values in the same order as the aligned copy: identical bits."""
    n, d = 1000, 64
    x = make_rows(n, d, seed=5, offset=0.25).to(dtype)
    buf = torch.zeros(n * d + 2, dtype=dtype, device=DEV)
    view = buf[2:].view(n, d)
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.5, eps=1e-4)
    out_v, g_v = _run(view, kw)
    out_a, g_a = _run(x.to(DEV), kw)
    _check_losses(out_v, vicreg_f64(x, **kw)[0], f"offset view {dtype}")
    assert all(torch.equal(a, b) for a, b in zip(out_v, out_a)) and torch.equal(g_v, g_a)


def test_constant_columns_far_from_the_pivot_stay_finite():
    """Near-constant columns: rounding may leave a variance just below zero; the square roots clamp it."""
    x = torch.full((5000, 16), 37.123, dtype=torch.float32)
    x[:, 8:] += 1e-3 * torch.randn(5000, 8, generator=torch.Generator().manual_seed(3))
    out, g = _run(x.to(DEV), dict(variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=0.0 + 1e-12))
    assert all(bool(torch.isfinite(o)) for o in out) and bool(torch.isfinite(g).all())


def test_single_row_returns_zeros_without_a_launch():
    from frl_hip import ops
    from frl_hip.losses import variance_covariance_loss
    x = torch.randn(1, 16, device=DEV, requires_grad=True)
    ops.set_timing(True)
    try:
        out = variance_covariance_loss(x)
        assert "vicreg_fwd" not in dict(ops.timing_summary() or {})
    finally:
        ops.set_timing(False)
    assert len(out) == 3 and all(float(o) == 0.0 for o in out)
    if out[0].requires_grad:
        out[0].backward()
    assert x.grad is None or float(x.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# the VQ-VAE term (tiny f32 model: the configuration of the vqvae_tiny_seed0 fixture)
# ---------------------------------------------------------------------------------------------------------------------------------
VCR = dict(lambda_vcr=0.5, vcr_variance_weight=25.0, vcr_covariance_weight=1.0, vcr_variance_target=1.0)


def _state(fx):
    return {k[6:]: torch.from_numpy(fx[k]).float() for k in fx.files if k.startswith("state.")}


def _model(fx, **extra):
    from frl_hip.models import VQVAE
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, beta=0.25, hidden=16, z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4, compute_dtype=torch.float32, **extra).to(DEV)
    m.load_state_dict(_state(fx), strict=True)
    return m.train()


def _tiny(golden_dir):
    fx = np.load(os.path.join(golden_dir, "vqvae_tiny_seed0.npz"))
    return fx, torch.from_numpy(fx["tiles"]).float().to(DEV)


def test_vqvae_term_adds_the_weighted_totals(golden_dir):
    fx, tiles = _tiny(golden_dir)
    out1 = _model(fx, **VCR).forward_tiles(tiles[0])
    out0 = _model(fx).forward_tiles(tiles[0])
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.0)
    tt = vicreg_f64(out1["z_type"].reshape(-1, 8), **kw)[0][0]
    tp = vicreg_f64(out1["z_phase"].reshape(-1, 4), **kw)[0][0]
    diff = float(out1["loss"].detach()) - float(out0["loss"].detach())
    print(f"loss {float(out1['loss'].detach())!r} - {float(out0['loss'].detach())!r} = {diff!r}; 0.5 (type {tt!r} + phase {tp!r}) = {0.5 * (tt + tp)!r}")
    assert abs(diff - 0.5 * (tt + tp)) <= 2e-6 * max(1.0, abs(float(out1["loss"].detach())))
    assert abs(float(out1["vcr_loss"]) - tt) <= 2e-6 * max(1.0, abs(tt)) and abs(float(out1["vcr_loss_phase"]) - tp) <= 2e-6 * max(1.0, abs(tp))
    assert not out1["vcr_loss"].requires_grad
    m = _model(fx, **VCR).eval()                                          # the regulariser is a training term
    assert "vcr_loss" not in m.forward_tiles(tiles[0])


def test_vqvae_term_gradient_is_the_vicreg_gradient_through_the_encoder(golden_dir):
    fx, tiles = _tiny(golden_dir)
    m1, m0 = _model(fx, **VCR), _model(fx)
    m1.forward_tiles(tiles[0])["loss"].backward()
    out0 = m0.forward_tiles(tiles[0])
    kw = dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.0)
    extra = 0.5 * (vicreg_torch(out0["z_type"].reshape(-1, 8), **kw) + vicreg_torch(out0["z_phase"].reshape(-1, 4), **kw))
    (out0["loss"] + extra).backward()
    changed = 0
    for (n, p), (_, q) in zip(m1.named_parameters(), m0.named_parameters()):
        ref = q.grad.double().cpu().numpy()
        dev = np.abs(p.grad.double().cpu().numpy() - ref).max()
        assert dev <= 1e-6 + 2e-4 * np.abs(ref).max(), (n, dev)          # the f32 tolerance of test_vqvae_step_matches_oracle_fixture
        changed += int(np.abs(ref - fx["grad." + n]).max() > 1e-4 * max(np.abs(ref).max(), 1e-12))
    assert changed > 0                                                    # the term does reach the encoder's gradients


def test_lambda_zero_is_the_parent_model_bit_for_bit(golden_dir):
    fx, tiles = _tiny(golden_dir)
    ma, mb = _model(fx, lambda_vcr=0.0), _model(fx)
    oa, ob = ma.forward_tiles(tiles[0]), mb.forward_tiles(tiles[0])
    assert "vcr_loss" not in oa and "vcr_loss_phase" not in oa and set(oa) == set(ob)
    assert torch.equal(oa["loss"], ob["loss"])
    oa["loss"].backward()
    ob["loss"].backward()
    for (n, p), (_, q) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_graph_captured_step_with_the_term_equals_eager(golden_dir):
    from frl_hip.training.trainer import VQVAETrainer
    fx, tiles = _tiny(golden_dir)
    seq = [tiles[i].contiguous() for i in range(3)]

    def run(graphed):
        m = _model(fx, **VCR)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=8)
        losses = []
        for t in seq:
            out = tr.step_graphed(t) if graphed else tr.step(t)
            assert "vcr_loss" in out and "vcr_loss_phase" in out
            losses.append(float(out["loss"].detach()))
        torch.cuda.synchronize()
        return m, tr, losses

    m0, _, l0 = run(False)
    m1, tr1, l1 = run(True)
    assert tr1.graph_supported() and l0 == l1
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), n


def test_frozen_encoder_with_the_term_runs_and_gets_no_gradient(golden_dir):
    fx, tiles = _tiny(golden_dir)
    m = _model(fx, **VCR)
    frozen = [n for n, _ in m.named_parameters() if not n.startswith(("decoder_", "quant"))]
    assert frozen
    for n, p in m.named_parameters():
        p.requires_grad_(n not in frozen)
    out = m.forward_tiles(tiles[0])
    out["loss"].backward()
    assert "vcr_loss" in out and np.isfinite(float(out["loss"].detach()))
    for n, p in m.named_parameters():
        assert (p.grad is None) == (n in frozen), n
