"""GPU parity of the fused phase-type leakage loss (csrc/leakage.hip behind losses.phase_type_leakage_loss) against the fixtures of
tests/golden/make_type_phase_golden.py and, where no fixture is committed, against the float64 restatement (tests/type_phase_cases.py,
pinned to the fixtures by tests/test_cpu_type_phase.py).  Bounds: the project's standing ones for this kind of comparison
(tests/test_gpu_vicreg.py): 2e-6 * max(1, |loss64|) on the loss, 1e-5 * max|dh64| on the gradient; with bfloat16 h the expected values
are the restatement's on the bf16-rounded input and, per element, |g - g64| <= 2^-8 |g64| + 1e-5 max|g64|.  Where the loss is exactly
zero the gradient is compared with zero, not with torch's NaN."""
import os

import numpy as np
import pytest
import torch

import type_phase_cases as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(TP.LEAKAGE_CASES)


def _run(h, z, factor=1.0):
    from frl_hip.losses import phase_type_leakage_loss
    hh = h.detach().to(DEV).clone().requires_grad_(True)
    loss = phase_type_leakage_loss(hh, z.to(DEV))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    (factor * loss).backward()
    assert hh.grad.dtype == h.dtype and hh.grad.shape == h.shape
    return loss.detach(), hh.grad


def _check_loss(got, want, what):
    got, want = float(got), float(want)
    print(f"{what}: got {got!r} want {want!r} dev {abs(got - want):.3e} bound {2e-6 * max(1.0, abs(want)):.3e}")
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), what


def _check_grad(g, g64, scale, what):
    g64 = np.asarray(g64, dtype=np.float64)
    dev = np.abs(g.detach().double().cpu().numpy() - g64).max()
    print(f"{what} grad: dev / max {dev / scale:.3e} bound 1e-5")
    assert np.isfinite(dev) and dev <= 1e-5 * scale, what


@pytest.mark.parametrize("name", CASES)
def test_f32_matches_fixture(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, f"leakage_{name}.npz"))
    h, z = TP.leakage_inputs(name)
    loss, g = _run(h, z)
    _check_loss(loss, fx["loss64"], name)
    _check_grad(g[torch.from_numpy(fx["rows"]).to(DEV)], fx["dh64"], float(fx["dh_max"]), name)
    _check_grad(g, TP.leakage_f64(h, z)[1].numpy(), float(fx["dh_max"]), name + " (every row, restatement)")
    loss2, g2 = _run(h, z)                                              # bit-reproducible: identical bits, loss and gradient
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


@pytest.mark.parametrize("factor", [3.0, -0.25])
def test_upstream_factor(golden_dir, factor):
    fx = np.load(os.path.join(golden_dir, "leakage_a.npz"))
    h, z = TP.leakage_inputs("a")
    _, g = _run(h, z, factor)
    _check_grad(g, factor * fx["dh64"], abs(factor) * float(fx["dh_max"]), f"a upstream {factor}")


@pytest.mark.parametrize("n,p,dz,offset", [(100, 64, 128, 0.0), (300, 20, 33, 2.0), (20000, 12, 64, 5.0), (1000, 1, 1, 0.0), (129, 33, 128, 0.0)])
def test_limits_and_odd_shapes_match_the_restatement(n, p, dz, offset):
    """The widest rows (the three register tilings of the moments kernel: P <= 16, <= 32, <= 64), single columns, and more rows than
    256 workgroups take one tile each of."""
    h, z = TP.make_leakage_inputs(n, p, dz, 800 + n + p, offset)
    want, g64 = TP.leakage_f64(h, z)
    assert want >= 0.1
    loss, g = _run(h, z)
    _check_loss(loss, want, f"{n}x{p}x{dz}")
    _check_grad(g, g64.numpy(), float(g64.abs().max()), f"{n}x{p}x{dz}")
    loss2, g2 = _run(h, z)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


@pytest.mark.parametrize("h_dtype,z_dtype", [(torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16)])
@pytest.mark.parametrize("name", ["a", "b"])
def test_bf16_rows(name, h_dtype, z_dtype):
    """Expected values: the restatement in float64 on the ROUNDED inputs, which the kernel reads exactly.  Loss: the f32 bound.  Gradient
    in bfloat16, elementwise: |g - g64| <= 2^-8 |g64| + 1e-5 max|g64| (one bf16 rounding of the output + the f32 bound)."""
    h, z = TP.leakage_inputs(name)
    hb, zb = h.to(h_dtype), z.to(z_dtype)
    want, g64 = TP.leakage_f64(hb, zb)
    loss, g = _run(hb, zb)
    assert g.dtype == h_dtype
    _check_loss(loss, want, f"{name} {h_dtype} {z_dtype}")
    g64 = g64.numpy()
    if h_dtype == torch.float32:
        _check_grad(g, g64, np.abs(g64).max(), f"{name} f32 h, bf16 z")
        return
    err = np.abs(g.double().cpu().numpy() - g64)
    bound = 2.0 ** -8 * np.abs(g64) + 1e-5 * np.abs(g64).max()
    print(f"{name} {h_dtype} {z_dtype} grad: worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


def test_zero_loss_gives_zero_gradient_not_nan():
    """N = 1, h constant in every column, z constant in every column: the loss is exactly zero and so is the gradient (the reference's
    autograd returns NaN: the derivative of sqrt at 0)."""
    h, z = TP.leakage_inputs("a")
    for what, hh, zz in (("N = 1", h[:1], z[:1]), ("constant h", torch.full_like(h, 37.123), z), ("constant z", h, torch.full_like(z, -0.3)),
                         ("constant h, 1031 rows", torch.full((1031, 12), 37.123), TP.leakage_inputs("b")[1])):
        loss, g = _run(hh, zz)
        print(f"{what}: loss {float(loss)!r} max|dh| {float(g.abs().max())!r}")
        assert float(loss) == 0.0 and not bool(g.any()) and bool(torch.isfinite(g).all()), what


def test_one_constant_column_gets_exactly_no_gradient():
    h, z = TP.leakage_inputs("b")
    h = h.clone()
    h[:, 3] = 37.123
    want, g64 = TP.leakage_f64(h, z)
    loss, g = _run(h, z)
    _check_loss(loss, want, "one constant column")
    _check_grad(g, g64.numpy(), float(g64.abs().max()), "one constant column")
    assert not bool(g[:, 3].any())


def test_h_without_grad_launches_no_backward_and_z_receives_none():
    from frl_hip import ops
    from frl_hip.losses import phase_type_leakage_loss
    h, z = TP.leakage_inputs("a")
    zz = z.to(DEV).requires_grad_(True)
    ops.set_timing(True)
    try:
        loss = phase_type_leakage_loss(h.to(DEV), zz)
        assert not loss.requires_grad and loss.grad_fn is None
        hh = h.to(DEV).requires_grad_(True)
        loss2 = phase_type_leakage_loss(hh, zz)
        summary = dict(ops.timing_summary() or {})
        assert summary["leakage_fwd"][0] == 2 and "leakage_bwd" not in summary
        (loss2 + 0.0 * zz.sum()).backward()
        assert dict(ops.timing_summary())["leakage_bwd"][0] == 1
    finally:
        ops.set_timing(False)
    assert torch.equal(loss, loss2.detach())
    assert hh.grad is not None and not bool(zz.grad.any())              # z_type is detached inside: nothing flows to it


def test_graph_capture_replays_on_new_inputs():
    """Forward and backward captured once (the upstream factor is read on the device), replayed twice on other values."""
    from frl_hip.losses import phase_type_leakage_loss
    ha, za = TP.leakage_inputs("b")
    hb, zb = TP.make_leakage_inputs(1031, 12, 64, 911, 3.0)
    h_in = ha.to(DEV).clone().requires_grad_(True)
    z_in, f_in = za.to(DEV).clone(), torch.ones((), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                       # warm-up off the default stream, as torch asks before a capture
        (f_in * phase_type_leakage_loss(h_in, z_in)).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    h_in.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = phase_type_leakage_loss(h_in, z_in)
        (f_in * loss).backward()
    g_out = h_in.grad
    for h, z, factor in ((hb, zb, 2.0), (ha, za, 1.0)):
        with torch.no_grad():
            h_in.copy_(h)
            z_in.copy_(z)
            f_in.fill_(factor)
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_g = _run(h, z, factor)
        assert torch.equal(loss.detach(), want_loss) and torch.equal(g_out, want_g)
