"""One-pass decoder loss + gradients (frl_decoder_mse_fwd_bwd / frl_decoder_mse_reduce) against the unchanged pair
frl_decoder_mse_fwd + frl_decoder_mse_bwd on the same inputs: gradients bit for bit, the loss within the tolerance of the decoder test
against the float64 oracle (tests/test_gpu_kernels_blocks.py: 2e-3 relative), the promise guard, and which path a call takes.

Loss: the one-pass kernel forms diff as the forward kernel does and sums it in double per wave and workgroup, but its rows are
distributed over lanes and workgroups differently (64- / 128-row tiles over <= 256 workgroups instead of 16-row tiles over <= 1024), so the
float32 per-lane sums see the rows in another order: the loss is not expected to be bit-equal in general; each case prints what it got
(MI355X: bit-equal in all 72 comparisons of the first test)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_RTOL = 2e-3          # test_fused_decoder_mse's bound on the loss


def _inputs(P, cz, mask_kind, seed=0):
    g = torch.Generator().manual_seed(1000 * cz + P + seed)
    bf = torch.bfloat16
    z = torch.randn(P, cz, generator=g).to(bf).to(DEV)
    tgt = torch.randn(P, 64, generator=g).to(bf).to(DEV)
    w1 = (torch.randn(128, cz, generator=g) / cz ** 0.5).to(DEV)
    b1 = (torch.randn(128, generator=g) * 0.1).to(DEV)
    w2 = (torch.randn(64, 128, generator=g) / 128 ** 0.5).to(DEV)
    b2 = (torch.randn(64, generator=g) * 0.1).to(DEV)
    if mask_kind == "none":
        mask = None
    elif mask_kind == "random":
        mask = (torch.rand(P, generator=g) > 0.25).to(torch.uint8).to(DEV)
    else:
        mask = torch.zeros(P, dtype=torch.uint8, device=DEV)
    return z, w1, b1, w2, b2, tgt, mask


# (P, Cz) -> kernel: two-subgroup <1,4,true> (Cz <= 32, P >= 128; 70001 rows: uneven split, ragged last round), 8-wave <1,8> (P < 128),
# 4-wave <2,4> (Cz > 32)
SHAPES = [(70001, 12), (4096, 12), (100, 12), (4096, 64), (130, 64), (33333, 64)]


@pytest.mark.parametrize("gval", [1.0, 0.25])
@pytest.mark.parametrize("mask_kind", ["none", "random", "zero"])
@pytest.mark.parametrize("P,cz", SHAPES)
def test_onepass_equals_forward_backward_pair(P, cz, mask_kind, gval):
    from frl_hip import ops
    z, w1, b1, w2, b2, tgt, mask = _inputs(P, cz, mask_kind)
    g = torch.full((1,), gval, dtype=torch.float32, device=DEV)
    stats_ref, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, mask)
    ref = ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, mask, g, stats_ref)
    for rep in range(2):                                           # (the second call finds the control words the first one left)
        stats, dz, slabs = ops.decoder_mse_fwd_bwd(z, w1, b1, w2, b2, tgt, mask, g)
        got = (dz,) + ops.decoder_mse_reduce(slabs, w1, b1, w2, b2)
        torch.cuda.synchronize()
        for name, a, b in zip(("dz", "dw1", "db1", "dw2", "db2"), got, ref):
            assert torch.equal(a, b), f"{name} differs (call {rep})"
        l, lr = stats[0].item(), stats_ref[0].item()
        print(f"P={P} cz={cz} mask={mask_kind} g={gval}: loss {l!r} pair {lr!r} bit-equal={l == lr} rel={abs(l - lr) / max(abs(lr), 1e-30):.3e}")
        assert stats[1].item() == stats_ref[1].item()
        assert abs(l - lr) <= LOSS_RTOL * abs(lr)
        if mask_kind == "zero":
            assert l == 0.0 and stats[1].item() == 0.0 and not dz.float().abs().max().item() > 0
    assert int(ops._dec_ctl(DEV).abs().sum().item()) == 0          # control words are left zero


def test_onepass_mask_at_an_odd_address():
    """The mask count reads 16 bytes at a time only from an aligned mask; a view at an odd offset takes the byte loop."""
    from frl_hip import ops
    z, w1, b1, w2, b2, tgt, _ = _inputs(5001, 12, "none")
    base = (torch.rand(5002, generator=torch.Generator().manual_seed(3)) > 0.3).to(torch.uint8).to(DEV)
    mask = base[1:]
    g = torch.ones(1, dtype=torch.float32, device=DEV)
    stats_ref, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, mask)
    stats, _, _ = ops.decoder_mse_fwd_bwd(z, w1, b1, w2, b2, tgt, mask, g)
    assert stats[1].item() == stats_ref[1].item() == 64.0 * int(mask.sum().item())


def _leaves(P, cz, mask_kind, frozen, z_grad):
    z, w1, b1, w2, b2, tgt, mask = _inputs(P, cz, mask_kind, seed=7)
    z = z.requires_grad_(z_grad)
    ps = dict(w1=w1, b1=b1, w2=w2, b2=b2)
    for n, p in ps.items():
        p.requires_grad_(n not in frozen)
    return z, ps, tgt, mask


@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("case", ["all", "frozen-w1", "frozen-decoder", "z-no-grad"])
@pytest.mark.parametrize("P,cz,mask_kind", [(4096, 12, "random"), (4096, 64, "none")])
def test_onepass_autograd_equals_two_kernel_path(P, cz, mask_kind, case, deferred):
    from frl_hip import functional as Fh, ops
    frozen = {"frozen-w1": ("w1",), "frozen-decoder": ("w1", "b1", "w2", "b2")}.get(case, ())
    s = 0.5
    sdev = torch.full((1,), s, dtype=torch.float32, device=DEV)
    res = []
    ops.grad_scale_errors()
    for gs in (None, sdev):
        z, ps, tgt, mask = _leaves(P, cz, mask_kind, frozen, case != "z-no-grad")
        ops.set_timing(True)
        try:
            l, _ = Fh.decoder_mse(z, ps["w1"], ps["b1"], ps["w2"], ps["b2"], tgt, mask, grad_scale=gs)
            loss = Fh.scalar_combine([l], [s])[0]
            params = [p for p in ps.values() if p.requires_grad]
            if deferred:
                with ops.deferred_reductions(params):               # (its destination check runs at the block's end)
                    loss.backward()
            else:
                loss.backward()
            keys = set(ops.timing_summary())
        finally:
            ops.set_timing(False)
        assert ("decoder_mse_fwd_bwd" in keys) == (gs is not None) and ("decoder_mse_fwd" in keys) == (gs is None)
        res.append((l.item(), z.grad, {n: p.grad for n, p in ps.items()}))
    (l0, dz0, g0), (l1, dz1, g1) = res
    assert abs(l1 - l0) <= LOSS_RTOL * abs(l0)
    assert (dz0 is None) == (dz1 is None) and (dz0 is None or torch.equal(dz0, dz1))
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None) == (n in frozen), n
        assert g0[n] is None or torch.equal(g0[n], g1[n]), n
    assert not ops.grad_scale_errors()


@pytest.mark.parametrize("route", ["scalar_combine", "plain"])
def test_broken_promise_is_flagged_and_cleared(route):
    """A backward that hands the loss another gradient than it was computed for raises at the poll; the flag is cleared by the read."""
    from frl_hip import functional as Fh, ops
    ops.grad_scale_errors()
    one = torch.ones(1, dtype=torch.float32, device=DEV)

    def run(coef):
        z, ps, tgt, mask = _leaves(1000, 12, "random", (), True)
        l, _ = Fh.decoder_mse(z, ps["w1"], ps["b1"], ps["w2"], ps["b2"], tgt, mask, grad_scale=one)
        (Fh.scalar_combine([l], [coef])[0] if route == "scalar_combine" else l * coef).backward()

    run(1.0)
    assert not ops.grad_scale_errors()
    ops.check_grad_scale()
    run(3.0)
    with pytest.raises(RuntimeError, match="grad_scale"):
        ops.check_grad_scale()
    assert not ops.grad_scale_errors()                             # cleared by the read


def test_onepass_is_not_taken_without_a_train_backward():
    """no_grad, want_xhat and inputs without gradients keep the forward kernel; so do eval() and return_recon at the model level."""
    from frl_hip import functional as Fh, ops
    from frl_hip.models import VQVAE
    one = torch.ones(1, dtype=torch.float32, device=DEV)

    def keys_of(fn):
        ops.set_timing(True)
        try:
            fn()
            return set(ops.timing_summary())
        finally:
            ops.set_timing(False)

    z, ps, tgt, mask = _leaves(1000, 12, "random", (), True)
    call = lambda **kw: Fh.decoder_mse(z, ps["w1"], ps["b1"], ps["w2"], ps["b2"], tgt, mask, grad_scale=one, **kw)

    def under_no_grad():
        with torch.no_grad():
            call()

    for fn in (under_no_grad, lambda: call(want_xhat=True)):
        keys = keys_of(fn)
        assert "decoder_mse_fwd" in keys and "decoder_mse_fwd_bwd" not in keys
    assert "decoder_mse_fwd_bwd" in keys_of(call)

    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    tile = torch.randn(2, 3, 16, 16, 64, device=DEV)
    m.train()
    keys = keys_of(lambda: m.forward_tiles(tile)["loss"].backward())
    assert "decoder_mse_fwd_bwd" in keys and "decoder_mse_fwd" not in keys and "decoder_mse_bwd" not in keys
    keys = keys_of(lambda: m.forward_tiles(tile, return_recon=True)["loss"].backward())
    assert "decoder_mse_fwd_bwd" not in keys and "decoder_mse_fwd" in keys
    m.onepass_decoder = False
    keys = keys_of(lambda: m.forward_tiles(tile)["loss"].backward())
    assert "decoder_mse_fwd_bwd" not in keys and "decoder_mse_bwd" in keys
    m.onepass_decoder = True
    m.eval()
    keys = keys_of(lambda: m.forward_tiles(tile))
    assert "decoder_mse_fwd_bwd" not in keys and "decoder_mse_fwd" in keys
    assert not ops.grad_scale_errors()


def test_train_step_onepass_equals_two_kernel_step():
    """forward_tiles + backward in train mode: every parameter gradient bit-equal with and without the one-pass decoders."""
    from frl_hip import ops
    from frl_hip.models import VQVAE
    torch.manual_seed(1)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    m.train()
    tile = torch.randn(2, 3, 16, 16, 64, device=DEV)
    grads = []
    for on in (False, True):
        m.onepass_decoder = on
        m.zero_grad(set_to_none=True)
        out = m.forward_tiles(tile)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads.append((out["loss"].item(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = grads
    assert abs(l1 - l0) <= LOSS_RTOL * abs(l0)
    assert g0.keys() == g1.keys()
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
    assert not ops.grad_scale_errors()
