"""Fused decoder backward (csrc/dec_fused.hip) over the latent widths and row counts at which it changes kernel or path.

Widths: Cz <= 16 runs a 16-wide latent block (dz GEMM, dW1 accumulators, w1t image), 17..32 the 32-wide one, > 32 the 64-wide one, whose
8-wave kernel takes the 4-wave workgroup's rounds two at a time and fetches the dxhat -> dhidden fragments from the forward weight image with
transposing reads (its gradients equal the lockstep kernel's bit for bit, which the 1e-4 bound below includes); 12 / 33 / 48 are widths that
are no whole fragment.  Rows: 100 is below the subgroup threshold; 128 is exactly one round per subgroup of one workgroup; 129 leaves the second
workgroup's second subgroup without a round (its slab must come out zero); 200 has a ragged last round; 4133 and 33333 have more rounds than
subgroups, split unevenly.

Every case is checked against float64 autograd of the chain with the hidden activations rounded to bf16 (as test_fused_decoder_mse builds
it, at its tolerances), and the two-subgroup kernels against the lockstep ones: dz bit for bit (it is per row), the weight gradients up to
float32 summation order."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import frl_oracle as O  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
WIDTHS = [12, 16, 17, 32, 33, 48, 64]
ROWS = [100, 128, 129, 200, 4133, 33333]
MASKS = ["none", "random", "zero"]
GVAL = 0.8


def rel_err(got, ref):
    ref = ref.double().cpu()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _lib():
    from frl_hip import _lib
    return _lib.load()


def _inputs(P, cz, mask_kind):
    g = torch.Generator().manual_seed(1000 * cz + P)
    z = torch.randn(P, cz, generator=g).to(BF)
    tgt = torch.randn(P, 64, generator=g).to(BF)
    w1 = torch.randn(128, cz, generator=g) / cz ** 0.5
    b1 = torch.randn(128, generator=g) * 0.1
    w2 = torch.randn(64, 128, generator=g) / 128 ** 0.5
    b2 = torch.randn(64, generator=g) * 0.1
    if mask_kind == "none":
        mask = None
    elif mask_kind == "random":
        mask = torch.rand(P, generator=g) > 0.25
    else:
        mask = torch.zeros(P, dtype=torch.bool)
    return z, w1, b1, w2, b2, tgt, mask


def _float64(z, w1, b1, w2, b2, tgt, mask):
    """loss and d(GVAL * loss) / d(z, w1, b1, w2, b2) in float64, hidden activations rounded to bf16 (test_fused_decoder_mse)."""
    zd = z.double().requires_grad_(True)
    w1q, w2q = w1.to(BF).double().requires_grad_(True), w2.to(BF).double().requires_grad_(True)
    b1d, b2d = b1.double().requires_grad_(True), b2.double().requires_grad_(True)
    hid = torch.relu(zd @ w1q.t() + b1d)
    hid_q = hid.detach().to(BF).double() + (hid - hid.detach())
    xh = hid_q @ w2q.t() + b2d
    P = z.shape[0]
    loss = O.reconstruction_loss_l2(xh, tgt.double(), mask.unsqueeze(1).expand(P, 64) if mask is not None else None)
    leaves = (zd, w1q, b1d, w2q, b2d)
    if loss.requires_grad:
        (GVAL * loss).backward()
        grads = [t.grad for t in leaves]
    else:                                                          # nothing valid: the loss is the constant 0
        grads = [torch.zeros_like(t) for t in leaves]
    return loss.item(), grads


def _dev(z, w1, b1, w2, b2, tgt, mask):
    return tuple(None if t is None else (t.to(torch.uint8) if t.dtype == torch.bool else t).to(DEV) for t in (z, w1, b1, w2, b2, tgt, mask))


@functools.lru_cache(maxsize=None)
def _gscale():
    return torch.full((1,), GVAL, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("P", ROWS)
@pytest.mark.parametrize("cz", WIDTHS)
def test_widths_against_float64_and_lockstep(cz, P, mask_kind):
    from frl_hip import ops
    host = _inputs(P, cz, mask_kind)
    loss_ref, grads_ref = _float64(*host)
    z, w1, b1, w2, b2, tgt, mask = _dev(*host)
    g = _gscale()
    stats, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, mask)
    got = ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, mask, g, stats)
    torch.cuda.synchronize()
    l, nv = stats[0].item(), stats[1].item()
    n_valid = 64 * (P if host[6] is None else int(host[6].sum().item()))
    errs = [rel_err(a.float(), r) for a, r in zip(got, grads_ref)]
    print(f"cz={cz} P={P} mask={mask_kind}: loss {l!r} ref {loss_ref!r}; rel_err dz, dw1, db1, dw2, db2 = " + ", ".join(f"{e:.2e}" for e in errs))
    assert nv == n_valid
    assert abs(l - loss_ref) <= 2e-3 * abs(loss_ref)
    for name, e in zip(("dz", "dw1", "db1", "dw2", "db2"), errs):
        assert e <= 3e-2, name
    lib = _lib()
    was = lib.frl_decoder_mse_bwd_subgroups(0)
    try:
        lock = ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, mask, g, stats)
        torch.cuda.synchronize()
    finally:
        lib.frl_decoder_mse_bwd_subgroups(was)
    assert torch.equal(got[0], lock[0]), "dz depends on who computed the row"
    for name, a, b in zip(("dw1", "db1", "dw2", "db2"), got[1:], lock[1:]):
        e = rel_err(a, b)
        assert e <= 1e-4, (name, e)
    if mask_kind == "zero":
        assert l == 0.0 and nv == 0.0 and not got[0].float().abs().max().item() > 0


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("P", [129, 4133])
@pytest.mark.parametrize("cz", [16, 64])
def test_one_pass_equals_pair(cz, P, mask_kind):
    from frl_hip import ops
    z, w1, b1, w2, b2, tgt, mask = _dev(*_inputs(P, cz, mask_kind))
    g = _gscale()
    stats_ref, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, mask)
    ref = ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, mask, g, stats_ref)
    for rep in range(2):                                           # (the second call finds the control words the first one left)
        stats, dz, slabs = ops.decoder_mse_fwd_bwd(z, w1, b1, w2, b2, tgt, mask, g)
        got = (dz,) + ops.decoder_mse_reduce(slabs, w1, b1, w2, b2)
        torch.cuda.synchronize()
        for name, a, b in zip(("dz", "dw1", "db1", "dw2", "db2"), got, ref):
            assert torch.equal(a, b), f"{name} differs (call {rep})"
        l, lr = stats[0].item(), stats_ref[0].item()
        assert stats[1].item() == stats_ref[1].item()
        assert abs(l - lr) <= 2e-3 * abs(lr)
    assert int(ops._dec_ctl(DEV).abs().sum().item()) == 0


@pytest.mark.parametrize("P", [100, 4133])
@pytest.mark.parametrize("cz", [12, 16])
def test_canary_around_dz_and_unwritten_slab_columns(cz, P):
    """dz sits inside a larger buffer of a sentinel that stays untouched, and the workspace is all NaN before the call: a slab column the
    16-wide kernel no longer writes (>= 16), or a padding column (>= Cz), that reached a gradient would make it non-finite."""
    from frl_hip import ops
    z, w1, b1, w2, b2, tgt, mask = _dev(*_inputs(P, cz, "random"))
    g = _gscale()
    lib = _lib()
    stats, _ = ops.decoder_mse_fwd(z, w1, b1, w2, b2, tgt, mask)
    ref = ops.decoder_mse_bwd(z, w1, b1, w2, b2, tgt, mask, g, stats)
    ws = ops.workspace(lib.frl_decoder_mse_workspace_bytes(P, cz), z.device)
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    pad = 4096
    sentinel = -7.5                                                # exact in bf16
    big = torch.full((pad + P * cz + pad,), sentinel, dtype=BF, device=DEV)
    dz = big[pad:pad + P * cz]
    dw1, db1, dw2, db2 = (torch.empty_like(t) for t in (w1, b1, w2, b2))
    p = ops._p
    ops.check(lib.frl_decoder_mse_bwd(p(z), p(w1), p(b1), p(w2), p(b2), p(tgt), p(mask), p(g), p(stats), p(dz), p(dw1), p(db1), p(dw2), p(db2),
                                      P, cz, p(ws), ws.numel(), ops._stream()), "frl_decoder_mse_bwd")
    torch.cuda.synchronize()
    assert bool((big[:pad] == sentinel).all()) and bool((big[pad + P * cz:] == sentinel).all())
    assert torch.equal(dz.view(P, cz), ref[0])
    for name, a, b in zip(("dw1", "db1", "dw2", "db2"), (dw1, db1, dw2, db2), ref[1:]):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
