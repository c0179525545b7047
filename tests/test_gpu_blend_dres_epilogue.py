"""The gate blend's d(residual) = dout * gate formed in the epilogue of the backward-data convolution that consumes it (conv3x3
epi_mode 4) against the two-step form gate_blend_bwd -> conv3x3_bwd_data(add=, sub_from=): same bits, in the kernel pair and through
SpatialSmoothFn."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _rnd(shape, seed, dtype, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,H,W", [(1, 8, 8), (1, 9, 13), (2, 32, 32)])
def test_epilogue_forms_dres_with_the_bits_of_the_two_step_form(dtype, B, H, W):
    from frl_hip import ops
    C = 64
    dg1 = _rnd((B, H, W, C), 1, dtype)
    w = _rnd((C, C, 3, 3), 2, torch.float32, 0.05)
    dout, res = _rnd((B, H, W, C), 3, dtype), _rnd((B, H, W, C), 4, dtype)
    gate = torch.sigmoid(_rnd((B, H, W, C), 5, torch.float32)).to(dtype)
    dout[:, :, ::3] = 0.0                                    # signed-zero products and sums
    dout[:, ::2, 1::3] = -dout[:, ::2, 1::3].abs()
    dres, dgraw = ops.gate_blend_bwd(dout, None, res, gate, 0.0, sigmoid_mask=True)
    want = ops.conv3x3_bwd_data(dg1, w, None, ops.ACT_NONE, add=dres, sub_from=dout)
    none, dgraw2 = ops.gate_blend_bwd(dout, None, res, gate, 0.0, sigmoid_mask=True, want_dres=False)
    got = ops.conv3x3_bwd_data(dg1, w, None, ops.ACT_NONE, gate=gate, sub_from=dout)
    assert none is None and torch.equal(_bits(dgraw), _bits(dgraw2))
    assert torch.equal(_bits(got[0]), _bits(want[0])), "dres_tot"
    assert torch.equal(_bits(got[1]), _bits(want[1])), "d_tot"


def test_gate_needs_sub_from_and_excludes_add():
    from frl_hip import ops
    t = _rnd((1, 8, 8, 64), 1, torch.bfloat16)
    w = _rnd((64, 64, 3, 3), 2, torch.float32, 0.05)
    with pytest.raises(ValueError):
        ops.conv3x3_bwd_data(t, w, gate=t)
    with pytest.raises(ValueError):
        ops.conv3x3_bwd_data(t, w, gate=t, sub_from=t, add=t)


@pytest.mark.parametrize("with_dgate,min_gate", [(False, 0.0), (True, 0.0), (True, 0.1)])
def test_spatial_smooth_fn_same_gradients_with_the_fold_on_and_off(monkeypatch, with_dgate, min_gate):
    """(2, 32, 32, 64), hidden 64, bf16: dx and the ten parameter gradients bit-equal with FRL_HIP_DISABLE=dres and without; with a gate
    floor both runs take the two-step path."""
    from frl_hip import ops
    from frl_hip.models.blocks import EdgeAwareSmoothingConv2D
    torch.manual_seed(7)
    m = EdgeAwareSmoothingConv2D(64, gate_hidden=64).to(DEV)
    m.set_min_gate(min_gate)
    x0 = _rnd((2, 32, 32, 64), 9, torch.bfloat16, 0.7)
    dout = _rnd((2, 32, 32, 64), 10, torch.bfloat16)
    dgate = _rnd((2, 32, 32, 64), 11, torch.bfloat16, 0.3)
    seen = []
    real = ops.conv3x3_bwd_data

    def spy(*a, **k):
        seen.append(k.get("gate") is not None)
        return real(*a, **k)

    monkeypatch.setattr(ops, "conv3x3_bwd_data", spy)

    def run(disable):
        if disable:
            monkeypatch.setenv("FRL_HIP_DISABLE", "dres")
        else:
            monkeypatch.delenv("FRL_HIP_DISABLE", raising=False)
        del seen[:]
        m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        out, gate = m(x, return_gate=True)
        if with_dgate:
            torch.autograd.backward([out, gate], [dout, dgate])
        else:
            out.backward(dout)
        return x.grad.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}, any(seen)

    dx_on, g_on, folded_on = run(False)
    dx_off, g_off, folded_off = run(True)
    assert folded_on == (min_gate <= 0.0) and not folded_off
    assert len(g_on) == 10
    assert torch.equal(_bits(dx_on), _bits(dx_off))
    for n in g_on:
        assert torch.equal(g_on[n].view(torch.int32) if g_on[n].dtype == torch.float32 else _bits(g_on[n]),
                           g_off[n].view(torch.int32) if g_off[n].dtype == torch.float32 else _bits(g_off[n])), n
