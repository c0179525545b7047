"""tcn_chain_fwd_kernel's side output x_type (the time mean of the tile the kernel holds in registers anyway) against the stand-alone
mean_time pass, and the chain's own outputs with and without it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CH = 12
POISON = -7.0


def _setup(B, HW):
    from frl_hip.models.blocks import Conv2dParams, TCNEncoder
    torch.manual_seed(B * 131 + HW)
    tcn = TCNEncoder(64, [64, 64, 64], 3, [1, 2, 4], 0.0, 8).to(DEV)
    head = Conv2dParams(64, CH, 1).to(DEV)
    with torch.no_grad():
        for l in tcn.layers:
            l.norm.weight.uniform_(0.5, 1.5)
            l.norm.bias.uniform_(-0.3, 0.3)
    g = torch.Generator().manual_seed(HW + 7)
    x = torch.randn(B, 5, HW, 64, generator=g)
    x[0, :, 0, :8] = 0.0                                              # exact zeros, a negative zero and tiny values among the inputs
    x[0, 0, 0, 1] = -0.0
    x[0, :, 1, :] *= 1e-30
    x = x.to(torch.bfloat16).to(DEV)
    blocks = [(l.conv.weight, l.conv.bias, l.norm.weight, l.norm.bias, l.gate.weight, l.gate.bias, l.dilation, 8, False) for l in tcn.layers]
    return x, blocks, head


# (3, 24): 72 pixels -- 16-pixel tiles straddle samples and the last tile is partial; (1, 16): a single full tile
@pytest.mark.parametrize("B,HW", [(2, 64), (3, 24), (1, 16)])
@pytest.mark.parametrize("keep", [True, False])
def test_chain_side_output_equals_mean_time_and_leaves_the_chain_outputs_alone(B, HW, keep):
    from frl_hip import ops
    x, blocks, head = _setup(B, HW)
    assert ops.tcn_chain_supported(x, blocks, head.weight)
    want = ops.mean_time(x)                                           # [B, HW, 64]
    plain = ops.tcn_chain_fwd(x, blocks, head.weight, head.bias, keep_intermediates=keep)
    npix = B * HW
    buf = torch.full((npix + 1, 64), POISON, dtype=torch.bfloat16, device=DEV)     # one guard row behind the last pixel
    got = ops.tcn_chain_fwd(x, blocks, head.weight, head.bias, keep_intermediates=keep, want_xtype=buf)
    torch.cuda.synchronize()
    assert got[4] is buf
    # bit for bit: compare the raw 16-bit patterns (torch.equal would let -0.0 pass for +0.0)
    assert torch.equal(buf[:npix].view(torch.int16), want.reshape(npix, 64).view(torch.int16))
    assert torch.equal(buf[npix].float(), torch.full((64,), POISON, device=DEV)), "a row beyond npix was written"
    for a, b in zip(got[:4], plain):
        if keep or a is not None:
            assert a is not None and b is not None and torch.equal(a.view(torch.int16), b.view(torch.int16))
        else:
            assert a is None and b is None
    # an allocated side output (want_xtype=True) is the same tensor
    xt = ops.tcn_chain_fwd(x, blocks, head.weight, head.bias, keep_intermediates=keep, want_xtype=True)[4]
    assert xt.shape == want.shape and torch.equal(xt.view(torch.int16), want.view(torch.int16))


def test_chain_node_with_side_output_has_the_plain_node_gradients():
    """TcnChainHeadFn(..., True) -> (h, x_type): x_type carries no gradient, h and every gradient equal the plain node's bit for bit."""
    from frl_hip import functional as Fh
    x, blocks, head = _setup(2, 64)
    flat = [t for blk in blocks for t in blk[:6]]
    params = flat + [head.weight, head.bias]
    dh = torch.randn(2, 5, 64, CH, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(DEV)
    res = []
    for side in (False, True):
        for p in params:
            p.grad = None
        xin = x.clone().requires_grad_(True)
        out = Fh.TcnChainHeadFn.apply(xin, *flat, head.weight, head.bias, 8, 1e-5, *([True] if side else []))
        if side:
            out, xt = out
            assert not xt.requires_grad
        out.backward(dh)
        res.append([out.detach(), xin.grad] + [p.grad.clone() for p in params])
    for a, b in zip(*res):
        assert torch.equal(a, b)
