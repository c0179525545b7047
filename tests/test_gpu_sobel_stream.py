"""Row-band streaming Sobel kernels (csrc/stencil.hip) against the gather kernels they replace on the hot shapes: same bits, signed
zeros included, on every band layout; both against float64 F.conv2d at test_sobel's tolerances."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = {torch.float32: 3e-6, torch.bfloat16: 3e-2}      # test_gpu_kernels_blocks.MODES: relative to max|ref|, backward 2 x


@pytest.fixture()
def routes():
    """-> run(fn, stream): fn() with the streaming route on / forced off; the process switch is restored afterwards."""
    from frl_hip import ops
    was = ops.sobel_stream(True)

    def run(fn, stream):
        ops.sobel_stream(stream)
        try:
            return fn()
        finally:
            ops.sobel_stream(True)

    yield run
    ops.sobel_stream(was)


def _band():
    from frl_hip import ops
    return ops.sobel_stream_band()


def _inputs(shape, seed, dtype=torch.bfloat16):
    """randn with a block of exact zeros and a block that negates its left neighbour block: sums of +0 and -0 terms, and exact
    cancellations to a signed zero, occur in the chains."""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    c = shape[-1]
    t[..., : c // 4] = 0.0
    t[..., c // 4: c // 2] = -t[..., c // 2: c // 2 + c // 4]
    t[:, :, 1::5] = 0.0                                      # whole columns of zeros: chains made of zero terms only
    if shape[1] > 1:
        t[:, 1::3] = -t[:, 0::3][:, : t[:, 1::3].shape[1]]   # rows that negate the row above: vertical taps cancel exactly
    return t.to(DEV)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _ref64(x, dg):
    """float64 F.conv2d Sobel pair and its input gradient, NHWC in and out (test_sobel's reference)."""
    c = x.shape[-1]
    xr = x.double().cpu().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    sx = (torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]]) / 4).double().reshape(1, 1, 3, 3).expand(c, 1, 3, 3)
    sy = (torch.tensor([[-1., -2., -1.], [0., 0., 0.], [1., 2., 1.]]) / 4).double().reshape(1, 1, 3, 3).expand(c, 1, 3, 3)
    ref = torch.cat([F.conv2d(xr, sx, padding=1, groups=c), F.conv2d(xr, sy, padding=1, groups=c)], 1)
    ref.backward(dg.double().cpu().permute(0, 3, 1, 2).contiguous())
    return ref.detach().permute(0, 2, 3, 1).contiguous(), xr.grad.permute(0, 2, 3, 1).contiguous()


def _rel(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


def _shapes():
    band = 8                                                # the default height; test_default_band pins it
    return [(2, 32, 32, 64), (1, 1, 32, 64), (1, 2, 32, 64), (3, band + 1, 32, 64), (1, 2 * band - 1, 32, 64)]


def test_default_band():
    assert _band() == 8                                      # _shapes() is built around it


@pytest.mark.parametrize("B,H,W,C", _shapes())
def test_streaming_route_matches_the_gather_kernels_bit_for_bit(routes, B, H, W, C):
    from frl_hip import ops
    x, dg, add = _inputs((B, H, W, C), 1 + H), _inputs((B, H, W, 2 * C), 2 + H), _inputs((B, H, W, C), 3 + H)
    calls = {"fwd": lambda: ops.sobel_fwd(x), "bwd_add": lambda: ops.sobel_bwd(dg, add=add), "bwd": lambda: ops.sobel_bwd(dg)}
    out = {name: (routes(fn, True), routes(fn, False)) for name, fn in calls.items()}
    for name, (s, g) in out.items():
        assert torch.equal(_bits(s), _bits(g)), name
    # and both routes against float64 (test_sobel's check and tolerances)
    ref_g, ref_dx = _ref64(x, dg)
    for k in (0, 1):
        assert _rel(out["fwd"][k].float(), ref_g) <= ATOL[torch.bfloat16]
        assert _rel(out["bwd"][k].float(), ref_dx) <= 2 * ATOL[torch.bfloat16]
        assert _rel(out["bwd_add"][k].float(), ref_dx + add.double().cpu()) <= 2 * ATOL[torch.bfloat16]


@pytest.mark.parametrize("band", [1, 3, 16, 64])
def test_other_band_heights_match_too(routes, band):
    """Heights that do not divide H, one row per workgroup, H smaller than a band."""
    from frl_hip import ops
    B, H, W, C = 2, 13, 32, 64
    x, dg, add = _inputs((B, H, W, C), 21), _inputs((B, H, W, 2 * C), 22), _inputs((B, H, W, C), 23)
    want = routes(lambda: (ops.sobel_fwd(x), ops.sobel_bwd(dg, add=add), ops.sobel_bwd(dg)), False)
    was = ops.sobel_stream_band(band)
    try:
        got = routes(lambda: (ops.sobel_fwd(x), ops.sobel_bwd(dg, add=add), ops.sobel_bwd(dg)), True)
    finally:
        ops.sobel_stream_band(was)
    for g, w_ in zip(got, want):
        assert torch.equal(_bits(g), _bits(w_))


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, (1, 9, 13, 16)), (torch.float32, (1, 9, 13, 16)), (torch.float32, (2, 32, 32, 64))])
def test_shapes_outside_the_predicate_keep_the_gather_kernels(routes, dtype, shape):
    """W * C / 8 != 256, or float32: the switch changes nothing (same kernel either way) and the result matches float64."""
    from frl_hip import ops
    B, H, W, C = shape
    x, dg = _inputs(shape, 31, dtype), _inputs((B, H, W, 2 * C), 32, dtype)
    on = routes(lambda: (ops.sobel_fwd(x), ops.sobel_bwd(dg)), True)
    off = routes(lambda: (ops.sobel_fwd(x), ops.sobel_bwd(dg)), False)
    for a, b in zip(on, off):
        assert torch.equal(_bits(a), _bits(b))
    ref_g, ref_dx = _ref64(x, dg)
    assert _rel(on[0].float(), ref_g) <= ATOL[dtype]
    assert _rel(on[1].float(), ref_dx) <= 2 * ATOL[dtype]
