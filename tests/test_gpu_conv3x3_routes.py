"""GPU tests of the 3x3 convolution kernels (csrc/conv3x3.hip, csrc/conv3x3_wgrad.hip) on every tile, channel and store route of
tests/conv3x3_cases.py.

Exact tier: integer data on which float32 accumulation and bf16 stores are exact (conv3x3_cases.py says why, test_cpu_conv3x3_cases.py
checks it), float64 CPU references, torch.equal.  One dropped (tap, channel) term, a wrong channel guard or a skipped tile row changes an
integer and fails it.  Tolerance tier: the sigmoid paths on random data, with the tolerances of test_gpu_kernels_blocks.py::test_conv3x3.
"""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import conv3x3_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = {"f32": (3e-6, 2e-5), "bf16": (3e-2, 3e-2)}   # (activation tol, weight-grad tol) relative to max|ref|, as test_conv3x3


def _dev(t, dtype):
    return t.to(TORCH_DTYPE[dtype]).to(DEV).contiguous()


def _differs(got, want, what):
    """None when equal, else a description of the first mismatch (all comparisons of a test are reported together)."""
    got = got.detach().float().cpu()
    if got.shape != want.shape:
        return f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return None
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist())
    return f"{what}: {bad.shape[0]} of {want.numel()} values differ, first at {i}: got {got[i].item()}, want {want[i].item()}"


def rel_err(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6)


@contextlib.contextmanager
def hook(name, value):
    """Set one of the library's test hooks, restore the previous setting on the way out."""
    from frl_hip import _lib
    fn = getattr(_lib.load(), name)
    was = fn(value)
    try:
        yield
    finally:
        fn(was)


def _exact_conv_calls(case, dtype):
    """Every exact-tier call of the forward / bwd-data kernel on one kernel shape -> {expected-tensor name: device result}."""
    from frl_hip import ops
    inp, _ = C.conv_exact(case)
    x, ymask = _dev(inp["x"], dtype), _dev(inp["y_relu_mask"], dtype)
    w_fwd, bias, w_bwd = inp["w_fwd"].to(DEV), inp["bias"].to(DEV), inp["w_bwd"].to(DEV)
    add, sub = _dev(inp["add"], dtype), _dev(inp["sub_from"], dtype)
    got = {"y_none": ops.conv3x3_fwd(x, w_fwd, bias, ops.ACT_NONE), "y_relu": ops.conv3x3_fwd(x, w_fwd, bias, ops.ACT_RELU),
           "dx_plain": ops.conv3x3_bwd_data(x, w_bwd), "dx_mask": ops.conv3x3_bwd_data(x, w_bwd, ymask, ops.ACT_RELU),
           "dx_add": ops.conv3x3_bwd_data(x, w_bwd, ymask, ops.ACT_RELU, add=add)}
    got["dx_plain.sub"], got["out2_sub"] = ops.conv3x3_bwd_data(x, w_bwd, sub_from=sub)
    got["dx_add.both"], got["out2_both"] = ops.conv3x3_bwd_data(x, w_bwd, ymask, ops.ACT_RELU, add=add, sub_from=sub)
    got["dx_out_relu"] = ops.conv3x3_bwd_data(x, w_bwd, out_y=_dev(inp["out_y_relu"], dtype), out_act=ops.ACT_RELU)
    got["dx_out_sig"] = ops.conv3x3_bwd_data(x, w_bwd, ymask, ops.ACT_RELU, out_y=_dev(inp["out_y_sig"], dtype), out_act=ops.ACT_SIGMOID)
    return got


CONV_PARAMS = [pytest.param(c, d, id=f"{c.name}-{d}") for c in C.CONV_CASES for d in C.DTYPES]
WGRAD_PARAMS = [pytest.param(c, d, id=f"{c.name}-{d}") for c in C.WGRAD_CASES for d in C.DTYPES]


@pytest.mark.parametrize("case,dtype", CONV_PARAMS)
def test_forward_and_bwd_data_are_exact_on_integer_data(case, dtype):
    """Forward (none, ReLU), bwd-data (plain, ReLU mask), the add / sub_from / both epilogues and the out_y epilogues (ReLU; sigmoid with
    out_y in {0, 0.5, 1}) against float64, bit for bit."""
    _, exp = C.conv_exact(case)
    got = _exact_conv_calls(case, dtype)
    torch.cuda.synchronize()
    assert set(k.split(".")[0] for k in got) == set(exp)
    bad = [m for m in (_differs(g, exp[k.split(".")[0]], k) for k, g in got.items()) if m]
    assert not bad, f"{case.name} {dtype} {C.conv_route(dtype, case.B, case.H, case.W, case.Cr, case.Cp)}:\n" + "\n".join(bad)


@pytest.mark.parametrize("case,dtype", WGRAD_PARAMS)
def test_weight_gradient_is_exact_on_integer_data(case, dtype):
    """dw and db without and with a ReLU mask, vector and scalar fragment reads, with and without the bias gradient."""
    from frl_hip import ops
    inp, exp = C.wgrad_exact(case)
    x, dy, ymask = _dev(inp["x"], dtype), _dev(inp["dy"], dtype), _dev(inp["y_relu_mask"], dtype)
    bad = []
    for mask in C.WGRAD_MASKS:
        y, act = (ymask, ops.ACT_RELU) if mask == "relu" else (None, ops.ACT_NONE)
        for scalar in (False, True):
            for want_bias in (True, False):
                dw, db = ops.conv3x3_bwd_weight(dy, x, y, act, scalar_frags=scalar, want_bias=want_bias)
                tag = f"mask={mask} scalar_frags={scalar} want_bias={want_bias}"
                bad.append(_differs(dw, exp[f"dw_{mask}"], f"dw {tag}"))
                if want_bias:
                    bad.append(_differs(db, exp[f"db_{mask}"], f"db {tag}"))
                else:
                    assert db is None
    bad = [m for m in bad if m]
    assert not bad, f"{case.name} {dtype} {C.wgrad_route(dtype, case.B, case.H, case.W, case.Cin, case.Cout)}:\n" + "\n".join(bad)


TALL_CASES = [c for c in C.CONV_CASES if c.H >= C.TALL_MIN_H]


@pytest.mark.parametrize("case", TALL_CASES, ids=lambda c: c.name)
def test_tile32_hook_both_tile_heights_give_the_same_exact_result(case):
    """frl_conv3x3_tile32(0) sends a bf16 image of >= 32 rows through the 16-row tile (for 75 x 33 x 17: 450 tiles, the persistent loop
    of THAT instantiation); both settings must give the float64 result on every call of the exact tier."""
    assert C.conv_route("bf16", case.B, case.H, case.W, case.Cr, case.Cp, tile32=True)["th"] == 32
    _, exp = C.conv_exact(case)
    res = {}
    for on in (0, 1):
        with hook("frl_conv3x3_tile32", on):
            res[on] = _exact_conv_calls(case, "bf16")
            torch.cuda.synchronize()
    bad = []
    for k in res[0]:
        if not torch.equal(res[0][k], res[1][k]):
            bad.append(f"{k}: the 16-row and the 32-row tile disagree")
        bad += [m for m in (_differs(res[on][k], exp[k.split(".")[0]], f"{k} tile32={on}") for on in (0, 1)) if m]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)


def test_tile32_hook_returns_and_restores_the_setting():
    from frl_hip import _lib
    lib = _lib.load()
    was = lib.frl_conv3x3_tile32(0)
    try:
        assert was == 1 and lib.frl_conv3x3_tile32(1) == 0 and lib.frl_conv3x3_tile32(1) == 1
    finally:
        lib.frl_conv3x3_tile32(was)
    was = lib.frl_conv3x3_wgrad_force_generic(1)
    try:
        assert was == 0 and lib.frl_conv3x3_wgrad_force_generic(0) == 1 and lib.frl_conv3x3_wgrad_force_generic(0) == 0
    finally:
        lib.frl_conv3x3_wgrad_force_generic(was)


BAND_CASES = [c for c in C.WGRAD_CASES if C.wgrad_route("bf16", c.B, c.H, c.W, c.Cin, c.Cout)["kernel"] == "band"]


@pytest.mark.parametrize("case", BAND_CASES, ids=lambda c: c.name)
def test_wgrad_force_generic_hook_band_and_generic_kernels_agree(case):
    from frl_hip import ops
    inp, exp = C.wgrad_exact(case)
    x, dy, ymask = _dev(inp["x"], "bf16"), _dev(inp["dy"], "bf16"), _dev(inp["y_relu_mask"], "bf16")
    bad = []
    for mask in C.WGRAD_MASKS:
        y, act = (ymask, ops.ACT_RELU) if mask == "relu" else (None, ops.ACT_NONE)
        res = {}
        for on in (1, 0):
            with hook("frl_conv3x3_wgrad_force_generic", on):
                res[on] = ops.conv3x3_bwd_weight(dy, x, y, act)
                torch.cuda.synchronize()
        for i, nm in enumerate(("dw", "db")):
            if not torch.equal(res[0][i], res[1][i]):
                bad.append(f"{nm} mask={mask}: band and generic kernel disagree")
            bad += [m for m in (_differs(res[on][i], exp[f"{nm}_{mask}"], f"{nm} mask={mask} force_generic={on}") for on in (0, 1)) if m]
    assert len(BAND_CASES) >= 5 and not bad, f"{case.name}:\n" + "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------------------------
# Tolerance tier
# ----------------------------------------------------------------------------------------------------------------------------------
def _q(t, dtype):
    return t.to(TORCH_DTYPE[dtype]).double()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _random_layer(B, H, W, cin, cout, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = _q(torch.randn(B, H, W, cin, generator=g), dtype)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)
    wq = _q(w, dtype) if dtype == "bf16" else w.double()         # the bf16 kernels round the float32 master weights to bf16
    b = (torch.randn(cout, generator=g) * 0.1).float()
    return g, x, w, wq, b


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("B,H,W,cin,cout", C.TOL_SHAPES)
def test_sigmoid_paths_match_float64(B, H, W, cin, cout, dtype):
    """Forward sigmoid; bwd-data and weight gradient through the sigmoid mask (the DEVICE output as the mask, as autograd does); the
    sigmoid out_y epilogue (mode 3); the gate blend (mode 1)."""
    from frl_hip import ops
    atol, wtol = MODES[dtype]
    g, x, w, wq, b = _random_layer(B, H, W, cin, cout, dtype, 1000 + H * W + cin + cout)
    dy = _q(torch.randn(B, H, W, cout, generator=g), dtype)
    out_y = _q(torch.sigmoid(torch.randn(B, H, W, cin, generator=g)), dtype)
    sm, res = _q(torch.randn(B, H, W, cout, generator=g), dtype), _q(torch.randn(B, H, W, cout, generator=g), dtype)
    xd, dyd, wd, bd = _dev(x, dtype), _dev(dy, dtype), w.float().to(DEV), b.to(DEV)
    err = {}
    y_ref = torch.sigmoid(_nhwc(F.conv2d(_nchw(x), wq, b.double(), padding=1)))
    yd = ops.conv3x3_fwd(xd, wd, bd, ops.ACT_SIGMOID)
    err["fwd_sigmoid"] = (rel_err(yd.float(), y_ref), atol)
    yq = yd.float().cpu().double()
    dpre = dy * yq * (1 - yq)
    dx_ref = _nhwc(F.conv_transpose2d(_nchw(dpre), wq, padding=1))
    err["dx_sigmoid_mask"] = (rel_err(ops.conv3x3_bwd_data(dyd, wd, yd, ops.ACT_SIGMOID).float(), dx_ref), atol * 2)
    dw_ref = torch.nn.grad.conv2d_weight(_nchw(x), (cout, cin, 3, 3), _nchw(dpre), padding=1)
    for scalar in (False, True):
        dw, db = ops.conv3x3_bwd_weight(dyd, xd, yd, ops.ACT_SIGMOID, scalar_frags=scalar)
        err[f"dw_sigmoid_mask.scalar={scalar}"] = (rel_err(dw, dw_ref), wtol * 2)
        err[f"db_sigmoid_mask.scalar={scalar}"] = (rel_err(db, dpre.sum(dim=(0, 1, 2))), wtol * 2)
    dx3 = ops.conv3x3_bwd_data(dyd, wd, yd, ops.ACT_SIGMOID, out_y=_dev(out_y, dtype), out_act=ops.ACT_SIGMOID)
    err["dx_out_y_sigmoid"] = (rel_err(dx3.float(), dx_ref * out_y * (1 - out_y)), atol * 2)
    out, gate = ops.conv3x3_fwd_gate_blend(xd, wd, bd, _dev(sm, dtype), _dev(res, dtype))
    err["gate_blend.gate"] = (rel_err(gate.float(), y_ref), atol)
    err["gate_blend.out"] = (rel_err(out.float(), sm + y_ref * res), atol)
    for k, (e, tol) in err.items():
        print(f"conv3x3 tolerance tier {(B, H, W, cin, cout)} {dtype} {k}: {e:.3e} (ceiling {tol:.1e})")
    bad = {k: v for k, v in err.items() if not v[0] <= v[1]}
    assert not bad, bad


@pytest.mark.parametrize("case,dtype", CONV_PARAMS)
def test_gate_blend_epilogue_matches_float64_on_every_route(case, dtype):
    """Epilogue mode 1 (gate = sigmoid(conv + bias), out = smoothed + gate * residual) cannot be exact; it is held to the forward
    tolerance on every route of the table, on random data."""
    from frl_hip import ops
    atol, _ = MODES[dtype]
    B, H, W, cin, cout = case.B, case.H, case.W, case.Cr, case.Cp
    g, x, w, wq, b = _random_layer(B, H, W, cin, cout, dtype, case.seed % 100003)
    sm, res = _q(torch.randn(B, H, W, cout, generator=g), dtype), _q(torch.randn(B, H, W, cout, generator=g), dtype)
    gate_ref = torch.sigmoid(_nhwc(F.conv2d(_nchw(x), wq, b.double(), padding=1)))
    out, gate = ops.conv3x3_fwd_gate_blend(_dev(x, dtype), w.float().to(DEV), b.to(DEV), _dev(sm, dtype), _dev(res, dtype))
    e_gate, e_out = rel_err(gate.float(), gate_ref), rel_err(out.float(), sm + gate_ref * res)
    print(f"conv3x3 gate blend {case.name} {dtype}: gate {e_gate:.3e}, out {e_out:.3e} (ceiling {atol:.1e})")
    assert e_gate <= atol and e_out <= atol, (case.name, dtype, e_gate, e_out)
