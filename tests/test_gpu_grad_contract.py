"""The gradient contract of the autograd wrappers when not every tensor wants a gradient (frozen parameters, a frozen input) and when not
every output feeds the loss (None upstream gradients), with and without ops.deferred_reductions.

For every requires_grad mask of a row: a frozen tensor ends with .grad None, every trainable gradient equals the all-trainable run's bit
for bit, the backward gives the same bits with and without deferral and leaves nothing parked; the all-trainable run itself is held
against a float64 reference with the tolerance of the op's own parity test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import frl_oracle as O  # noqa: E402

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32


def rel_err(got, ref, floor=1e-6):
    ref = ref.double().cpu()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), floor)


def q(t, dtype):
    """The float64 value of t rounded to the storage dtype."""
    return t.to(dtype).double()


def _lib():
    from frl_hip import _lib
    return _lib.load()


def _backward(ts, outs, ups, defer):
    from frl_hip import ops
    pairs = [(o, u) for o, u in zip(outs, ups) if u is not None and o is not None and o.requires_grad]
    params = [t for t in ts.values() if t.requires_grad]
    if defer:
        with ops.deferred_reductions(params):
            torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    else:
        torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
    torch.cuda.synchronize()
    assert _lib().frl_defer_pending() == 0
    return {n: (None if t.grad is None else t.grad.detach().clone()) for n, t in ts.items()}


def _run(row, trainable, defer):
    ts = {n: v.detach().clone().to(DEV).requires_grad_(n in trainable) for n, v in row["leaves"].items()}
    outs = row["fn"](ts)
    return _backward(ts, outs, row["ups"], defer)


def _masks(row):
    names = list(row["leaves"])
    inputs = [n for n in names if n in row.get("inputs", ())]
    params = [n for n in names if n not in inputs]
    masks = [("all", set(names))]
    if inputs:
        masks += [("inputs", set(inputs)), ("params", set(params))]
    masks += [(f"frozen:{p}", set(names) - {p}) for p in params]
    for w, b in row.get("wb", ()):                                   # bias-carrying convolutions: one of the pair trains alone
        masks += [(f"only:{w}", {w}), (f"only:{b}", {b})]
    return masks


def _check_row(row):
    """The whole mask sweep of one row."""
    full = _run(row, set(row["leaves"]), False)
    errs = {n: rel_err(full[n], row["ref"][n], row.get("floor", 1e-6)) for n in row["tol"]}    # the all-trainable run against float64
    assert all(errs[n] <= row["tol"][n] for n in errs), str(sorted(errs.items()))
    for label, mask in _masks(row):
        if not any(n in mask for n in row["tol"]) and not any(n in mask for n in row.get("inputs", ())):
            continue
        got = _run(row, mask, False)
        dfr = _run(row, mask, True)
        for n in row["leaves"]:
            if n not in mask:
                assert got[n] is None and dfr[n] is None, (label, n)
                continue
            assert torch.equal(got[n], dfr[n]), (label, n, "deferral changed the bits")
            # (the no-dx TCN backward that runs when the input needs no gradient gives the same parameter-gradient bits too)
            assert torch.equal(got[n], full[n]), (label, n, "bits differ from the all-trainable run")


def _ref_grads(ref_leaves, outs, ups):
    pairs = [(o, u) for o, u in zip(outs, ups) if u is not None]
    torch.autograd.backward([o for o, _ in pairs], [u.double().cpu() for _, u in pairs])
    return {n: t.grad for n, t in ref_leaves.items() if t.grad is not None}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
def conv1x1_row(dtype, p, cin, cout, bias, act):
    from frl_hip import functional as Fh
    g = _gen(p + cin + cout)
    x = torch.randn(p, cin, generator=g).to(dtype)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    leaves = {"x": x, "w": w}
    if bias:
        leaves["b"] = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(p, cout, generator=g).to(dtype)
    r = {n: (q(v, dtype) if (n == "w" and dtype == BF) else v.double()).requires_grad_(True) for n, v in leaves.items()}
    r["x"] = q(x, dtype).requires_grad_(True)
    y = r["x"] @ r["w"].T + (r["b"] if bias else 0.0)
    if act == 1:                                                     # the ReLU mask the kernel applied (values at 0 are not under test)
        yk = Fh.conv1x1(x.to(DEV), w.to(DEV), leaves["b"].to(DEV) if bias else None, act).cpu()
        y = y * (yk > 0).double()
    # test_conv1x1_bwd: |err| <= tol * max(max|ref|, 1), tol 2e-2 / 2e-6 for dx and 4 x 2e-5 for dW, db
    wt = 4 * 2e-5
    return dict(leaves=leaves, inputs=("x",), wb=[("w", "b")] if bias else [], floor=1.0,
                fn=lambda t: (Fh.conv1x1(t["x"], t["w"], t.get("b"), act),), ups=[dy.to(DEV)],
                ref=_ref_grads(r, [y], [dy]), tol={"x": 2e-2 if dtype == BF else 2e-6, "w": wt, **({"b": wt} if bias else {})})


def conv3x3_row(dtype, B, H, W, cin, cout, bias, act):
    from frl_hip import functional as Fh
    g = _gen(B * H * W + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g).to(dtype)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    leaves = {"x": x, "w": w}
    if bias:
        leaves["b"] = torch.randn(cout, generator=g) * 0.1
    dy = torch.randn(B, H, W, cout, generator=g).to(dtype)
    wt = 2 * (3e-2 if dtype == BF else 2e-5)
    r = {n: (q(v, dtype) if (n == "w" and dtype == BF) else v.double()).requires_grad_(True) for n, v in leaves.items()}
    r["x"] = q(x, dtype).requires_grad_(True)
    y = F.conv2d(r["x"].permute(0, 3, 1, 2), r["w"], r.get("b"), padding=1)
    y = (torch.relu(y) if act == 1 else torch.sigmoid(y) if act == 2 else y).permute(0, 2, 3, 1)
    return dict(leaves=leaves, inputs=("x",), wb=[("w", "b")] if bias else [],
                fn=lambda t: (Fh.conv3x3(t["x"], t["w"], t.get("b"), act),), ups=[dy.to(DEV)],
                ref=_ref_grads(r, [y], [dy]), tol={"x": 2 * (3e-2 if dtype == BF else 3e-6), "w": wt, **({"b": wt} if bias else {})})


def groupnorm_row(dtype, B, HW, C, G, relu):
    from frl_hip import functional as Fh
    g = _gen(B * HW + C)
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + 0.3).to(dtype)
    leaves = {"x": x, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g) * 0.2}
    dy = torch.randn(B, HW, C, generator=g).to(dtype)
    r = {n: (q(v, dtype) if n == "x" else v.double()).requires_grad_(True) for n, v in leaves.items()}
    y = O.group_norm(r["x"].permute(0, 2, 1), G, r["gamma"], r["beta"]).permute(0, 2, 1)
    y = torch.relu(y) if relu else y
    at, wt = (3e-2, 3e-2) if dtype == BF else (3e-6, 2e-5)
    return dict(leaves=leaves, inputs=("x",), fn=lambda t: (Fh.group_norm(t["x"], t["gamma"], t["beta"], G, 1e-5, relu),),
                ups=[dy.to(DEV)], ref=_ref_grads(r, [y], [dy]), tol={"x": 2 * at, "gamma": wt, "beta": wt})


def encoder2_row(B, H, W):
    """csrc/enc_fused.hip (bf16 64 -> 128 -> 64); its input is data: parameters only."""
    from frl_hip import functional as Fh, ops
    g = _gen(B * H + W)
    x = torch.randn(B, H, W, 64, generator=g).to(BF)
    leaves = {"w1": torch.randn(128, 64, generator=g) / 8.0, "g1": torch.randn(128, generator=g) * 0.3 + 1.0,
              "b1": torch.randn(128, generator=g) * 0.3, "w2": torch.randn(64, 128, generator=g) / 128 ** 0.5,
              "g2": torch.randn(64, generator=g) * 0.3 + 1.0, "b2": torch.randn(64, generator=g) * 0.3}
    assert ops.encoder2_supported(64, 128, 64, 8, 8, H * W, BF)
    dz = torch.randn(B, H, W, 64, generator=g).to(BF)
    r = {n: (q(v, BF) if v.dim() == 2 else v.double()).requires_grad_(True) for n, v in leaves.items()}
    xc = q(x, BF).permute(0, 3, 1, 2)
    h = F.relu(O.group_norm(F.conv2d(xc, r["w1"][:, :, None, None]), 8, r["g1"], r["b1"]))
    z = O.group_norm(F.conv2d(h, r["w2"][:, :, None, None]), 8, r["g2"], r["b2"]).permute(0, 2, 3, 1)
    xd = x.to(DEV)
    return dict(leaves=leaves, fn=lambda t: (Fh.encoder2(xd, *[t[n] for n in ("w1", "g1", "b1", "w2", "g2", "b2")]),), ups=[dz.to(DEV)],
                ref=_ref_grads(r, [z], [dz]), tol={n: 1.5e-2 for n in leaves})       # test_fused_two_layer_encoder_matches_float64...


TCN_NAMES = ("conv.weight", "conv.bias", "norm.weight", "norm.bias", "gate.weight", "gate.bias", "projection.weight", "projection.bias")


def _tcn_state(g, cin, cout, prefix=""):
    st = {prefix + "conv.weight": torch.randn(cout, cin, 3, generator=g) / (3 * cin) ** 0.5,
          prefix + "conv.bias": torch.randn(cout, generator=g) * 0.1, prefix + "norm.weight": torch.rand(cout, generator=g) + 0.5,
          prefix + "norm.bias": torch.randn(cout, generator=g) * 0.2, prefix + "gate.weight": torch.randn(cout, cout, 1, generator=g) / cout ** 0.5,
          prefix + "gate.bias": torch.randn(cout, generator=g) * 0.1}
    if cin != cout:
        st[prefix + "projection.weight"] = torch.randn(cout, cin, 1, generator=g) / cin ** 0.5
        st[prefix + "projection.bias"] = torch.randn(cout, generator=g) * 0.1
    return st


def _ref_state(st, dtype):
    mm = ("conv.weight", "gate.weight", "projection.weight", "head.weight")
    return {k: (q(v, dtype) if (dtype == BF and k.endswith(mm)) else v.double()).requires_grad_(True) for k, v in st.items()}


def tcn_block_row(dtype, B, T, HW, cin, cout, G, dil):
    from frl_hip import functional as Fh
    g = _gen(T * HW + cin + cout + dil)
    st = _tcn_state(g, cin, cout)
    x = torch.randn(B, T, HW, cin, generator=g).to(dtype)
    dy = torch.randn(B, T, HW, cout, generator=g).to(dtype)
    leaves = {"x": x, **st}
    r = _ref_state(st, dtype)
    r["x"] = q(x, dtype).requires_grad_(True)
    xr = r["x"].permute(0, 2, 3, 1).reshape(B * HW, cin, T)
    y = O.tcn_block_forward(r, xr, dil, G, "").reshape(B, HW, cout, T).permute(0, 3, 1, 2)
    at, wt = (3e-2, 3e-2) if dtype == BF else (3e-6, 2e-5)

    def fn(t):
        return (Fh.TcnBlockFn.apply(t["x"], *[t.get(n) for n in TCN_NAMES], dil, G, 1e-5),)
    return dict(leaves=leaves, inputs=("x",), wb=[("conv.weight", "conv.bias")], fn=fn, ups=[dy.to(DEV)],
                ref=_ref_grads(r, [y], [dy]), tol={"x": 4 * at, **{n: 4 * wt for n in st}})


def chain_head_row(B, HW, head_in_kernel):
    """Three hot GatedResidualBlocks + the 1x1 phase head (TcnChainHeadFn), bf16 64 channels, T = 5, head 12 channels.  The reference is
    the block-by-block composition (TcnBlockFn x 3 + conv1x1, each held against float64 by its own parity test), with the bounds of
    test_phase_chain_forward_in_one_launch_equals_the_block_by_block_path: the same bits when the head's backward-data is its own launch;
    1e-2 on the parameter gradients and 1.6e-2 on the input gradient when the last block's kernel takes dh itself."""
    from frl_hip import functional as Fh
    g = _gen(B * HW)
    T, G = 5, 8
    st = {}
    for i in range(3):
        st.update(_tcn_state(g, 64, 64, f"l{i}."))
    st["head.weight"] = torch.randn(12, 64, 1, 1, generator=g) / 8.0
    st["head.bias"] = torch.randn(12, generator=g) * 0.1
    x = torch.randn(B, T, HW, 64, generator=g).to(BF)
    dh = torch.randn(B, T, HW, 12, generator=g).to(BF).to(DEV)
    order = [f"l{i}.{n}" for i in range(3) for n in TCN_NAMES[:6]] + ["head.weight", "head.bias"]
    r = {n: v.to(DEV).requires_grad_(True) for n, v in {"x": x, **st}.items()}
    h = r["x"]
    for i, d in enumerate((1, 2, 4)):
        h = Fh.TcnBlockFn.apply(h, *[r[f"l{i}.{n}"] for n in TCN_NAMES[:6]], None, None, d, G, 1e-5)
    Fh.conv1x1(h, r["head.weight"], r["head.bias"]).backward(dh)
    ref = {n: t.grad.detach().clone() for n, t in r.items()}

    def fn(t):
        return (Fh.TcnChainHeadFn.apply(t["x"], *[t[n] for n in order], G, 1e-5),)
    tol = {"x": 1.6e-2, **{n: 1e-2 for n in st}} if head_in_kernel else {n: 0.0 for n in ref}
    return dict(leaves={"x": x, **st}, inputs=("x",), wb=[("head.weight", "head.bias")], fn=fn, ups=[dh], ref=ref, tol=tol)


def film_fused_row(B, T, HW):
    from frl_hip import functional as Fh
    g = _gen(B * T + HW)
    zt = torch.randn(B, HW, 64, generator=g).to(BF)
    h = torch.randn(B, T, HW, 12, generator=g).to(BF)
    names = ["w1g", "b1g", "w2g", "b2g", "w1b", "b1b", "w2b", "b2b"]
    shapes = [(32, 64), (32,), (12, 32), (12,), (32, 64), (32,), (12, 32), (12,)]
    leaves = {"h": h, **{n: torch.randn(*s, generator=g) * (0.3 if len(s) == 2 else 0.5) for n, s in zip(names, shapes)}}
    dz = torch.randn(B, T, HW, 12, generator=g).to(BF)
    r = {n: (q(v, BF) if v.dim() == 2 or n == "h" else v.double()).requires_grad_(True) for n, v in leaves.items()}
    ztr = q(zt, BF)
    gamma = torch.relu(ztr @ r["w1g"].T + r["b1g"]) @ r["w2g"].T + r["b2g"]
    beta = torch.relu(ztr @ r["w1b"].T + r["b1b"]) @ r["w2b"].T + r["b2b"]
    z = gamma.unsqueeze(1) * r["h"] + beta.unsqueeze(1)
    ztd = zt.to(DEV)

    def fn(t):
        return Fh.FilmFusedFn.apply(t["h"], ztd, *[t[n] for n in names])
    return dict(leaves=leaves, inputs=("h",), fn=fn, ups=[dz.to(DEV), None, None], ref=_ref_grads(r, [z], [dz]),
                tol={"h": 1e-2, **{n: 2e-2 for n in names}})


def decoder_mse_row(P, cz, use_mask):
    from frl_hip import functional as Fh
    g = _gen(P + cz)
    leaves = {"z": torch.randn(P, cz, generator=g).to(BF), "w1": torch.randn(128, cz, 1, 1, generator=g) / cz ** 0.5,
              "b1": torch.randn(128, generator=g) * 0.1, "w2": torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5,
              "b2": torch.randn(64, generator=g) * 0.1}
    target = torch.randn(P, 64, generator=g).to(BF)
    mask = (torch.rand(P, generator=g) > 0.3) if use_mask else None
    r = {n: (q(v, BF) if n in ("z", "w1", "w2") else v.double()).requires_grad_(True) for n, v in leaves.items()}
    hid = torch.relu(r["z"] @ r["w1"][:, :, 0, 0].T + r["b1"])
    xhat = hid @ r["w2"][:, :, 0, 0].T + r["b2"]
    m = torch.ones(P, dtype=torch.bool) if mask is None else mask
    loss = ((xhat - q(target, BF)) ** 2)[m].mean()
    td, md = target.to(DEV), (None if mask is None else mask.to(DEV))

    def fn(t):
        return Fh.decoder_mse(t["z"], t["w1"], t["b1"], t["w2"], t["b2"], td, md, want_xhat=True)
    return dict(leaves=leaves, inputs=("z",), wb=[("w1", "b1"), ("w2", "b2")], fn=fn, ups=[torch.ones((), device=DEV), None],
                ref=_ref_grads(r, [loss], [torch.ones((), dtype=torch.float64)]), tol={n: 3e-2 for n in leaves})      # test_fused_decoder_mse


def vq_row(dtype, N, K, d):
    """VQFn: the straight-through quantizer with the codebook as a parameter ("all") and as a non-parameter ("inputs" mask)."""
    from frl_hip import functional as Fh
    g = _gen(N + K + d)
    z = torch.randn(N, d, generator=g).to(dtype)
    cb = torch.randn(K, d, generator=g)
    gzq = torch.randn(N, d, generator=g).to(dtype)
    ups = [gzq.to(DEV), torch.tensor(1.3, device=DEV), torch.tensor(0.25, device=DEV), None, None, None, None]
    r = {"z": q(z, dtype).requires_grad_(True), "codebook": cb.double().requires_grad_(True)}
    idx = Fh.VQFn.apply(z.to(DEV), cb.to(DEV))[4].long().cpu()              # (the kernel's assignment: near-ties are not under test)
    # in bf16 the kernels see the codebook rounded to bf16 (test_vq_bwd_and_ema: e_eff): the rounded value, the identity derivative
    e_eff = r["codebook"] + (q(cb, dtype) - cb.double())
    zq = e_eff[idx]
    lcb = ((r["z"].detach() - zq) ** 2).mean()
    lcm = ((r["z"] - zq.detach()) ** 2).mean()
    zst = r["z"] + (zq - r["z"]).detach()
    ref = _ref_grads(r, [zst, lcb, lcm], [gzq.double(), torch.tensor(1.3, dtype=torch.float64), torch.tensor(0.25, dtype=torch.float64)])
    return dict(leaves={"z": z, "codebook": cb}, inputs=("z",), fn=lambda t: Fh.VQFn.apply(t["z"], t["codebook"]), ups=ups, ref=ref,
                tol={"z": 1e-2 if dtype == BF else 1e-6, "codebook": 1e-4})          # test_vq_bwd_and_ema


def film_row(dtype):
    """FilmFn (unfused modulation); test_streaming_ops: dh within atol, dgamma / dbeta within 2 atol."""
    from frl_hip import functional as Fh
    g = _gen(31)
    B, T, P, C = 2, 5, 64, 12
    leaves = {"h": torch.randn(B, T, P, C, generator=g).to(dtype), "gamma": torch.randn(B, P, C, generator=g).to(dtype),
              "beta": torch.randn(B, P, C, generator=g).to(dtype)}
    do = torch.randn(B, T, P, C, generator=g).to(dtype)
    r = {n: q(v, dtype).requires_grad_(True) for n, v in leaves.items()}
    out = r["gamma"].unsqueeze(1) * r["h"] + r["beta"].unsqueeze(1)
    at = 3e-2 if dtype == BF else 3e-6
    return dict(leaves=leaves, inputs=("h",), fn=lambda t: (Fh.FilmFn.apply(t["h"], t["gamma"], t["beta"]),), ups=[do.to(DEV)],
                ref=_ref_grads(r, [out], [do]), tol={"h": at, "gamma": 2 * at, "beta": 2 * at})


def edge_smooth_row(dtype):
    """EdgeSmoothFn (both outputs feed the loss); test_edge_smooth_stencil: every gradient within 3 atol."""
    from frl_hip import functional as Fh
    from test_gpu_kernels_blocks import _smooth_ref
    g = _gen(32)
    B, H, W, C, R = 1, 8, 8, 8, 4
    leaves = {"x": torch.randn(B, H, W, C, generator=g).to(dtype), "a": torch.randn(B, H, W, 8 * R, generator=g).to(dtype),
              "b": torch.randn(B, H, W, C * R, generator=g).to(dtype)}
    ups = [torch.randn(B, H, W, C, generator=g).to(dtype) for _ in range(2)]
    r = {n: q(v, dtype).requires_grad_(True) for n, v in leaves.items()}
    sm, res = _smooth_ref(*(r[n].permute(0, 3, 1, 2) for n in ("x", "a", "b")), R, 3)
    at = 3e-2 if dtype == BF else 3e-6
    return dict(leaves=leaves, inputs=("x", "a", "b"), fn=lambda t: Fh.EdgeSmoothFn.apply(t["x"], t["a"], t["b"], R, 3),
                ups=[u.to(DEV) for u in ups], ref=_ref_grads(r, [sm.permute(0, 2, 3, 1), res.permute(0, 2, 3, 1)], ups),
                tol={n: 3 * at for n in leaves})


def gate_blend_row(dtype, min_gate):
    """GateBlendFn, both outputs feeding the loss; test_streaming_ops: every gradient within atol."""
    from frl_hip import functional as Fh
    g = _gen(33)
    leaves = {"sm": torch.randn(64, 16, generator=g).to(dtype), "res": torch.randn(64, 16, generator=g).to(dtype),
              "graw": torch.rand(64, 16, generator=g).to(dtype)}
    ups = [torch.randn(64, 16, generator=g).to(dtype) for _ in range(2)]
    r = {n: q(v, dtype).requires_grad_(True) for n, v in leaves.items()}
    gate = r["graw"].clamp(min=min_gate) if min_gate > 0 else r["graw"]
    at = 3e-2 if dtype == BF else 3e-6
    return dict(leaves=leaves, inputs=tuple(leaves), fn=lambda t: Fh.GateBlendFn.apply(t["sm"], t["res"], t["graw"], min_gate),
                ups=[u.to(DEV) for u in ups], ref=_ref_grads(r, [r["sm"] + gate * r["res"], gate], ups), tol={n: at for n in leaves})


def mse_row(dtype, use_mask):
    """MseFn (the target is data); test_streaming_ops: dpred within atol."""
    from frl_hip import functional as Fh
    g = _gen(34)
    pred, target = torch.randn(300, 64, generator=g).to(dtype), torch.randn(300, 64, generator=g).to(dtype)
    mask = (torch.rand(300, generator=g) > 0.3) if use_mask else None
    r = {"pred": q(pred, dtype).requires_grad_(True)}
    loss = O.reconstruction_loss_l2(r["pred"], q(target, dtype), mask.unsqueeze(1).expand(300, 64) if use_mask else None)
    td, md = target.to(DEV), (None if mask is None else mask.to(DEV))
    return dict(leaves={"pred": pred}, inputs=("pred",), fn=lambda t: (Fh.mse_loss(t["pred"], td, md),),
                ups=[torch.tensor(0.7, device=DEV)], ref=_ref_grads(r, [loss], [torch.tensor(0.7)]),
                tol={"pred": 3e-2 if dtype == BF else 3e-6})


def channel_scale_row(dtype):
    """ChannelScaleFn (the Dropout2d scale is data); test_channel_scale_dropout2d: 1e-6 / 8e-3."""
    from frl_hip import functional as Fh
    g = _gen(35)
    x = torch.randn(3, 5, 7, 16, generator=g).to(dtype)
    sc = (torch.rand(3, 16, generator=g) > 0.3).float() * 2.0
    dy = torch.randn(3, 5, 7, 16, generator=g).to(dtype)
    r = {"x": q(x, dtype).requires_grad_(True)}
    y = r["x"] * sc.double().view(3, 1, 1, 16)
    scd = sc.to(dtype).to(DEV)
    return dict(leaves={"x": x}, inputs=("x",), fn=lambda t: (Fh.ChannelScaleFn.apply(t["x"], scd),), ups=[dy.to(DEV)],
                ref=_ref_grads(r, [y], [dy]), tol={"x": 8e-3 if dtype == BF else 1e-6})


def gather_row():
    """_GatherFn (extract_at_locations); test_extract_at_locations_matches_reference: within 1e-6 (absolute, gradients of order 1)."""
    from frl_hip.utils import extract_at_locations
    g = _gen(36)
    feat = torch.randn(16, 20, 24, generator=g)
    coords = torch.stack([torch.randint(0, 20, (300,), generator=g), torch.randint(0, 24, (300,), generator=g)], 1)
    w = torch.randn(300, 16, generator=g)
    r = {"feat": feat.double().requires_grad_(True)}
    out = r["feat"][:, coords[:, 0], coords[:, 1]].T
    cd = coords.to(DEV)
    return dict(leaves={"feat": feat}, inputs=("feat",), fn=lambda t: (extract_at_locations(t["feat"], cd),), ups=[w.to(DEV)],
                ref=_ref_grads(r, [out], [w]), tol={"feat": 1e-6}, floor=1.0)


def infonce_row(sim):
    """_InfoNCEFn (contrastive_loss); test_contrastive_loss_matches_reference: within 1e-5 of max|grad|."""
    from frl_hip.losses.contrastive import contrastive_loss
    g = _gen(37)
    emb = torch.randn(64, 16, generator=g)
    pos = torch.randint(0, 64, (80, 2), generator=g)
    neg = torch.randint(0, 64, (300, 2), generator=g)
    pw = torch.rand(80, generator=g) + 0.5
    r = {"emb": emb.double().requires_grad_(True)}
    loss = O.contrastive_loss_oracle(r["emb"], pos, neg, pw.double(), None, temperature=0.1, similarity=sim)
    pd, nd, pwd = pos.to(DEV), neg.to(DEV), pw.to(DEV)
    return dict(leaves={"emb": emb}, inputs=("emb",), ups=[torch.tensor(1.0, device=DEV)],
                fn=lambda t: (contrastive_loss(t["emb"], pd, nd, pwd, None, temperature=0.1, similarity=sim),),
                ref=_ref_grads(r, [loss], [torch.tensor(1.0)]), tol={"emb": 1e-5})


ROWS = {
    "conv1x1-hot": lambda: conv1x1_row(BF, 4096, 64, 64, True, 1),
    "conv1x1-hot-nobias": lambda: conv1x1_row(BF, 4096, 64, 64, False, 0),
    "conv1x1-f32": lambda: conv1x1_row(F32, 333, 24, 16, True, 0),
    "conv1x1-f32-nobias": lambda: conv1x1_row(F32, 333, 24, 16, False, 1),
    "conv3x3-hot": lambda: conv3x3_row(BF, 2, 32, 32, 64, 64, True, 1),
    "conv3x3-hot-nobias": lambda: conv3x3_row(BF, 2, 32, 32, 64, 64, False, 0),
    "conv3x3-f32": lambda: conv3x3_row(F32, 1, 13, 21, 16, 8, True, 2),
    "conv3x3-f32-nobias": lambda: conv3x3_row(F32, 1, 13, 21, 16, 8, False, 1),
    "groupnorm-hot": lambda: groupnorm_row(BF, 2, 1024, 64, 8, True),
    "groupnorm-f32": lambda: groupnorm_row(F32, 2, 100, 16, 4, False),
    "encoder2-hot": lambda: encoder2_row(2, 32, 32),
    "tcn-hot": lambda: tcn_block_row(BF, 2, 5, 1024, 64, 64, 8, 2),
    "tcn-f32": lambda: tcn_block_row(F32, 2, 5, 64, 8, 8, 4, 1),
    "tcn-f32-proj": lambda: tcn_block_row(F32, 2, 5, 64, 8, 16, 4, 2),
    "film-fused-hot": lambda: film_fused_row(2, 5, 1024),
    "film-fused-ragged": lambda: film_fused_row(3, 1, 100),
    "decoder-mse-hot": lambda: decoder_mse_row(4096, 64, False),
    "decoder-mse-masked": lambda: decoder_mse_row(1000, 12, True),
    "vq-hot": lambda: vq_row(BF, 4096, 64, 64),
    "vq-f32": lambda: vq_row(F32, 333, 40, 12),
    "film-bf16": lambda: film_row(BF),
    "film-f32": lambda: film_row(F32),
    "edge-smooth-bf16": lambda: edge_smooth_row(BF),
    "edge-smooth-f32": lambda: edge_smooth_row(F32),
    "gate-blend-bf16": lambda: gate_blend_row(BF, 0.0),
    "gate-blend-f32-floor": lambda: gate_blend_row(F32, 0.55),
    "mse-bf16": lambda: mse_row(BF, False),
    "mse-f32-masked": lambda: mse_row(F32, True),
    "channel-scale-bf16": lambda: channel_scale_row(BF),
    "channel-scale-f32": lambda: channel_scale_row(F32),
    "gather": gather_row,
    "infonce-l2": lambda: infonce_row("l2"),
    "infonce-cosine": lambda: infonce_row("cosine"),
}


@pytest.mark.parametrize("name", list(ROWS))
def test_wrapper_gradient_contract_under_every_mask(name):
    _check_row(ROWS[name]())


@pytest.mark.parametrize("route", ["head-in-kernel", "headbwd-disabled"])
def test_tcn_chain_head_gradient_contract(route, monkeypatch):
    if route == "headbwd-disabled":
        monkeypatch.setenv("FRL_HIP_DISABLE", "headbwd")
    _check_row(chain_head_row(2, 1024, route == "head-in-kernel"))


# ---------------------------------------------------------------------------------------------------------------------------------
# partial upstream gradients (multi-output wrappers with set_materialize_grads(False))
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF])
def test_vq_partial_upstream_gradients_match_float64(dtype):
    from frl_hip import functional as Fh
    g = _gen(5)
    N, K, d = 1000, 40, 16
    z = torch.randn(N, d, generator=g).to(dtype)
    cb = torch.randn(K, d, generator=g)
    gzq = torch.randn(N, d, generator=g).to(dtype)
    for which in ("zq", "commit", "codebook"):
        zd = z.to(DEV).requires_grad_(True)
        cd = cb.to(DEV).requires_grad_(True)
        zq, lcb, lcm = Fh.VQFn.apply(zd, cd)[:3]
        out = {"zq": (zq, gzq.to(DEV)), "commit": (lcm, torch.tensor(0.7, device=DEV)), "codebook": (lcb, torch.tensor(1.9, device=DEV))}[which]
        torch.autograd.backward([out[0]], [out[1]])
        zr, cr = q(z, dtype).requires_grad_(True), cb.double().requires_grad_(True)
        e = (cr + (q(cb, dtype) - cb.double()))[Fh.VQFn.apply(z.to(DEV), cb.to(DEV))[4].long().cpu()]     # e_eff of test_vq_bwd_and_ema
        o = {"zq": zr + (e - zr).detach(), "commit": ((zr - e.detach()) ** 2).mean(), "codebook": ((zr.detach() - e) ** 2).mean()}[which]
        o.backward(out[1].double().cpu())
        for got, ref, n in ((zd.grad, zr.grad, "z"), (cd.grad, cr.grad, "codebook")):
            if ref is None or not ref.abs().max() > 0:
                assert got is None or not got.abs().max() > 0, (which, n)
            else:
                tol = 1e-4 if n == "codebook" else 1e-2 if dtype == BF else 1e-6       # test_vq_bwd_and_ema
                assert rel_err(got, ref) <= tol, (which, n, rel_err(got, ref))
    # the differentiable outputs are not views of the non-differentiable stats
    outs = Fh.VQFn.apply(z.to(DEV).requires_grad_(True), cb.to(DEV).requires_grad_(True))
    stats = outs[6]
    assert not stats.requires_grad and not outs[4].requires_grad and not outs[5].requires_grad
    for o in outs[1:4]:
        assert o.requires_grad and o.untyped_storage().data_ptr() != stats.untyped_storage().data_ptr()
    assert outs[1].item() == outs[2].item() == stats[3].item() and outs[3].item() == stats[1].item()


@pytest.mark.parametrize("dtype", [F32, BF])
def test_gate_blend_gate_only_upstream_matches_float64(dtype):
    from frl_hip import functional as Fh
    g = _gen(11)
    sm, res, graw = (torch.randn(4096, 64, generator=g).to(dtype) for _ in range(3))
    graw = torch.sigmoid(graw.float()).to(dtype)
    dg = torch.randn(4096, 64, generator=g).to(dtype)
    for min_gate in (0.0, 0.1):
        t = [v.to(DEV).requires_grad_(True) for v in (sm, res, graw)]
        out, gate = Fh.GateBlendFn.apply(*t, min_gate)
        gate.backward(dg.to(DEV))
        r = [q(v, dtype).requires_grad_(True) for v in (sm, res, graw)]
        gr = r[2].clamp(min=min_gate) if min_gate > 0 else r[2]
        gr.backward(dg.double())
        assert t[0].grad is None or not t[0].grad.abs().max() > 0
        assert t[1].grad is None or not t[1].grad.abs().max() > 0
        assert rel_err(t[2].grad, r[2].grad) <= (3e-2 if dtype == BF else 3e-6)


def _smooth_module(C, hidden, seed):
    from frl_hip.models.blocks import EdgeAwareSmoothingConv2D
    torch.manual_seed(seed)
    return EdgeAwareSmoothingConv2D(C, gate_hidden=hidden).to(DEV)


@pytest.mark.parametrize("which", ["out", "gate"])
def test_spatial_smoothing_partial_upstream_matches_the_modular_chain(which):
    """SpatialSmoothFn (f32, generic configuration) with the loss on one of its two outputs, against the modular chain of autograd nodes
    (SobelFn, conv3x3, conv1x1 heads, EdgeSmoothFn, GateBlendFn: each held against float64 by its own parity test), within the f32 bound
    of test_spatial_smoothing_block_as_one_autograd_node_matches_the_modular_chain (2e-5 of the largest gradient)."""
    m = _smooth_module(16, 24, 3)
    x = torch.randn(1, 9, 13, 16, generator=_gen(4)) * 0.7
    up = torch.randn(1, 9, 13, 16, generator=_gen(6)).to(DEV)
    res = {}
    for fuse in (True, False):
        m.fuse = fuse
        m.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        out, gate = m(xd, return_gate=True)
        ({"out": out, "gate": gate}[which]).backward(up)
        res[fuse] = (xd.grad.clone(), {n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()})
    (gxf, gf), (gxm, gm) = res[True], res[False]
    assert (gxf - gxm).abs().max().item() <= 2e-5 * gxm.abs().max().item()
    for n in gm:
        if gm[n] is None:
            assert gf[n] is None or not gf[n].abs().max() > 0, n
        else:
            assert (gf[n] - gm[n]).abs().max().item() <= 2e-5 * max(gm[n].abs().max().item(), 1e-6), n


@pytest.mark.parametrize("route", ["fused-heads", "modular", "generic-f32"])
def test_spatial_smoothing_gradient_contract_under_freezing(route, monkeypatch):
    """SpatialSmoothFn at the hot configuration (fused heads), with the heads on the modular kernels, and at a generic f32 configuration:
    each parameter frozen on its own, the input frozen; trainable gradients equal the all-trainable run bit for bit, with and without
    deferral."""
    if route == "modular":
        monkeypatch.setenv("FRL_HIP_DISABLE", "heads")
    shape, dt, m = ((2, 32, 32, 64), BF, _smooth_module(64, 64, 7)) if route != "generic-f32" else ((1, 9, 13, 16), F32, _smooth_module(16, 24, 7))
    m.fuse = True
    x = (torch.randn(*shape, generator=_gen(8)) * 0.7).to(dt).to(DEV)
    ups = [torch.randn(*shape, generator=_gen(s)).to(dt).to(DEV) for s in (9, 10)]
    names = [n for n, _ in m.named_parameters()]

    def run(trainable, defer):
        for n, p in m.named_parameters():
            p.grad = None
            p.requires_grad_(n in trainable)
        xd = x.clone().requires_grad_("x" in trainable)
        out, gate = m(xd, return_gate=True)
        ts = {"x": xd, **dict(m.named_parameters())}
        return _backward(ts, [out, gate], ups, defer)

    full = run(set(names) | {"x"}, False)
    masks = [{"x"} | set(names) - {n} for n in names] + [set(names), {"x"}]
    for n in names:
        if n.endswith(".weight") and n[:-6] + "bias" in names:
            masks.append({n[:-6] + "bias"})
    for mask in masks:
        a, b = run(mask, False), run(mask, True)
        for n in ["x"] + names:
            if n not in mask:
                assert a[n] is None and b[n] is None, (route, n)
            else:
                assert torch.equal(a[n], b[n]) and torch.equal(a[n], full[n]), (route, sorted(set(names) - mask), n)


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: freezing parts of the VQ-VAE
# ---------------------------------------------------------------------------------------------------------------------------------
FREEZES = {
    "phase_tcn.layers.0": lambda n: n.startswith("phase_tcn.layers.0."),
    "phase_film": lambda n: n.startswith("phase_film."),
    "gate_net": lambda n: n.startswith("spatial_conv.gate_net."),
    "type_encoder": lambda n: n.startswith("encoder."),
    "decoder_type.w0": lambda n: n == "decoder_type.layers.0.weight",
    "codebook": lambda n: n == "quant.codebook",
}


def _make_model():
    from frl_hip.models import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(64, 64, generator=_gen(7)))
    return m


def _freeze(m, frozen):
    for n, p in m.named_parameters():
        p.requires_grad_(not frozen(n))


def test_frozen_parts_of_the_full_width_model_leave_the_other_gradients_bitwise_unchanged():
    """bf16 full width (hot kernels): one forward_tiles + backward per frozen part, with deferral off and on; the trainable gradients
    equal the unfrozen run's bit for bit and frozen parameters get no gradient."""
    from frl_hip import ops
    tile = torch.randn(2, 5, 32, 32, 64, generator=_gen(13)).to(BF).to(DEV)

    def grads(frozen, defer):
        m = _make_model()
        _freeze(m, frozen)
        loss = m.forward_tiles(tile)["loss"]
        params = [p for p in m.parameters() if p.requires_grad]
        if defer:
            with ops.deferred_reductions(params):
                loss.backward()
        else:
            loss.backward()
        torch.cuda.synchronize()
        assert _lib().frl_defer_pending() == 0
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in m.named_parameters()}

    base = grads(lambda n: False, False)
    assert all(v is not None for v in base.values())
    for key, frozen in FREEZES.items():
        for defer in (False, True):
            got = grads(frozen, defer)
            for n, g in got.items():
                if frozen(n):
                    assert g is None, (key, defer, n)
                else:
                    assert g is not None and torch.equal(g, base[n]), (key, defer, n)


@pytest.mark.parametrize("key", ["phase_tcn.layers.0", "phase_film", "gate_net", "type_encoder", "decoder_type.w0", "codebook"])
def test_trainer_with_frozen_parameters_is_deferral_and_graph_invariant(key):
    """VQVAETrainer: three eager steps and three step_graphed steps, deferral on and off, end in equal parameters; the frozen ones are
    unchanged bit for bit."""
    from frl_hip.training.trainer import VQVAETrainer
    frozen = FREEZES[key]
    g = _gen(13)
    tiles = [torch.randn(2, 5, 32, 32, 64, generator=g).to(BF).to(DEV) for _ in range(3)]
    init = {n: p.detach().clone() for n, p in _make_model().named_parameters()}
    for graphed in (False, True):
        runs = []
        for defer in (False, True):
            m = _make_model()
            _freeze(m, frozen)
            tr = VQVAETrainer(m, lr=1e-3, total_steps=10, defer_reductions=defer)
            losses = [float((tr.step_graphed(t) if graphed else tr.step(t))["loss"].detach()) for t in tiles]
            torch.cuda.synchronize()
            assert _lib().frl_defer_pending() == 0
            assert all(np.isfinite(losses)), losses
            runs.append((m, losses))
        (m0, l0), (m1, l1) = runs
        assert l0 == l1, (key, graphed, l0, l1)
        for (n, p), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
            assert torch.equal(p, p1), (key, graphed, n)
            if frozen(n):
                assert torch.equal(p, init[n]), (key, graphed, n)


@pytest.mark.parametrize("case", ["conv1x1", "groupnorm-frozen-affine+bias-only-conv", "decoder-frozen-z"])
def test_gradient_accumulation_under_deferral_sums_or_raises(case):
    """A second backward into already populated .grad tensors inside deferred_reductions: the result is the sum of the two undeferred
    gradients, or the block raises (naming the .grad as invalid); never anything else.  The second and third cases put frozen tensors
    whose gradients are computed but never parked (GroupNorm's affine gradients, the decoder's dz) in the same backward: their freed
    addresses may come back for a parked gradient, which must not exempt that gradient from the check."""
    from frl_hip import functional as Fh, ops
    g = _gen(21)
    x = torch.randn(4096, 64, generator=g).to(BF).to(DEV)
    w0 = torch.randn(64, 64, generator=g) * 0.1
    b0 = torch.randn(64, generator=g) * 0.1
    gam = (torch.rand(64, generator=g) + 0.5).to(DEV)
    bet = (torch.randn(64, generator=g) * 0.2).to(DEV)
    dec = [t.to(DEV) for t in (torch.randn(128, 64, 1, 1, generator=g) / 8.0, torch.randn(128, generator=g) * 0.1,
                               torch.randn(64, 128, 1, 1, generator=g) / 128 ** 0.5)]
    target = torch.randn(4096, 64, generator=g).to(BF).to(DEV)
    dy1, dy2 = (torch.randn(4096, 64, generator=g).to(BF).to(DEV) for _ in range(2))

    def one(dy, w, b):
        if case == "conv1x1":
            Fh.conv1x1(x, w, b, 1).backward(dy)
        elif case.startswith("groupnorm"):                          # w frozen, GroupNorm affine frozen, only the conv bias trains
            Fh.conv1x1(Fh.group_norm(x.reshape(4, 1024, 64), gam, bet, 8), w.detach(), b, 0).backward(dy.reshape(4, 1024, 64))
        else:                                                        # decoder with a frozen input: the bias of its second layer trains
            scale = dy.float().mean()
            (Fh.decoder_mse(x, dec[0], dec[1], dec[2], b, target)[0] * scale).backward()

    w, b = w0.to(DEV).requires_grad_(True), b0.to(DEV).requires_grad_(True)
    params = [w, b] if case == "conv1x1" else [b]
    one(dy1, w, b)
    g1 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    one(dy2, w, b)
    g2 = [p.grad.clone() for p in params]
    for p, a in zip(params, g1):
        p.grad = a.clone()
    try:
        with ops.deferred_reductions(params):
            one(dy2, w, b)
    except RuntimeError as e:
        assert "deferred_reductions" in str(e) and "invalid" in str(e)
    else:
        torch.cuda.synchronize()
        for p, a, c in zip(params, g1, g2):
            assert torch.equal(p.grad, a + c)
    assert _lib().frl_defer_pending() == 0 and _lib().frl_defer_begin() == 0 and _lib().frl_defer_abort() == 0


@pytest.mark.parametrize("key", list(FREEZES))
def test_tiny_f32_model_with_frozen_parts_matches_the_oracle(key, golden_dir):
    """Tiny f32 fixture (generic kernels): after one forward_tiles + backward with a part frozen, the trainable gradients match
    frl_oracle.vqvae_loss_and_grads (recorded in the fixture: freezing does not change the other gradients)."""
    import os
    from frl_hip.models import VQVAE
    fx = np.load(os.path.join(golden_dir, "vqvae_tiny_seed0.npz"))
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, beta=0.25, hidden=16, z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4, compute_dtype=torch.float32).to(DEV)
    res = m.load_state_dict({k[6:]: torch.from_numpy(fx[k]).float() for k in fx.files if k.startswith("state.")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    frozen = FREEZES[key]
    _freeze(m, frozen)
    assert any(frozen(n) for n, _ in m.named_parameters())
    m.train()
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    m.forward_tiles(tiles[0])["loss"].backward()
    for n, p in m.named_parameters():
        if frozen(n):
            assert p.grad is None, n
        else:
            ref = fx["grad." + n]
            err = float(np.abs(p.grad.detach().double().cpu().numpy() - ref).max())
            assert err <= 1e-6 + 2e-4 * np.abs(ref).max(), (key, n, err)
