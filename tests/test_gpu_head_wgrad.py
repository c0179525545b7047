"""The streaming weight-gradient kernel for thin bf16 outputs (csrc/pw_wgrad_thin.hip: the 64 -> 12 phase head) against the generic
pw_wgrad_kernel it replaces: same workgroups, same row order, same MFMA operand sequence, so dW and db are equal BIT FOR BIT
(frl_wgrad_thin(1) against frl_wgrad_thin(0)); against float64 at the bound test_conv1x1_bwd applies to this operation; routing; and
the whole model, eager, deferred and graph-captured.

Shapes: the ring of the kernel is 4 tiles deep, so with the workgroup bound at 64 the cases P = 64 * 64 * k give every workgroup k tiles:
the ring under-filled (k < 3), exactly primed (3), exactly filled (4), wrapped once (5, 7) and several times (9, 12); the same cases
cover any depth up to 8.  (The largest input is 49 152 x 76 bf16 elements, 7.5 MB.)"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
CIN = 64

# (P, Cout, workgroup bound or None for the default of 512, want_bias)
CASES = ([(64, 12, None, True), (192, 12, None, True)]
         + [(64 * 64 * k, 12, 64, True) for k in (1, 2, 3, 4, 5, 7, 9, 12)]
         + [(64 * 197, 12, 64, True),       # 49 workgroups of 4 tiles, one of 1 tile, 14 with none (zero slabs)
            (64 * 513, 12, None, True)]     # workgroups of 2 tiles, one of 1, the rest empty
         + [(64 * 64 * 3, co, 64, True) for co in (4, 8, 16)]
         + [(64 * 64 * 3, 12, 64, False)])


def _ids(c):
    return f"P{c[0]}-co{c[1]}-wgs{c[2]}-bias{int(c[3])}"


class _hooks:
    """Sets frl_wgrad_thin / frl_wgrad_set_max_workgroups for a block and puts the previous settings back."""

    def __init__(self, thin=None, max_wgs=None):
        self.thin, self.max_wgs = thin, max_wgs

    def __enter__(self):
        from frl_hip import _lib, ops
        self.was_thin = ops.wgrad_thin(self.thin) if self.thin is not None else None
        self.was_wgs = _lib.load().frl_wgrad_set_max_workgroups(self.max_wgs) if self.max_wgs is not None else None
        return self

    def __exit__(self, *exc):
        from frl_hip import _lib, ops
        if self.was_wgs is not None:
            _lib.load().frl_wgrad_set_max_workgroups(self.was_wgs)
        if self.was_thin is not None:
            ops.wgrad_thin(self.was_thin)
        return False


def _inputs(P, cout, cin=CIN, seed=None):
    g = torch.Generator().manual_seed(P * 3 + cin + cout if seed is None else seed)
    x = torch.randn(P, cin, generator=g).to(BF)
    dy = torch.randn(P, cout, generator=g).to(BF)
    return dy, x


@functools.lru_cache(maxsize=None)
def _case(P, cout, max_wgs, want_bias):
    """(dw, db) of the generic and of the thin route and the float64 reference of one case; computed once, left unchanged by its users."""
    from frl_hip import ops
    dy, x = _inputs(P, cout)
    dyd, xd = dy.to(DEV), x.to(DEV)
    res = {}
    for thin in (False, True):
        with _hooks(thin=thin, max_wgs=max_wgs):
            dw, db = ops.conv1x1_bwd_weight(dyd, xd, None, 0, want_bias=want_bias)
            torch.cuda.synchronize()
        res[thin] = (dw.cpu(), None if db is None else db.cpu())
    return res[False], res[True], (dy.double().t() @ x.double(), dy.double().sum(0))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_thin_route_equals_the_generic_route_bit_for_bit(case):
    (dw0, db0), (dw1, db1), _ = _case(*case)
    assert torch.equal(dw1, dw0)
    if case[3]:
        assert torch.equal(db1, db0)
    else:
        assert db0 is None and db1 is None


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_thin_route_against_float64(case):
    """8e-5 * max(|ref|, 1), the bound of test_conv1x1_bwd: a float32 chain of 32-row steps without any workgroup split stays below
    1.2e-6 relative at these sizes."""
    _, (dw, db), (ref_dw, ref_db) = _case(*case)
    err = (dw.double() - ref_dw).abs().max().item()
    print(f"dw err {err:.3e} of {ref_dw.abs().max().item():.3e}")
    assert err <= 8e-5 * max(ref_dw.abs().max().item(), 1.0)
    if case[3]:
        err = (db.double() - ref_db).abs().max().item()
        print(f"db err {err:.3e} of {ref_db.abs().max().item():.3e}")
        assert err <= 8e-5 * max(ref_db.abs().max().item(), 1.0)


def _kernels_of(fn):
    """Names of the library kernels that fn() launched."""
    from frl_hip import ops
    ops.kernel_timing(True)
    try:
        ops.kernel_timing_report()
        out = fn()
        torch.cuda.synchronize()
        return out, set(ops.kernel_timing_report())
    finally:
        ops.kernel_timing(False)


def _ran(names, kernel):
    return any(n == kernel or n.startswith(kernel + "<") for n in names)


def test_eligible_call_takes_the_thin_kernel_and_the_hook_turns_it_off():
    from frl_hip import ops
    dy, x = _inputs(640, 12)
    dyd, xd = dy.to(DEV), x.to(DEV)
    with _hooks(thin=True):
        _, names = _kernels_of(lambda: ops.conv1x1_bwd_weight(dyd, xd, None, 0))
    assert _ran(names, "pw_wgrad_thin_kernel") and not _ran(names, "pw_wgrad_kernel"), names
    with _hooks(thin=False):
        _, names = _kernels_of(lambda: ops.conv1x1_bwd_weight(dyd, xd, None, 0))
    assert _ran(names, "pw_wgrad_kernel") and not _ran(names, "pw_wgrad_thin_kernel"), names
    with _hooks(thin=True) as h:
        assert h.was_thin is True, "the default is on"


def _fallback_call(kind):
    from frl_hip import ops
    if kind == "ragged-P":
        dy, x = _inputs(1000, 12)
        args, kw = (dy.to(DEV), x.to(DEV), None, 0), {}
    elif kind == "Cin32":
        dy, x = _inputs(640, 12, cin=32)
        args, kw = (dy.to(DEV), x.to(DEV), None, 0), {}
    elif kind == "mask":
        dy, x = _inputs(640, 12)
        y = torch.randn(640, 12, generator=torch.Generator().manual_seed(5)).to(BF)
        args, kw = (dy.to(DEV), x.to(DEV), y.to(DEV), 1), {}
    elif kind == "scalar-frags":
        dy, x = _inputs(640, 12)
        args, kw = (dy.to(DEV), x.to(DEV), None, 0), {"scalar_frags": True}
    else:                                                     # dy one 24-byte row into a larger buffer: 8-byte aligned only
        dy, x = _inputs(641, 12)
        buf = dy.to(DEV).reshape(-1)
        view = buf[12:].view(640, 12)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        args, kw = (view, x[1:].contiguous().to(DEV), None, 0), {}
    return lambda: ops.conv1x1_bwd_weight(*args, **kw)


@pytest.mark.parametrize("kind", ["ragged-P", "Cin32", "mask", "scalar-frags", "dy-8-byte-aligned"])
def test_ineligible_calls_keep_the_generic_kernel(kind):
    call = _fallback_call(kind)
    res = {}
    for thin in (True, False):
        with _hooks(thin=thin):
            (dw, db), names = _kernels_of(call)
        assert _ran(names, "pw_wgrad_kernel") and not _ran(names, "pw_wgrad_thin_kernel"), (thin, names)
        res[thin] = (dw.cpu(), db.cpu())
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


# ---- in the model: 2 tiles of 5 x 8 x 8 x 64 -> R = 640 phase rows, ten 64-row tiles ----
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _model():
    from frl_hip.models import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=32, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=BF).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(32, 64, generator=_gen(7)))
    return m


def _tiles(n):
    g = _gen(13)
    return [torch.randn(2, 5, 8, 8, 64, generator=g).to(BF).to(DEV) for _ in range(n)]


def _same(a, b):
    if a.dtype == BF:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


def test_model_step_is_the_same_with_the_hook_on_and_off():
    runs = {}
    for thin in (False, True):
        m, tile = _model(), _tiles(1)[0]

        def step():
            out = m.forward_tiles(tile)
            out["loss"].backward()
            return out

        with _hooks(thin=thin):
            out, names = _kernels_of(step)
        assert _ran(names, "pw_wgrad_thin_kernel") == thin, names    # the head's gradient is the eligible call of the step
        runs[thin] = ({k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)},
                      {n: p.grad.clone() for n, p in m.named_parameters()})
    (o0, g0), (o1, g1) = runs[False], runs[True]
    assert set(o0) == set(o1) and set(g0) == set(g1)
    for k in o0:
        assert _same(o1[k], o0[k]), k
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n


def test_deferred_and_graphed_steps_with_the_thin_kernel_equal_eager_steps_without():
    from frl_hip.training.trainer import VQVAETrainer
    tiles = _tiles(3)
    runs = {}
    for name, (thin, graphed) in {"generic-eager": (False, False), "thin-eager": (True, False), "thin-graphed": (True, True)}.items():
        with _hooks(thin=thin):
            m = _model()
            tr = VQVAETrainer(m, lr=1e-3, total_steps=10, defer_reductions=True)
            losses = [float((tr.step_graphed(t) if graphed else tr.step(t))["loss"].detach()) for t in tiles]
            torch.cuda.synchronize()
            if graphed:
                assert tr.graph_supported()
        runs[name] = (m, losses)
    for other in ("thin-eager", "thin-graphed"):
        assert runs["generic-eager"][1] == runs[other][1], other
        for (n, p), (_, p1) in zip(runs["generic-eager"][0].named_parameters(), runs[other][0].named_parameters()):
            assert torch.equal(p, p1), (other, n)
