"""GPU tests of the merged 3x3 weight gradient (frl_conv3x3_bwd_weight_multi: csrc/conv3x3.hip, csrc/conv3x3_wgrad.hip): up to four jobs
over images of one shape in ONE launch of the band kernel, the workgroups divided between the jobs (frl_hip/wgrad_split.py).

Exact tier: the integer data of tests/conv3x3_cases.py, on which float32 accumulation is exact in any order, so torch.equal against the
float64 reference is a real check of the merged route, whose workgroups chain several units of tiles across images; the same results must
come from the job-by-job route (hook off) and from the single calls.  Bit tier: on random data, where the order of the float32 adds
matters, the merged call must still give the single calls' bits (the chains of the slab reduction, tests/test_cpu_wgrad_split.py), with
immediate and with deferred reductions.  Tolerance tier: random data against float64 with the bf16 weight-gradient ceiling of
test_gpu_conv3x3_routes.py.  Node level: SpatialSmoothFn with and without the merged call, bit for bit (one tile per workgroup
under both routes), with deferred reductions and frozen parameters."""
import contextlib
import functools

import pytest
import torch

import conv3x3_cases as C
from frl_hip import wgrad_split as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
WTOL = 3e-2          # MODES["bf16"][1] of test_gpu_conv3x3_routes.py: weight gradients relative to max|ref|


@functools.lru_cache(maxsize=None)
def _exact(B, H, W, cin):
    """Integer inputs on the device and float64 results of one (shape, Cin -> 64) layer, computed once for all tests."""
    inp, exp = C.wgrad_exact(C.WgradCase(B, H, W, cin, 64))
    return {k: v.to(BF).to(DEV).contiguous() for k, v in inp.items()}, exp


@contextlib.contextmanager
def multi_hook(on):
    from frl_hip import ops
    was = ops.conv3x3_wgrad_multi(on)
    try:
        yield
    finally:
        ops.conv3x3_wgrad_multi(was)


def _jobs(shape, spec):
    """spec: [(Cin, mask, want_weight, want_bias), ...] -> (jobs for ops.conv3x3_bwd_weight_multi, expected [(dw, db), ...])."""
    from frl_hip import ops
    jobs, want = [], []
    for cin, mask, ww, wb in spec:
        inp, exp = _exact(*shape, cin)
        y, act = (inp["y_relu_mask"], ops.ACT_RELU) if mask == "relu" else (None, ops.ACT_NONE)
        jobs.append((inp["dy"], inp["x"], y, act, ww, wb))
        want.append((exp[f"dw_{mask}"] if ww else None, exp[f"db_{mask}"] if wb else None))
    return jobs, want


def _launches(fn):
    """-> (result of fn(), {kernel name: launches} of the 3x3 weight-gradient kernels fn() issued)."""
    from frl_hip import ops
    ops.kernel_timing(True)
    try:
        ops.kernel_timing_report()
        out = fn()
        rep = ops.kernel_timing_report()
    finally:
        ops.kernel_timing(False)
    return out, {k: c for k, (c, _) in rep.items() if "conv3x3_wgrad" in k}


THREE = [(64, "none", True, True), (64, "relu", True, True), (128, "relu", True, True)]
EXACT = [
    pytest.param((100, 24, 32), THREE, id="3jobs-100x24x32"),        # 300 bands per job: units of 2 tiles, 150 busy; 64 workgroups per chunk chain 3 or 2 of them across images
    pytest.param((2, 24, 96), THREE, id="3jobs-2x24x96"),            # 18 bands per job: one tile per workgroup, 3 bands per image row
    pytest.param((1, 8, 32), THREE, id="3jobs-1x8x32"),              # one tile per job
    pytest.param((100, 24, 32), [(64, "relu", True, True), (128, "none", True, False)], id="2jobs-mask-nobias-100x24x32"),
    pytest.param((100, 24, 32), [(128, "relu", True, True)], id="1job-100x24x32"),
    pytest.param((2, 24, 96), [(64, "none", False, True), (64, "relu", True, True)], id="2jobs-bias-only-2x24x96"),
]


@pytest.mark.parametrize("shape,spec", EXACT)
def test_merged_weight_gradients_are_exact_on_integer_data(shape, spec):
    from frl_hip import ops
    jobs, want = _jobs(shape, spec)
    assert ops.conv3x3_wgrad_multi_supported(jobs)
    with multi_hook(True):
        got, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    assert seen == {"conv3x3_wgrad_multi_kernel": 1}, seen
    with multi_hook(False):
        serial, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    assert seen == {"conv3x3_wgrad_kernel": len(jobs)}, seen
    single = [ops.conv3x3_bwd_weight(dy, x, y, act, want_bias=wb) for dy, x, y, act, _, wb in jobs]
    torch.cuda.synchronize()
    bad = []
    for j, ((dw, db), (dws, dbs), (dw1, db1), (edw, edb)) in enumerate(zip(got, serial, single, want)):
        for nm, g, s, one, e in (("dw", dw, dws, dw1, edw), ("db", db, dbs, db1, edb)):
            if e is None:
                assert g is None and s is None
                continue
            for route, t in (("merged", g), ("job by job", s), ("single call", one)):
                if not torch.equal(t.cpu(), e):
                    n = (t.cpu() != e).sum().item()
                    bad.append(f"job {j} {nm} {route}: {n} of {e.numel()} values differ from float64")
    assert not bad, f"{shape} {S.split(*shape, [c for c, *_ in spec])}:\n" + "\n".join(bad)


def test_merged_weight_gradients_match_float64_on_random_data():
    from frl_hip import ops
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(20)
    jobs, refs = [], []
    for cin, act in ((64, ops.ACT_SIGMOID), (64, ops.ACT_RELU), (128, ops.ACT_NONE)):
        x = torch.randn(B, H, W, cin, generator=g).to(BF)
        dy = torch.randn(B, H, W, 64, generator=g).to(BF)
        y = {ops.ACT_SIGMOID: torch.sigmoid(torch.randn(B, H, W, 64, generator=g)), ops.ACT_RELU: torch.randn(B, H, W, 64, generator=g).clamp(min=0),
             ops.ACT_NONE: None}[act]
        y = None if y is None else y.to(BF)
        # the kernel rounds dy .* act'(y) to bf16 before the contraction: the float64 reference takes the unrounded product, the ceiling covers it
        d = dy.double() * {ops.ACT_SIGMOID: lambda t: t * (1 - t), ops.ACT_RELU: lambda t: (t > 0).double(), ops.ACT_NONE: lambda t: 1.0}[act](
            None if y is None else y.double())
        refs.append((torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (64, cin, 3, 3), d.permute(0, 3, 1, 2), padding=1), d.sum(dim=(0, 1, 2))))
        jobs.append((dy.to(DEV), x.to(DEV), None if y is None else y.to(DEV), act, True, True))
    with multi_hook(True):
        got, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    torch.cuda.synchronize()
    assert seen == {"conv3x3_wgrad_multi_kernel": 1}, seen
    bad = {}
    for j, ((dw, db), (rw, rb)) in enumerate(zip(got, refs)):
        for nm, t, r in (("dw", dw, rw), ("db", db, rb)):
            e = (t.cpu().double() - r).abs().max().item() / max(r.abs().max().item(), 1e-6)
            print(f"conv3x3 merged wgrad tolerance tier job {j} {nm}: {e:.3e} (ceiling {WTOL:.1e})")
            if not e <= WTOL:
                bad[(j, nm)] = e
    assert not bad, bad


@pytest.mark.parametrize("shape", [(300, 8, 32), (128, 16, 64), (257, 8, 32)], ids=lambda s: "x".join(map(str, s)))
def test_merged_weight_gradients_keep_the_single_calls_bits_on_random_data(shape):
    """300 tiles: units of 2, chains of 3 and 2 busy units; 512 tiles: units of 2, every chain full; 257 tiles: units of 2, 129 busy, the
    last of one tile.  Random bf16 data: any other order of the float32 adds changes bits."""
    from frl_hip import ops
    B, H, W = shape
    g = torch.Generator().manual_seed(30 + B)
    jobs = []
    for cin, act in ((64, ops.ACT_NONE), (64, ops.ACT_SIGMOID), (128, ops.ACT_NONE)):
        x = torch.randn(B, H, W, cin, generator=g).to(BF).to(DEV)
        dy = torch.randn(B, H, W, 64, generator=g).to(BF).to(DEV)
        y = torch.sigmoid(torch.randn(B, H, W, 64, generator=g)).to(BF).to(DEV) if act else None
        jobs.append((dy, x, y, act, True, True))
    assert [j["nunits"] for j in S.split(B, H, W, [64, 64, 128])] == [4, 4, 4]
    with multi_hook(True):
        got, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    assert seen == {"conv3x3_wgrad_multi_kernel": 1}, seen
    # the same call with its three reductions parked and run by the one deferred launch (slab_reduce_jobs_kernel at 64 slabs per job),
    # as the train step runs it; the gradients go to no parameter here, so they are handed to ops.discard
    from frl_hip import _lib
    with multi_hook(True):
        with ops.deferred_reductions([]):
            parked = ops.conv3x3_bwd_weight_multi(jobs)
            assert _lib.load().frl_defer_pending() == len(jobs)
            for dw, db in parked:
                ops.discard(dw, db)
    single = [ops.conv3x3_bwd_weight(dy, x, y, act) for dy, x, y, act, _, _ in jobs]
    torch.cuda.synchronize()
    for route, res in (("immediate", got), ("deferred", parked)):
        for j, ((dw, db), (dw1, db1)) in enumerate(zip(res, single)):
            assert dw1.abs().max() > 0 and torch.equal(dw, dw1), (route, j, (dw != dw1).sum().item(), dw.numel())
            assert torch.equal(db, db1), (route, j, (db != db1).sum().item())


def test_shapes_without_a_bit_exact_split_run_job_by_job():
    """100 tiles per job: three jobs do not fit 256 workgroups together and the single call has no 256 slabs to chain."""
    from frl_hip import ops
    g = torch.Generator().manual_seed(22)
    jobs = [(torch.randn(100, 8, 32, 64, generator=g).to(BF).to(DEV), torch.randn(100, 8, 32, c, generator=g).to(BF).to(DEV), None, ops.ACT_NONE, True, True)
            for c in (64, 64, 128)]
    assert not ops.conv3x3_wgrad_multi_supported(jobs)
    got, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    assert seen == {"conv3x3_wgrad_kernel": 3}, seen
    for (dw, db), (dy, x, y, act, _, _) in zip(got, jobs):
        dw1, db1 = ops.conv3x3_bwd_weight(dy, x, y, act)
        assert torch.equal(dw, dw1) and torch.equal(db, db1)


def test_jobs_the_band_kernel_does_not_take_run_job_by_job():
    """float32 jobs and a ragged shape are no case for the merged launch: the call runs them through the single-call route, same bits."""
    from frl_hip import ops
    g = torch.Generator().manual_seed(21)
    jobs = []
    for cin, cout in ((12, 8), (20, 6)):
        jobs.append((torch.randn(2, 9, 11, cout, generator=g).to(DEV), torch.randn(2, 9, 11, cin, generator=g).to(DEV), None, ops.ACT_NONE, True, True))
    assert not ops.conv3x3_wgrad_multi_supported(jobs)
    got, seen = _launches(lambda: ops.conv3x3_bwd_weight_multi(jobs))
    assert seen == {"conv3x3_wgrad_kernel": 2}, seen
    for (dw, db), (dy, x, y, act, _, _) in zip(got, jobs):
        dw1, db1 = ops.conv3x3_bwd_weight(dy, x, y, act)
        assert torch.equal(dw, dw1) and torch.equal(db, db1)


def test_hook_returns_and_restores_the_setting():
    from frl_hip import _lib
    lib = _lib.load()
    was = lib.frl_conv3x3_wgrad_multi(0)
    try:
        assert was == 1 and lib.frl_conv3x3_wgrad_multi(1) == 0 and lib.frl_conv3x3_wgrad_multi(1) == 1
    finally:
        lib.frl_conv3x3_wgrad_multi(was)
    assert lib.frl_conv3x3_wgrad_multi(was) == was


def test_workspace_follows_the_split():
    import ctypes
    from frl_hip import _lib, ops
    lib = _lib.load()
    cin, cout = (ctypes.c_int * 3)(64, 64, 128), (ctypes.c_int * 3)(64, 64, 64)
    for shape in ((256, 32, 32), (100, 24, 32), (2, 24, 96)):
        assert lib.frl_conv3x3_bwd_weight_multi_workspace_bytes(3, *shape, cin, cout, ops.BF16) == S.workspace_bytes(*shape, [64, 64, 128]), shape
    with multi_hook(False):
        assert lib.frl_conv3x3_bwd_weight_multi_workspace_bytes(3, 256, 32, 32, cin, cout, ops.BF16) == \
            sum(lib.frl_conv3x3_bwd_weight_workspace_bytes(256, 32, 32, c, 64) for c in (64, 64, 128))


# ----------------------------------------------------------------------------------------------------------------------------------
# Node level: SpatialSmoothFn
# ----------------------------------------------------------------------------------------------------------------------------------
FROZEN = {"none": (), "gate_net.0": ("gate_net.0.weight", "gate_net.0.bias"), "mix_backbone.0.bias": ("mix_backbone.0.bias",),
          "gate_net.2.weight": ("gate_net.2.weight",)}


@pytest.mark.parametrize("frozen", list(FROZEN))
def test_smoothing_block_gradients_do_not_depend_on_the_merged_call(frozen, monkeypatch):
    """EdgeAwareSmoothingConv2D(64, gate_hidden=64), bf16, (2, 32, 32, 64): 8 tiles per job, one per workgroup under both routes, so dx and
    all ten parameter gradients are bit-equal with FRL_HIP_DISABLE=wgradmulti and without, with deferred reductions on and off; a frozen
    parameter has no gradient under either."""
    from frl_hip import ops
    from frl_hip.models.blocks import EdgeAwareSmoothingConv2D
    torch.manual_seed(11)
    m = EdgeAwareSmoothingConv2D(64, gate_hidden=64).to(DEV)
    m.fuse = True
    names = [n for n, _ in m.named_parameters()]
    assert len(names) == 10 and all(n in names for n in FROZEN[frozen])
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(2, 32, 32, 64, generator=g) * 0.7).to(BF).to(DEV)
    ups = [torch.randn(2, 32, 32, 64, generator=g).to(BF).to(DEV) for _ in range(2)]

    def run(defer):
        for n, p in m.named_parameters():
            p.grad = None
            p.requires_grad_(n not in FROZEN[frozen])
        xd = x.clone().requires_grad_(True)
        out, gate = m(xd, return_gate=True)
        params = [p for p in m.parameters() if p.requires_grad] + [xd]

        def back():
            if defer:
                with ops.deferred_reductions(params):
                    torch.autograd.backward([out, gate], ups)
            else:
                torch.autograd.backward([out, gate], ups)
        _, seen = _launches(back)
        torch.cuda.synchronize()
        return {"x": xd.grad.clone(), **{n: None if p.grad is None else p.grad.clone() for n, p in m.named_parameters()}}, seen

    res = {}
    for route in ("merged", "separate"):
        if route == "separate":
            monkeypatch.setenv("FRL_HIP_DISABLE", "wgradmulti")
        for defer in (False, True):
            res[route, defer], seen = run(defer)
            live = 3 - (frozen == "gate_net.0")
            assert seen == ({"conv3x3_wgrad_multi_kernel": 1} if route == "merged" else {"conv3x3_wgrad_kernel": live}), (route, seen)
    base = res["separate", False]
    for n in ["x"] + names:
        if n in FROZEN[frozen]:
            assert all(r[n] is None for r in res.values()), n
        else:
            assert base[n] is not None and all(torch.equal(r[n], base[n]) for r in res.values()), (frozen, n)
