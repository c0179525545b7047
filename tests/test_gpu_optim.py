"""Fused clip + AdamW (csrc/optim.hip through frl_hip.training.optim.HipAdamW) and frl_multi_tensor_scale_copy against the float64
runner of tests/optim_cases.py: every element of the parameters AND of both moments, after every step of a schedule that reaches the
later descriptor-table batches, the grid-stride loop, the strided re-sum of the partials, device-skipped steps (ok = 0, -1, NaN), tensors
without a gradient, the device learning rate, checkpoints, a captured step and the 576-tensor limit.

Tolerance: GPU_MARGIN (2) x what float32 torch.optim.AdamW itself loses against float64 on the same schedule (measured on the CPU by
tests/test_cpu_optim_cases.py, pinned in optim_cases.py)."""
import ctypes
import functools
import struct

import pytest
import torch

import optim_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WRONG_LR = 0.5                                            # host learning rate of the runs that supply the real one through lr_dev


@functools.lru_cache(maxsize=None)
def _case(name):
    return C.full_case() if name == "full" else C.graph_case()


@functools.lru_cache(maxsize=None)
def _grads(name, step):
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return tuple(None if g is None else g.to(DEV) for g in _case(name).grads(step))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 runner, once per schedule: per step (params, exp_avg, exp_avg_sq) as flat float64 tensors (shared between steps that change
    nothing), torch's per-parameter steps and the float64 gradient norm."""
    case, out, flats = _case(name), [], None
    for snap in C.run_torch(case):
        ev = case.events[snap.step]
        if flats is None or (ev.applied and len(ev.absent) < len(case.numels)):
            flats = (C.flat64(snap.params), C.flat64(snap.exp_avg), C.flat64(snap.exp_avg_sq))
        out.append(dict(flats=flats, steps=snap.steps, norm=snap.norm))
    return out


def _make(case, params=None, lr_dev=False):
    from frl_hip.training.optim import HipAdamW
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in (case.params if params is None else params)]
    opt = HipAdamW([{"params": [p], "weight_decay": wd} for p, wd in zip(params, case.wds)], lr=WRONG_LR, betas=C.BETAS, eps=C.EPS)
    if lr_dev:
        opt.lr_dev = torch.zeros(1, dtype=torch.float32, device=DEV)
    return opt


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


def _state(opt):
    return _flat(opt.params), _flat(opt.exp_avg), _flat(opt.exp_avg_sq)


def _same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _sd_steps(opt):
    st = opt.state_dict()["state"]
    return [int(float(st[i]["step"])) for i in range(len(opt.params))]


def _step(opt, name, s, grads=None):
    """Event s of the schedule through HipAdamW.step: the learning rate goes through lr_dev when the optimizer has one (the host value
    then stays wrong), else through param_groups."""
    ev = _case(name).events[s]
    if opt.lr_dev is not None:
        opt.lr_dev.fill_(ev.lr)
    else:
        for g in opt.param_groups:
            g["lr"] = ev.lr
    ok = torch.tensor([ev.ok], dtype=torch.float32, device=DEV)
    return opt.step(ev.max_norm, grads=list(_grads(name, s)) if grads is None else grads, ok=ok)


@functools.lru_cache(maxsize=None)
def _gpu_run(name, lr_dev=False):
    """The whole schedule on the GPU, once: per step the flat state, the returned norm, the device counters and the checkpoint's steps."""
    opt, out = _make(_case(name), lr_dev=lr_dev), []
    for s in range(len(_case(name).events)):
        norm = _step(opt, name, s)
        out.append(dict(state=_state(opt), norm=float(norm.item()), counters=opt.applied_and_skipped, steps=_sd_steps(opt)))
    return out


def _deviation(state, ref, numels):
    p, m, v = (t.to("cpu", torch.float64) for t in state)
    return C.param_dev_u(p, ref[0]), C.moment_dev_rel(m, ref[1], numels), C.moment_dev_rel(v, ref[2], numels)


def test_trajectory_matches_float64_after_every_step():
    """Expected to fail on a count kept as `counters[0] - lag` with a host-side lag: tensors without a gradient on the skipped step 0
    then take their first update with update number 0 (lr / (1 - beta1^0) = inf)."""
    case, run, ref = _case("full"), _gpu_run("full"), _reference("full")
    tol = (C.GPU_MARGIN * C.F32_PARAM_DEV_U, C.GPU_MARGIN * C.F32_M_DEV_REL, C.GPU_MARGIN * C.F32_V_DEV_REL)
    start = tuple(t.to(DEV) for t in (torch.cat(case.params), torch.zeros(sum(case.numels)), torch.zeros(sum(case.numels))))
    worst = [0.0, 0.0, 0.0]
    for s, ev in enumerate(case.events):
        before = run[s - 1]["state"] if s else start
        state = run[s]["state"]
        assert all(bool(torch.isfinite(t).all()) for t in state), f"step {s}: non-finite parameters or moments"
        if not ev.applied or len(ev.absent) == len(case.numels):
            assert _same_bits(state, before), f"step {s} (ok = {ev.ok}) changed parameters or moments"
        assert run[s]["counters"] == case.expected_counters(s + 1), f"step {s}: (applied, skipped)"
        dev = _deviation(state, ref[s]["flats"], case.numels)
        print(f"step {s}: parameters {dev[0]:.3f} u, exp_avg {dev[1]:.3e}, exp_avg_sq {dev[2]:.3e}   (limits {tol[0]:.1f} u, {tol[1]:.1e}, {tol[2]:.1e})")
        worst = [max(w, d) for w, d in zip(worst, dev)]
    assert worst[0] <= tol[0] and worst[1] <= tol[1] and worst[2] <= tol[2], (worst, tol)


def test_returned_norm_matches_float64():
    """Each thread sums at most 16 fma terms per chunk in float32 before the float64 reduction: 16 * 2^-24 relative on the sum of squares,
    half of it on the root, plus one float32 cast -- 1e-6 covers it."""
    case, run, ref = _case("full"), _gpu_run("full"), _reference("full")
    checked = 0
    for s, ev in enumerate(case.events):
        if ev.applied and len(ev.absent) < len(case.numels):
            print(f"step {s}: norm {run[s]['norm']!r}, float64 {ref[s]['norm']!r}, relative {abs(run[s]['norm'] - ref[s]['norm']) / ref[s]['norm']:.2e}")
            assert abs(run[s]["norm"] - ref[s]["norm"]) <= 1e-6 * ref[s]["norm"], s
            checked += 1
    assert checked == 6


def test_device_learning_rate_gives_the_same_bits():
    """lr_dev is the only source of the learning rate when it is set: the host value (left wrong on purpose) must not leak in."""
    host, dev = _gpu_run("full"), _gpu_run("full", True)
    for s, (a, b) in enumerate(zip(host, dev)):
        assert _same_bits(a["state"], b["state"]), f"step {s}"
        assert a["norm"] == b["norm"] and a["counters"] == b["counters"] and a["steps"] == b["steps"]


def test_checkpoint_steps_are_per_tensor_and_resume_is_exact():
    case, name, run, ref = _case("full"), "full", _gpu_run("full"), _reference("full")
    for s in range(len(case.events)):
        assert run[s]["steps"] == ref[s]["steps"] == case.expected_steps(s + 1), f"state_dict steps after step {s}"
    forks = {}
    opt = _make(case)
    for s in range(len(case.events)):
        _step(opt, name, s)
        if s in (0, 4, 5, 7):                              # right after each skipped step (0, 4, 7), and after an applied one
            sd = opt.state_dict()
            sd["state"] = {i: {k: v.clone() for k, v in st.items()} for i, st in sd["state"].items()}
            forks[s] = (sd, [p.detach().clone() for p in opt.params])
    assert _same_bits(_state(opt), run[-1]["state"])       # the kernels are deterministic: same schedule, same bits
    for at, (sd, params) in forks.items():
        resumed = _make(case, params=params)
        resumed.load_state_dict(sd)
        assert _sd_steps(resumed) == ref[at]["steps"]
        for s in range(at + 1, len(case.events)):
            _step(resumed, name, s)
            assert _same_bits(_state(resumed), run[s]["state"]), f"resumed after step {at}: differs at step {s}"
        assert _sd_steps(resumed) == ref[-1]["steps"]


def test_captured_step_counts_updates_on_the_device():
    """One HipAdamW.step captured as a linear graph (static gradient buffers, ok and lr as device words), two tensors outside its table.
    Replays run no Python: only a count kept on the device knows how many updates the table's tensors took and the two others did not.
    Expected to fail on a host-side lag: the eager step then gives the two tensors update number 2 instead of 1."""
    case, name, ref = _case("graph"), "graph", _reference("graph")
    tol = (C.GPU_MARGIN * C.GRAPH_F32_PARAM_DEV_U, C.GPU_MARGIN * C.GRAPH_F32_M_DEV_REL, C.GPU_MARGIN * C.GRAPH_F32_V_DEV_REL)
    opt = _make(case, lr_dev=True)
    ok = torch.zeros(1, dtype=torch.float32, device=DEV)
    static = [None if i in C.GRAPH_ABSENT else torch.zeros(n, device=DEV) for i, n in enumerate(case.numels)]

    def load(s):
        for buf, g in zip(static, _grads(name, s)):
            assert (buf is None) == (g is None)
            if buf is not None:
                buf.copy_(g)
        ok.fill_(case.events[s].ok)
        opt.lr_dev.fill_(case.events[s].lr)

    def check(s):
        dev = _deviation(_state(opt), ref[s]["flats"], case.numels)
        print(f"event {s}: parameters {dev[0]:.3f} u, exp_avg {dev[1]:.3e}, exp_avg_sq {dev[2]:.3e}   (limits {tol[0]:.1f} u, {tol[1]:.1e}, {tol[2]:.1e})")
        assert dev[0] <= tol[0] and dev[1] <= tol[1] and dev[2] <= tol[2], (s, dev, tol)
        assert _sd_steps(opt) == ref[s]["steps"], s
        assert opt.applied_and_skipped == case.expected_counters(s + 1), s

    load(0)
    opt.step(1.0, grads=static, ok=ok)                     # eager: builds the tables and the workspace the capture must not allocate
    check(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step(1.0, grads=static, ok=ok)
    for s in (1, 2, 3):
        before = _state(opt)
        load(s)
        graph.replay()
        torch.cuda.synchronize()
        if not case.events[s].applied:
            assert _same_bits(_state(opt), before)
        check(s)
    ok.fill_(case.events[4].ok)
    opt.lr_dev.fill_(case.events[4].lr)
    opt.step(1.0, grads=list(_grads(name, 4)), ok=ok)      # eager, and the two tensors take their first update
    check(4)


def test_table_limit_576_tensors():
    """576 tensors with a gradient (8 batches of 72 records) are accepted; 577 raise before anything is launched or counted.

    Bounds for one-element tensors over two steps, from the float32 format (e = 2^-24).  Parameter: per step the rounding of
    decay = 1 - lr * wd (e |p|), of p * decay and of the final fma (half an ulp each, at most 1 u): 6 u.  exp_avg_sq is a sum of
    positive terms, each off by 1 - beta2 formed in float32 (4 e), the clipped gradient entering twice (its own rounding, the float32
    cast of the norm, the division behind the clip factor: 6 e) and three roundings of the products and the fma: 13 e per step, 26 e =
    1.6e-6 of v after two.  exp_avg can cancel (0.9 m + 0.1 g with opposite signs), so a one-element tensor's error is measured against
    the same recurrence over absolute values, a = 0.9 a + 0.1 |g'|: 4 e for 1 - beta1, 3 e in g', two roundings: 9 e per step, 18 e =
    1.1e-6 of a after two."""
    from frl_hip.training.optim import HipAdamW
    n = C.MAX_TENSORS + 1
    events = [C.Event(lr=1e-3, max_norm=1.0, ok=1.0, scale=1.0, absent=frozenset({n - 1})),
              C.Event(lr=2e-3, max_norm=1.0, ok=1.0, scale=0.1, absent=frozenset({0}))]
    case = C.Case(numels=[1] * n, wds=[0.0 if i % 2 == 0 else 0.01 for i in range(n)], events=events, seed=31)
    ref = [(C.flat64(r.params), C.flat64(r.exp_avg), C.flat64(r.exp_avg_sq), r.steps, r.norm) for r in C.run_torch(case)]
    params = [torch.nn.Parameter(p.clone().to(DEV)) for p in case.params]
    opt = HipAdamW([{"params": [p], "weight_decay": wd} for p, wd in zip(params, case.wds)], lr=1e-3, betas=C.BETAS, eps=C.EPS)
    a = torch.zeros(n, dtype=torch.float64)

    def step(s):
        grads = case.grads(s)
        coef = min(1.0, 1.0 / (ref[s][4] + 1e-6))
        for i, g in enumerate(grads):
            if g is not None:
                a[i] = C.BETAS[0] * a[i] + (1.0 - C.BETAS[0]) * abs(float(g)) * coef
        for g in opt.param_groups:
            g["lr"] = case.events[s].lr
        opt.step(1.0, grads=[None if g is None else g.to(DEV) for g in grads])
        p, m, v = (t.to("cpu", torch.float64) for t in _state(opt))
        dev = (C.param_dev_u(p, ref[s][0]), float(((m - ref[s][1]).abs() / a.clamp(min=1e-300)).max()),
               float(((v - ref[s][2]).abs() / ref[s][2].clamp(min=1e-300)).max()))
        print(f"step {s}: parameters {dev[0]:.3f} u, exp_avg {dev[1]:.3e} of a, exp_avg_sq {dev[2]:.3e}")
        assert dev[0] <= 6.0 and dev[1] <= 1.1e-6 and dev[2] <= 1.6e-6, (s, dev)
        assert _sd_steps(opt) == ref[s][3]

    step(0)
    before, counts = _state(opt), (opt.step_count, opt.applied_and_skipped, _sd_steps(opt))
    with pytest.raises(Exception, match="576"):
        opt.step(1.0, grads=[torch.ones(1, device=DEV) for _ in range(n)])
    torch.cuda.synchronize()
    assert _same_bits(_state(opt), before) and (opt.step_count, opt.applied_and_skipped, _sd_steps(opt)) == counts
    step(1)
    assert opt.applied_and_skipped == (2, 0)


def test_multi_tensor_scale_copy_every_element_and_canaries():
    """frl_multi_tensor_scale_copy as the data-parallel reducer calls it: 300 records (more than two 144-record batches), chunk-edge
    sizes and one source of more than 512 chunks, every seventh source NULL, destinations at odd offsets of one canary-filled buffer."""
    from frl_hip import _lib
    from frl_hip.training.optim import ChunkTable
    numels = C.EDGE_NUMELS + C.small_numels(290, 9)
    numels.insert(200, C.BIG_NUMEL)
    assert len(numels) == 300
    g = torch.Generator().manual_seed(41)
    srcs = [None if i % 7 == 0 else torch.randn(n, generator=g) for i, n in enumerate(numels)]
    assert srcs[200] is not None and srcs[7] is None
    scale = torch.tensor(1.0 / 3.0, dtype=torch.float32)
    canary, gap = -12345.678, 3
    want = torch.full((sum(numels) + gap * (len(numels) + 1),), canary, dtype=torch.float32)
    offs, off = [], gap
    for n, s in zip(numels, srcs):
        want[off:off + n] = 0.0 if s is None else scale * s
        offs.append(off)
        off += n + gap
    dst = torch.full_like(want, canary, device=DEV)
    src_dev = [None if s is None else s.to(DEV) for s in srcs]
    raw = b"".join(struct.pack("<QQq", 0 if s is None else s.data_ptr(), dst.data_ptr() + 4 * o, n) for s, o, n in zip(src_dev, offs, numels))
    desc = ctypes.create_string_buffer(raw, len(raw))
    chunks = ChunkTable(numels, torch.device(DEV))
    _lib.check(_lib.load().frl_multi_tensor_scale_copy(ctypes.cast(desc, ctypes.c_void_p), len(numels), ctypes.c_void_p(chunks.dev.data_ptr()),
                                                       ctypes.cast(chunks.host_tensor_col, ctypes.c_void_p), chunks.n, float(scale),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "frl_multi_tensor_scale_copy")
    got = dst.cpu()
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
    assert diff.numel() == 0, f"{diff.numel()} elements differ, first at flat offset {int(diff[0])}"
