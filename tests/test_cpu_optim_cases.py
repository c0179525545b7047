"""The optimizer schedule of tests/optim_cases.py on the CPU: float32 torch.optim.AdamW against the float64 runner.  What float32 torch
loses over the schedule is the yardstick of tests/test_gpu_optim.py (the HIP kernel may deviate twice as much), so the figures are
measured here and pinned as constants in optim_cases.py."""
import math

import pytest
import torch

import optim_cases as C


def _measure(case):
    dev = {"p": 0.0, "m": 0.0, "v": 0.0}
    for s32, s64 in zip(C.run_torch(case, torch.float32), C.run_torch(case, torch.float64)):
        want = case.expected_steps(s64.step + 1)
        assert s64.steps == want and s32.steps == want, f"step {s64.step}: torch's per-parameter step is not the applied-with-gradient count"
        dev["p"] = max(dev["p"], C.param_dev_u(C.flat64(s32.params), C.flat64(s64.params)))
        dev["m"] = max(dev["m"], C.moment_dev_rel(C.flat64(s32.exp_avg), C.flat64(s64.exp_avg), case.numels))
        dev["v"] = max(dev["v"], C.moment_dev_rel(C.flat64(s32.exp_avg_sq), C.flat64(s64.exp_avg_sq), case.numels))
        assert all(bool(torch.isfinite(t).all()) for t in s32.params)
    return dev


@pytest.mark.parametrize("name,pinned", [("full", (C.F32_PARAM_DEV_U, C.F32_M_DEV_REL, C.F32_V_DEV_REL)),
                                         ("graph", (C.GRAPH_F32_PARAM_DEV_U, C.GRAPH_F32_M_DEV_REL, C.GRAPH_F32_V_DEV_REL))])
def test_float32_torch_deviation_is_the_pinned_one(name, pinned):
    case = C.full_case() if name == "full" else C.graph_case()
    dev = _measure(case)
    print(f"{name}: float32 torch vs float64: parameters {dev['p']:.3f} u, exp_avg {dev['m']:.3e}, exp_avg_sq {dev['v']:.3e} (relative)")
    for got, pin in zip((dev["p"], dev["m"], dev["v"]), pinned):
        assert math.isfinite(got) and got <= pin <= 2.0 * got, (name, dev, pinned)


def test_schedule_is_the_one_the_kernels_need():
    case = C.full_case()
    n = len(case.numels)
    assert case.numels[:9] == C.EDGE_NUMELS and case.numels[C.BIG_INDEX] == C.BIG_NUMEL and C.BIG_INDEX >= C.BATCH
    assert n == 160 and all(1 <= k <= 300 for i, k in enumerate(case.numels) if i >= 9 and i != C.BIG_INDEX)
    assert set(case.wds) == {0.0, 0.01} and case.wds[0] != case.wds[1]
    ev = case.events
    assert len(ev) == 10 and len({e.lr for e in ev}) == 10
    assert [e.max_norm for e in ev].count(0.0) == 1 and [e.max_norm for e in ev].count(1.0) == 9
    skipped = [s for s, e in enumerate(ev) if not e.applied]
    assert skipped == [0, 4, 7] and [ev[s].ok for s in (0, 4)] == [0.0, -1.0] and math.isnan(ev[7].ok)
    assert min(e.scale for e in ev) == 1e-4 and max(e.scale for e in ev) == 1e3
    assert sum(1 for e in ev if len(e.absent) == n) == 1 and ev[C.NO_GRAD_STEP].applied
    missing = {i: [s for s, e in enumerate(ev) if i in e.absent and s != C.NO_GRAD_STEP] for i in range(n)}
    assert any(m == [1, 3, 5, 7, 9] for m in missing.values()) and any(m == [0, 2, 4, 8] for m in missing.values())   # alternate
    assert any(m == [0, 1, 2, 3, 4] for m in missing.values())
    assert any(m == skipped for m in missing.values())
    assert any(len(m) == 9 for m in missing.values())                                                            # never a gradient
    # clipping is active on some applied steps and not on others: the norm is sqrt(sum g^2) ~ scale * sqrt(live elements)
    norms = [s.norm for s in C.run_torch(C.Case(case.numels, case.wds, [C.Event(e.lr, e.max_norm, 0.0, e.scale, e.absent) for e in ev], case.seed))]
    active = [norms[s] > 1.0 for s, e in enumerate(ev) if e.applied and e.max_norm > 0 and s != C.NO_GRAD_STEP]
    assert any(active) and not all(active)
    # every gradient value is far inside float32's range for g * g (no underflow to a subnormal, no overflow)
    for s in range(10):
        gs = torch.cat([g for g in case.grads(s) if g is not None] or [torch.ones(1)]).abs()
        assert 1e-15 < float(gs[gs > 0].min()) and float(gs.max()) < 1e15
    assert case.expected_steps(10)[C.BIG_INDEX] == 6 and case.expected_counters(10) == (6, 3)
