"""Shared cases for the fused clip + AdamW step (csrc/optim.hip, frl_hip.training.optim.HipAdamW): a seeded schedule of parameter
tensors, weight decays and per-step events, and the plain-torch runner both the CPU and the GPU tests compare against.  Touches no GPU.

    reference = torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=False) on CPU copies, one param group per tensor (weight
    decay is per tensor), neither function called on a skipped step (the reference trainer drops the whole batch), no clipping with
    max_norm <= 0.

The tensor set reaches what the kernels branch on: the 4096-element chunk edges, three 72-tensor batches of the by-value descriptor
table, and one tensor of more than 512 chunks (the grid-stride loop, and a re-sum of more than 64 partials) in the SECOND batch.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch

BATCH = 72                                               # OPT_BATCH of csrc/optim.hip
MAX_TENSORS = 576                                        # 8 batches x 512 partial sums = the 4096-double workspace
EDGE_NUMELS = [1, 255, 256, 257, 4095, 4096, 4097, 8192, 3 * 4096 + 5]
BIG_NUMEL = 513 * 4096 + 17                              # 514 chunks > the 512-workgroup grid
BETAS = (0.9, 0.95)
EPS = 1e-8

# Deviation of float32 torch.optim.AdamW (CPU) from the float64 runner over full_case(), measured by tests/test_cpu_optim_cases.py
# (which fails when a figure here is exceeded or is more than twice what it measures):
#   parameters in units of u = 2**-24 * max(1, |p_ref|), elementwise; moments relative to each tensor's max |m| / max |v|.
F32_PARAM_DEV_U = 7.0      # measured 6.77
F32_M_DEV_REL = 4.6e-5     # measured 4.59e-5: float32 torch's norm of the 2.1 M-element gradient is 2.7e-5 low, and so is its clip factor
F32_V_DEV_REL = 5.6e-5     # measured 5.51e-5 (the clip factor squared)
# The same for graph_case() (four applied steps, 100 tensors of at most 12293 elements: float32 norms are accurate there).
GRAPH_F32_PARAM_DEV_U = 5.5   # measured 5.47
GRAPH_F32_M_DEV_REL = 2.3e-7   # measured 2.23e-7
GRAPH_F32_V_DEV_REL = 3.5e-7   # measured 3.41e-7
# The HIP kernel may deviate twice as much: its operation order is not torch's float32 path (decay multiply first, then
# m / denom * step_size, fused multiply-adds, a float64 clip norm).
GPU_MARGIN = 2.0


@dataclass
class Event:
    lr: float
    max_norm: float
    ok: float                                            # the device guard word: applied <=> ok > 0 (0.0, -1.0 and NaN all skip)
    scale: float                                         # gradient scale
    absent: frozenset                                    # tensor indices without a gradient this step

    @property
    def applied(self) -> bool:
        return self.ok > 0.0                             # False for NaN, as `ok[0] > 0.f` on the device


@dataclass
class Case:
    numels: List[int]
    wds: List[float]
    events: List[Event]
    seed: int
    params: List[torch.Tensor] = field(default_factory=list)

    def __post_init__(self):
        g = torch.Generator().manual_seed(self.seed)
        self.params = [torch.randn(n, generator=g) for n in self.numels]

    def grads(self, step: int) -> List[Optional[torch.Tensor]]:
        """float32 gradients of one step (None: the tensor has none), regenerated from the seed on every call."""
        ev = self.events[step]
        g = torch.Generator().manual_seed(self.seed * 1000 + 17 + step)
        return [None if i in ev.absent else torch.randn(n, generator=g) * ev.scale for i, n in enumerate(self.numels)]

    def expected_steps(self, upto: int) -> List[int]:
        """Per-tensor update count after events[:upto]: applied steps on which the tensor had a gradient."""
        return [sum(1 for ev in self.events[:upto] if ev.applied and i not in ev.absent) for i in range(len(self.numels))]

    def expected_counters(self, upto: int):
        """(applied, skipped) as HipAdamW counts them: a step on which NO tensor has a gradient launches nothing and counts as neither."""
        live = [ev for ev in self.events[:upto] if len(ev.absent) < len(self.numels)]
        return sum(1 for ev in live if ev.applied), sum(1 for ev in live if not ev.applied)


def small_numels(count: int, seed: int) -> List[int]:
    return torch.randint(1, 301, (count,), generator=torch.Generator().manual_seed(seed)).tolist()


SKIPPED = (0, 4, 7)
NO_GRAD_STEP = 6
BIG_INDEX = 100


def full_case() -> Case:
    """160 tensors (9 chunk-edge sizes, 150 of 1..300 elements, the 514-chunk one at index 100), 10 steps."""
    numels = EDGE_NUMELS + small_numels(150, 5)
    numels.insert(BIG_INDEX, BIG_NUMEL)
    n = len(numels)
    wds = [0.0 if i % 2 == 0 else 0.01 for i in range(n)]
    alt_odd, alt_even = {3, 20, 130}, {6, 81}            # without a gradient on odd / even steps
    first_five = {1, 40, 101, 150}                       # steps 0..4
    on_skipped = {2, 50, 120}                            # exactly the skipped steps, step 0 included
    never = {10, 145}
    #          step:  0     1     2     3     4     5     6     7     8     9
    scales = [1e-1, 1e-4, 1e3, 1e-2, 1e3, 3e-4, 1.0, 1e2, 1.0, 1e-3]     # sum over ~2.4 M elements: the norm is ~1550 x scale
    oks = [0.0, 1.0, 1.0, 1.0, -1.0, 1.0, 1.0, math.nan, 1.0, 1.0]
    events = []
    for s in range(10):
        absent = set(never)
        absent |= alt_odd if s % 2 == 1 else alt_even
        if s < 5:
            absent |= first_five
        if s in SKIPPED:
            absent |= on_skipped
        if s == NO_GRAD_STEP:
            absent = set(range(n))
        events.append(Event(lr=2e-3 * (0.5 + 0.1 * s), max_norm=0.0 if s == 3 else 1.0, ok=oks[s], scale=scales[s],
                            absent=frozenset(absent)))
    assert [s for s, ev in enumerate(events) if not ev.applied] == list(SKIPPED)
    live_before_big = min(BIG_INDEX - len([i for i in ev.absent if i < BIG_INDEX]) for s, ev in enumerate(events) if s != NO_GRAD_STEP)
    assert BATCH <= live_before_big < 2 * BATCH          # the grid-stride batch is the second one on every step
    assert min(n - len(ev.absent) for s, ev in enumerate(events) if s != NO_GRAD_STEP) > 2 * BATCH
    return Case(numels=numels, wds=wds, events=events, seed=11)


GRAPH_ABSENT = frozenset({4, 90})


def graph_case() -> Case:
    """The captured-step schedule: an eager first step (it builds the tables the capture needs), three replays of one captured step (the
    second at ok = 0), all with tensors 4 and 90 absent from the table, then an eager step that gives every tensor a gradient."""
    numels = EDGE_NUMELS + small_numels(91, 6)
    wds = [0.0 if i % 2 == 0 else 0.01 for i in range(len(numels))]
    spec = [(1.0, 1.0), (1.0, 1e-4), (0.0, 10.0), (1.0, 1.0), (1.0, 1e-2)]
    events = [Event(lr=1e-3 * (1 + s), max_norm=1.0, ok=ok, scale=sc, absent=GRAPH_ABSENT if s < 4 else frozenset())
              for s, (ok, sc) in enumerate(spec)]
    return Case(numels=numels, wds=wds, events=events, seed=23)


@dataclass
class Snapshot:
    step: int                                            # index of the event just processed
    params: List[torch.Tensor]                           # live tensors of the runner: read them before advancing it
    exp_avg: List[torch.Tensor]
    exp_avg_sq: List[torch.Tensor]
    steps: List[int]                                     # torch's per-parameter state["step"], 0 where torch holds no state
    norm: float                                          # float64 global gradient norm of this step's gradients (0.0 without any)


def run_torch(case: Case, dtype=torch.float64):
    """Generator over the schedule: clip_grad_norm_ + AdamW(foreach=False) in `dtype` on the CPU, one Snapshot per event."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in case.params]
    opt = torch.optim.AdamW([{"params": [p], "weight_decay": wd} for p, wd in zip(params, case.wds)], lr=1.0, betas=BETAS, eps=EPS,
                            foreach=False)
    zeros = [torch.zeros_like(p) for p in params]
    for s, ev in enumerate(case.events):
        grads = case.grads(s)
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads if g is not None))
        if ev.applied:
            for p, g in zip(params, grads):
                p.grad = None if g is None else g.to(dtype)
            for grp in opt.param_groups:
                grp["lr"] = ev.lr
            live = [p for p in params if p.grad is not None]
            if live and ev.max_norm > 0:
                torch.nn.utils.clip_grad_norm_(live, ev.max_norm, foreach=False)
            if live:
                opt.step()
        st = [opt.state.get(p, {}) for p in params]
        yield Snapshot(step=s, params=[p.detach() for p in params],
                       exp_avg=[t.get("exp_avg", z) for t, z in zip(st, zeros)], exp_avg_sq=[t.get("exp_avg_sq", z) for t, z in zip(st, zeros)],
                       steps=[int(float(t["step"])) if "step" in t else 0 for t in st], norm=norm)


def flat64(tensors) -> torch.Tensor:
    return torch.cat([t.detach().reshape(-1).to("cpu", torch.float64) for t in tensors])


def param_dev_u(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max over elements of |got - ref| / (2**-24 * max(1, |ref|)); flat float64 inputs."""
    return float(((got - ref).abs() / (2.0 ** -24 * ref.abs().clamp(min=1.0))).max())


def moment_dev_rel(got: torch.Tensor, ref: torch.Tensor, numels: List[int]) -> float:
    """max over elements of |got - ref| / (max |ref| of the element's tensor); a tensor whose reference moment is all zero (torch holds
    no state for it) must be exactly zero -- inf otherwise.  Flat float64 inputs."""
    n = torch.tensor(numels)
    top = torch.stack([r.abs().max() for r in ref.split(numels)])
    scale = torch.repeat_interleave(top, n)
    err = (got - ref).abs()
    if bool((err[scale == 0] != 0).any()):
        return math.inf
    return float((err[scale > 0] / scale[scale > 0]).max()) if bool((scale > 0).any()) else 0.0
