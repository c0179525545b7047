"""The reference, bounds, emulation and case table of tests/vq_backward_cases.py, checked without a GPU: the float64 reference against
autograd through the oracle's quantizer, the EMA reference against the oracle's update, the float32 emulation of the kernels' arithmetic
inside every bound on every case (so the bounds are not tighter than correct float32 code needs), every mutant outside at least one bound
wherever it applies (so they are not looser than a wrong kernel needs), and the table reaching every branch the kernels have."""
import functools

import pytest
import torch

import frl_oracle as O
import vq_backward_cases as C

# (name, gscale given, g_out given): the upstream variants the GPU test runs
VARIANTS = (("scaled", True, True), ("unit_scale", False, True), ("no_gout", True, False))
SMALL = ("N300-K16-d8-one_code", "N65-K37-d40-sorted", "N3000-K37-d50-uniform", "N3000-K257-d72-edges", "N3000-K37-d10-uniform",
         "N16385-K37-d12-half_unused")


@functools.lru_cache(maxsize=None)
def _reference(cid, dtype, variant):
    case = C.case_by_id(cid)
    _, scaled, with_gout = next(v for v in VARIANTS if v[0] == variant)
    inp = C.inputs(case, dtype)
    return C.reference(inp, inp["gscale"] if scaled else None, C.BETA, with_gout)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cid", SMALL)
def test_reference_equals_float64_autograd_through_the_oracle(cid, dtype):
    """d/dz and d/dE of  <z_st, g_out> + gs1 L_codebook + gs0 beta L_commit  (the kernel folds beta into the commitment scale)."""
    case = C.case_by_id(cid)
    inp = C.inputs(case, dtype)
    ref = _reference(cid, dtype, "scaled")
    z = inp["z"].double().requires_grad_(True)
    e = inp["e_eff"].double().requires_grad_(True)
    z_st, _, _, _, l_cb, l_cm = O.vq_forward(z, e, beta=C.BETA, idx=inp["idx"].long())
    gs0, gs1 = float(inp["gscale"][0]), float(inp["gscale"][1])
    ((z_st * inp["g_out"].double()).sum() + gs1 * l_cb + gs0 * C.BETA * l_cm).backward()
    assert (z.grad - ref["gz"]).abs().max() <= 1e-12 * ref["gz"].abs().max()
    assert (e.grad - ref["ge"]).abs().max() <= 1e-12 * ref["ge"].abs().max()
    assert torch.equal(torch.bincount(inp["idx"].long(), minlength=case.k).to(torch.int32), inp["counts"])


@pytest.mark.parametrize("k,d", C.EMA_SHAPES)
def test_ema_reference_equals_the_oracle_with_rounded_scalars(k, d):
    g = torch.Generator().manual_seed(k + d)
    n = 40 * k
    z = torch.randint(-8, 9, (n, d), generator=g).double() / 4            # per-code sums are exact in float32
    idx = torch.randint(0, max(k // 2, 1), (n,), generator=g)
    inp = C.ema_inputs(k, d)
    inp = dict(inp, sums=torch.zeros(k, d, dtype=torch.float64).index_add_(0, idx, z).float(),
               counts=torch.bincount(idx, minlength=k).to(torch.int32))
    assert torch.equal(inp["sums"].double(), torch.zeros(k, d, dtype=torch.float64).index_add_(0, idx, z))
    dc, ep = C.ema_scalars(C.EMA_DECAY, C.EMA_EPS)
    cb, cnt, sm = O.vq_ema_update(inp["codebook"].double(), inp["ema_count"].double(), inp["ema_sum"].double(), z, idx, dc, ep)
    ref = C.ema_reference(inp)
    for got, name in ((cb, "codebook"), (cnt, "ema_count"), (sm, "ema_sum")):
        assert (got - ref[name]).abs().max() <= 1e-13 * ref[name].abs().max(), name


@pytest.mark.parametrize("k,d", C.EMA_SHAPES)
def test_ema_emulation_inside_bounds_and_unrounded_decay_outside(k, d):
    inp = C.ema_inputs(k, d)
    ref = C.ema_reference(inp)
    r = C.ema_ratios(C.ema_emulate(inp), ref)
    print(f"EMA K={k} d={d}: emulation err/bound {r}")
    assert max(r.values()) <= 1.0, r
    if k > 1:                                              # where the old count is zero, the 1e-6 relative error of 1 - 0.99 is all there is
        wrong = C.ema_reference(inp, rounded=False)
        r = C.ema_ratios(wrong, ref)
        print(f"EMA K={k} d={d}: float64 reference with the unrounded decay, err/bound {r}")
        assert r["ema_count"] > 1.0, r


WORST = {}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_emulation_inside_bounds_and_mutants_outside(cid, dtype):
    case = C.case_by_id(cid)
    inp = C.inputs(case, dtype)
    sums = {m: C.emulate_sums(inp, dtype, m) for m in (None, "moved_row")}
    for variant, scaled, with_gout in VARIANTS:
        gs = inp["gscale"] if scaled else None
        ref = _reference(cid, dtype, variant)
        r = C.ratios(C.emulate(inp, dtype, gs, C.BETA, with_gout, sums=sums[None]), ref)
        for name, v in r.items():
            key = ("f32" if dtype == "f32" else "%d,%d,%d" % C.bf16_instance(case.d), name)
            WORST[key] = max(WORST.get(key, 0.0), v)
        assert max(r.values()) <= 1.0, (variant, r)
        for mutant in C.MUTANTS:
            if not C.mutant_applies(mutant, case, dtype, gs, C.BETA, with_gout):
                continue
            m = C.ratios(C.emulate(inp, dtype, gs, C.BETA, with_gout, mutant=mutant, sums=sums.get(mutant, sums[None])), ref)
            assert max(m.values()) > 1.0, (variant, mutant, m)
            key = ("mutant", mutant)
            WORST[key] = min(WORST.get(key, float("inf")), max(m.values()))
    _reference.cache_clear()


def test_report_worst_ratios():
    """Printed with -s: the worst emulation err/bound per kernel instance and output, and the least err/bound any mutant reached."""
    for key in sorted(WORST):
        print("%-8s %-20s %.4g" % (key[0], key[1], WORST[key]))


def test_unused_codes_have_zero_bounds():
    case = C.case_by_id("N3000-K1030-d32-half_unused")
    ref = C.reference(C.inputs(case, "bf16"), None, C.BETA)
    assert bool((ref["sums_bound"][case.k // 2:] == 0).all()) and bool((ref["ge_bound"][case.k // 2:] == 0).all())
    assert bool((ref["sums_bound"][:case.k // 2] > 0).any())
    got = dict(sums=ref["sums"].clone(), ge=ref["ge"].clone())
    got["sums"][-1, -1] = 1e-30
    assert C.ratios(got, ref)["sums"] == float("inf")


def test_restated_host_decisions():
    assert [C.bf16_chunk(d) for d in (8, 32, 33, 64, 65, 128)] == [512, 512, 512, 512, 256, 256]
    assert C.chunk_sizes(385, 64, "f32") == [193, 192]
    assert C.chunk_sizes(512, 64, "f32") == [256, 256] and C.f32_lds_bytes(512, 64) == 64 * 1024
    assert C.chunk_sizes(1030, 64, "f32") == [258, 258, 258, 256] and C.f32_lds_bytes(1030, 64) > 64 * 1024
    assert C.chunk_sizes(600, 128, "f32") == [150] * 4 and C.f32_lds_bytes(600, 128) == 76800
    assert C.chunk_sizes(96, 64, "f32") == [96]
    assert C.chunk_sizes(1030, 64, "bf16") == [512, 512, 6] and C.chunk_sizes(600, 100, "bf16") == [256, 256, 88]
    assert C.rows_per_workgroup(16385, "bf16") == 128 and C.rows_per_workgroup(16385, "f32") == 65
    part = C.row_partition(16385, "bf16")
    assert part[127] == (127 * 128, 16384) and part[128] == (16384, 16385) and part[129] == (16385, 16385)
    assert C.row_partition(16421, "bf16")[128] == (16384, 16421)
    assert C.row_partition(300, "f32")[149] == (298, 300) and C.row_partition(300, "f32")[150] == (300, 300)


def test_table_reaches_every_branch():
    reached = {"f32": set(), "bf16": set()}
    per_instance = {}
    for c in C.cases():
        for dtype in ("f32", "bf16"):
            b = C.branches(c.n, c.k, c.d, dtype)
            reached[dtype] |= b
            inst = next(x for x in b if x.startswith("instance:"))
            per_instance.setdefault(inst, set()).update(b)
    for inst in ("instance:4,2,8", "instance:4,4,8", "instance:2,8,8"):
        need = {"chunks:1", "chunks:2", "chunks:>=3", "ragged_last_chunk", "vector", "scalar", "below_padded_width", "empty_workgroups",
                "one_row_last_workgroup", "partial_last_tile", "n_below_tile", "several_tiles"}
        assert need <= per_instance[inst], (inst, need - per_instance[inst])
    need = {"chunks:1", "chunks:2", "chunks:>=3", "ragged_last_chunk", "vector", "scalar", "lds_opt_in", "empty_workgroups",
            "one_row_last_workgroup"}
    assert need <= per_instance["instance:f32"], need - per_instance["instance:f32"]
    assert {c.pattern for c in C.cases()} == set(C.PATTERNS)
    assert 40 <= len(C.cases()) <= 50
    for c, dtype in C.deferred_cases():
        assert len(C.chunk_sizes(c.k, c.d, dtype)) > 1
        if dtype == "f32":
            assert C.rows_per_workgroup(c.n, dtype) <= 2
