"""The quantizer's backward and EMA kernels (csrc/vq.hip through ops.vq_bwd / ops.vq_ema_update) against the float64 reference and the
a-priori bounds of tests/vq_backward_cases.py, elementwise, on every case of its table in both row dtypes and in every call variant
production uses: indices are synthetic, the upstream scales make the commitment and codebook terms O(1) against g_out, and the workspace
is filled with 0xFF bytes before every call so that a slab entry the kernel does not write shows as NaN.

bf16 (fixed-order MFMA accumulation, fixed-order slab reduction): the per-code sums and g_E are bit-identical from call to call, with and
without z_q, with and without g_z.  Nothing of the kind is asserted for g_z between the prefetch and staged paths, nor for float32, whose
kernel sums with LDS float atomics (but see vq_backward_cases.deferred_cases)."""
import math

import pytest
import torch

import vq_backward_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {}


def _ops():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    from frl_hip import ops
    return ops


def _on_device(inp):
    return {k: inp[k].to(DEV) for k in ("z", "g_out", "codebook", "idx", "counts", "zq", "gscale")}


def _bwd(ops, di, g_out=True, zq=True, gscale=True, beta=C.BETA, **kw):
    from frl_hip import _lib
    n, d = di["z"].shape
    k = di["codebook"].shape[0]
    ops.workspace(_lib.load().frl_vq_workspace_bytes(n, k, d), DEV).fill_(255)
    return ops.vq_bwd(di["g_out"] if g_out else None, di["z"], di["codebook"], di["idx"], di["counts"], di["gscale"] if gscale else None,
                      beta, zq=di["zq"] if zq else None, **kw)


def _inside(out, ref, what, key):
    gz, ge, sums = out
    r = C.ratios(dict(gz=gz, ge=ge, sums=sums), ref)
    print(f"    {what}: err/bound {({k: round(v, 4) for k, v in r.items()})}")
    for name, v in r.items():
        WORST[key + (name,)] = max(WORST.get(key + (name,), 0.0), v)
    assert all(v <= 1.0 for v in r.values()), (what, r)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_vq_bwd_inside_bounds(cid, dtype):
    ops = _ops()
    case = C.case_by_id(cid)
    inp = C.inputs(case, dtype)
    di = _on_device(inp)
    key = ("f32" if dtype == "f32" else "%d,%d,%d" % C.bf16_instance(case.d),)
    print(f"{cid} {dtype}: {case.why}")
    ref = C.reference(inp, inp["gscale"], C.BETA)
    full = _bwd(ops, di, want_sums=True)
    assert full[0].dtype == di["z"].dtype and full[0].shape == di["z"].shape
    assert full[1].dtype == torch.float32 and full[1].shape == (case.k, case.d) and full[2].shape == (case.k, case.d)
    _inside(full, ref, "z_q given", key)
    again = _bwd(ops, di, want_sums=True)
    staged = _bwd(ops, di, zq=False, want_sums=True)
    _inside(staged, ref, "z_q = None", key)
    no_gz = _bwd(ops, di, want_gz=False)
    assert no_gz[0] is None and no_gz[2] is None
    _inside(no_gz, ref, "want_gz = False", key)
    no_ge = _bwd(ops, di, want_ge=False)
    assert no_ge[1] is None and no_ge[2] is None
    _inside(no_ge, ref, "want_ge = False", key)
    ema = _bwd(ops, di, g_out=False, zq=False, gscale=False, beta=0.0, want_gz=False, want_ge=False, want_sums=True)
    assert ema[0] is None and ema[1] is None
    _inside(ema, ref, "the EMA call", key)
    if dtype == "bf16":
        for other, what in ((again, "a second call"), (staged, "z_q = None"), (ema, "the EMA call")):
            assert _same_bits(full[2], other[2]), f"per-code sums differ in bits: {what}"
        for other, what in ((again, "a second call"), (staged, "z_q = None"), (no_gz, "want_gz = False")):
            assert _same_bits(full[1], other[1]), f"g_E differs in bits: {what}"
    del ref
    ref = C.reference(inp, inp["gscale"], C.BETA, with_gout=False)
    _inside(_bwd(ops, di, g_out=False, want_sums=True), ref, "g_out = None", key)
    _inside(_bwd(ops, di, g_out=False, zq=False), ref, "g_out = None, z_q = None", key)
    ref = C.reference(inp, None, C.BETA)
    _inside(_bwd(ops, di, gscale=False, want_sums=True), ref, "gscale = None", key)


@pytest.mark.parametrize("which", [0, 1], ids=["bf16", "f32"])
def test_vq_bwd_deferred_reduction_gives_the_same_bits(which):
    ops = _ops()
    from frl_hip import _lib
    case, dtype = C.deferred_cases()[which]
    inp = C.inputs(case, dtype)
    di = _on_device(inp)
    ref = C.reference(inp, inp["gscale"], C.BETA)
    _, ge_now, _ = _bwd(ops, di)
    with ops.deferred_reductions([]):
        gz, ge, _ = ops.vq_bwd(di["g_out"], di["z"], di["codebook"], di["idx"], di["counts"], di["gscale"], C.BETA, zq=di["zq"])
        ops.discard(ge)                                    # no parameter adopts it here
        assert _lib.load().frl_defer_pending() == 1
    assert C.ratios(dict(gz=gz, ge=ge), ref)["ge"] <= 1.0
    assert _same_bits(ge, ge_now)


@pytest.mark.parametrize("k,d", C.EMA_SHAPES)
def test_vq_ema_update_inside_bounds_and_ok_guard(k, d):
    ops = _ops()
    inp = C.ema_inputs(k, d)
    ref = C.ema_reference(inp)
    state = lambda: {name: inp[name].clone().to(DEV) for name in ("ema_count", "ema_sum", "codebook")}
    sums, counts = inp["sums"].to(DEV), inp["counts"].to(DEV)

    def run(ok):
        st = state()
        okt = None if ok is None else torch.tensor([ok], dtype=torch.float32, device=DEV)
        ops.vq_ema_update(sums, counts, st["ema_count"], st["ema_sum"], st["codebook"], C.EMA_DECAY, C.EMA_EPS, okt)
        return st

    out = run(None)
    r = C.ema_ratios(out, ref)
    print(f"EMA K={k} d={d}: err/bound {({n: round(v, 4) for n, v in r.items()})}")
    for name, v in r.items():
        WORST[("ema", name)] = max(WORST.get(("ema", name), 0.0), v)
    assert all(v <= 1.0 for v in r.values()), r
    applied = run(1.0)
    for name in out:
        assert _same_bits(out[name], applied[name]), name
    for ok in (0.0, -1.0, math.nan):
        kept = run(ok)
        for name in kept:
            assert _same_bits(kept[name], inp[name].to(DEV)), (ok, name)


def test_vq_bwd_refusals():
    ops = _ops()
    from frl_hip._lib import FrlHipError
    g = torch.Generator().manual_seed(0)
    n, k = 100, 5

    def args(d, dtype):
        z = torch.randn(n, d, generator=g).to(dtype).to(DEV)
        cb = torch.randn(k, d, generator=g).to(DEV)
        idx = torch.randint(0, k, (n,), generator=g).to(torch.int32).to(DEV)
        counts = torch.bincount(idx.long(), minlength=k).to(torch.int32)
        return dict(g_out=torch.randn(n, d, generator=g).to(dtype).to(DEV), z=z, codebook=cb, idx=idx, counts=counts,
                    gscale=torch.ones(2, device=DEV), beta=C.BETA)

    with pytest.raises(FrlHipError):                       # the widest matrix-core instance covers 128 channels
        ops.vq_bwd(**args(136, torch.bfloat16))
    with pytest.raises(FrlHipError):
        ops.vq_bwd(**dict(args(8, torch.float32), codebook=torch.zeros(0, 8, device=DEV), counts=torch.zeros(0, dtype=torch.int32, device=DEV)))
    a = args(136, torch.float32)                           # the float32 kernel is generic in d
    gz, ge, sums = ops.vq_bwd(want_sums=True, **a)
    inp = dict(z=a["z"].cpu(), g_out=a["g_out"].cpu(), e_eff=a["codebook"].cpu(), idx=a["idx"].cpu())
    inp["sums64"] = torch.zeros(k, 136, dtype=torch.float64).index_add_(0, inp["idx"].long(), inp["z"].double())
    inp["abs_sums64"] = torch.zeros(k, 136, dtype=torch.float64).index_add_(0, inp["idx"].long(), inp["z"].double().abs())
    r = C.ratios(dict(gz=gz, ge=ge, sums=sums), C.reference(inp, a["gscale"].cpu(), C.BETA))
    assert all(v <= 1.0 for v in r.values()), r

    a = args(16, torch.bfloat16)
    wide = torch.randn(n, 32, generator=g).to(torch.bfloat16).to(DEV)
    bad = [dict(idx=a["idx"].long()), dict(idx=a["idx"][:-1]), dict(idx=a["idx"].cpu()),
           dict(counts=a["counts"].long()), dict(counts=a["counts"][:-1]),
           dict(z=wide[:, :16]), dict(z=a["z"].cpu()), dict(z=a["z"][:, :8].contiguous()),
           dict(g_out=a["g_out"].float()), dict(g_out=a["g_out"][:-1]), dict(g_out=wide[:, :16]),
           dict(zq=a["z"].float()), dict(zq=a["z"][1:]), dict(zq=wide[:, :16]),
           dict(gscale=a["gscale"].double()), dict(gscale=a["gscale"][:1]), dict(gscale=a["gscale"].cpu()),
           dict(gscale=torch.ones(4, device=DEV)[::2])]
    for change in bad:
        with pytest.raises(ValueError):
            ops.vq_bwd(**dict(a, **change))
        torch.cuda.synchronize()
    gz, ge, _ = ops.vq_bwd(zq=a["codebook"].to(torch.bfloat16)[a["idx"].long()], **a)      # and the valid call still runs
    assert bool(torch.isfinite(gz.float()).all()) and bool(torch.isfinite(ge).all())


def test_report_worst_ratios():
    """Printed with -s: the worst err/bound seen per kernel instance and output in this session."""
    for key in sorted(WORST):
        print("%-8s %-10s %.4g" % (key[0], key[1], WORST[key]))
