"""The train step without its framework launches: the quantizer's prepared image as a job of the post-optimizer pack launch, the second
statistics record stored by the assignment kernel, the quantizer backward reading its two upstream scalars in place, autograd nodes that
do not materialise zero gradients, and the cached root gradient.  Everything here is an equality of bits against the launches it replaces.

Shapes are the smallest that take each route: K x 64 codebooks of 64 and 512 codes (one LDS chunk: streaming kernel at N = 768 = three
batches of 256 rows, resident kernel at N = 1000) and 1024 codes (bf16 image 128 KB > 64 KB: the chunked route); the model is B = 2,
T = 5, 16 x 16 pixels (HW = 256, a multiple of 64: the hot kernels), K = 64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32

# device launches of one eager train step that the library does not issue (the replayed step adds one fill of the
# learning-rate word, outside the graph)
FRAMEWORK_LAUNCHES_LEFT = 0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _lib():
    from frl_hip import _lib
    return _lib.load()


def _ctl(img, k):
    """control block of a prepared image: 64 header ints + the histogram accumulator of K ints"""
    return img[:256 + 4 * k].view(torch.int32)


def _fresh_image(cb, n, dtype):
    """stand-alone prepare into a buffer that starts as 0xFF everywhere: every byte the kernel does not write is known"""
    from frl_hip import ops
    k, d = cb.shape
    buf = torch.full((_lib().frl_vq_prepared_bytes(k, d),), 255, dtype=torch.uint8, device=cb.device)
    out = ops.vq_prepare(cb.detach(), n, dtype, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    return out


def _quantizer_with_job(k, d, dtype, n, seed):
    """(quantizer, cache, optimizer): the quantizer's image exists, starts from 0xFF bytes, and is a job of the cache"""
    from frl_hip import ops
    from frl_hip.models.vqvae import VectorQuantizer
    from frl_hip.training.optim import HipAdamW
    q = VectorQuantizer(k, d).to(DEV)
    with torch.no_grad():
        q.codebook.copy_(torch.randn(k, d, generator=_gen(seed)))
    buf = torch.full((_lib().frl_vq_prepared_bytes(k, d),), 255, dtype=torch.uint8, device=DEV)
    q._prepared = ((None, None, dtype), buf)
    assert q.prepared(dtype, n).data_ptr() == buf.data_ptr()
    cache = ops.PackCache(torch.device(DEV), nbytes=1 << 20)
    assert cache.add_quantizer(q) and cache.add_quantizer(q)          # (registering twice is free)
    opt = HipAdamW([{"params": [q.codebook], "weight_decay": 0.0}], lr=1e-2)
    return q, cache, opt


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("k,d", [(64, 64), (512, 64), (1024, 64), (64, 32)])
def test_pack_job_prepare_equals_vq_prepare(k, d, dtype):
    """(64, 32): a bf16 image whose fragment part (256 items) is no whole block of the pack launch: its norm items start a block of their own."""
    from frl_hip import ops
    q, cache, opt = _quantizer_with_job(k, d, dtype, 768, seed=k)
    before = q._prepared[1].clone()
    q._prepared[1].fill_(255)                                         # whatever the refresh leaves here, the job wrote
    q.codebook.grad = torch.randn(k, d, generator=_gen(k + 1)).to(DEV)
    opt.step(1.0)
    version = q.codebook._version
    cache.refresh()
    cb = q.codebook.detach()
    assert q._prepared[0] == (cb.data_ptr(), version, dtype)          # current for the version the launch read: prepared() launches nothing
    img = q.prepared(dtype, 768)
    fresh = _fresh_image(cb, 768, dtype)
    assert img.data_ptr() == q._prepared[1].data_ptr() and torch.equal(img, fresh)     # norms, fragments, control block, and nothing else
    assert not torch.equal(img, before)                              # (the optimizer moved the codebook: another image)
    assert int(_ctl(img, k).abs().max()) == 0
    for n in (768, 1000):                                            # three whole streaming batches / the resident route (bf16, K <= 512)
        z = torch.randn(n, d, generator=_gen(n + k)).to(dtype).to(DEV)
        a = ops.vq_assign(z, cb, img)
        b = ops.vq_assign(z, cb, fresh)
        for x, y, name in zip(a, b, ("idx", "z_q", "stats", "counts")):
            assert torch.equal(x, y), (k, dtype, n, name)
        assert int(a[3].sum()) == n
        assert int(_ctl(img, k).abs().max()) == 0 and int(_ctl(fresh, k).abs().max()) == 0
    cache.close()


@pytest.mark.parametrize("k", [64, 1024])
def test_assignment_leaves_its_state_clean_and_stores_the_statistics_twice(k):
    """Two assignments in a row on different rows through ONE job-written image, nothing zeroed in between: the second equals the
    assignment through a fresh image, the second statistics record has the bits of the first, the control block reads zero."""
    from frl_hip import ops
    d = 64
    q, cache, opt = _quantizer_with_job(k, d, BF, 768, seed=3)
    q.codebook.grad = torch.randn(k, d, generator=_gen(4)).to(DEV)
    opt.step(1.0)
    cache.refresh()
    cb, img = q.codebook.detach(), q.prepared(BF, 768)
    for n in (768, 1000):
        z1, z2 = (torch.randn(n, d, generator=_gen(s)).to(BF).to(DEV) for s in (5, 6))
        ops.vq_assign(z1, cb, img, stats_copy=True)
        got = ops.vq_assign(z2, cb, img, stats_copy=True)
        ref = ops.vq_assign(z2, cb, _fresh_image(cb, n, BF))
        assert len(got) == 5 and torch.equal(got[4], got[2]) and got[4].data_ptr() != got[2].data_ptr()
        for x, y, name in zip(got, ref, ("idx", "z_q", "stats", "counts")):
            assert torch.equal(x, y), (k, n, name)
        assert int(_ctl(img, k).abs().max()) == 0
    cache.close()


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("which", ["commit", "codebook", "both", "neither"])
def test_vq_bwd_scalar_pointers_equal_the_stacked_pair(which, dtype):
    """N = 512, K = 64, d = 64: the two upstream scalars read where they lie (None: no gradient for that term) against the float32 [2]
    tensor that holds them, a zero in place of a missing one."""
    from frl_hip import ops
    n, k, d = 512, 64, 64
    g = _gen(11)
    z = torch.randn(n, d, generator=g).to(dtype).to(DEV)
    cb = torch.randn(k, d, generator=g).to(DEV)
    g_out = torch.randn(n, d, generator=g).to(dtype).to(DEV)
    idx, zq, _, counts = ops.vq_assign(z, cb)
    pool = torch.tensor([0.75, -3.0, 1.25, 7.0], device=DEV)          # the scalars are views into one tensor, not adjacent
    g_cm = pool[0] if which in ("commit", "both") else None
    g_cb = pool[2] if which in ("codebook", "both") else None
    stacked = torch.stack([torch.zeros((), device=DEV) if t is None else t for t in (g_cm, g_cb)])
    ref = ops.vq_bwd(g_out, z, cb, idx, counts, stacked, 0.25, zq=zq)
    got = ops.vq_bwd(g_out, z, cb, idx, counts, None, 0.25, zq=zq, scalars=(g_cm, g_cb))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), which
    if which == "neither":
        assert torch.equal(got[0], g_out) and int((got[1] != 0).sum()) == 0
    with pytest.raises(ValueError):
        ops.vq_bwd(g_out, z, cb, idx, counts, stacked, 0.25, zq=zq, scalars=(g_cm, g_cb))


# ---------------------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(freeze_codebook=False):
    from frl_hip.models import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=BF).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(64, 64, generator=_gen(7)))
    if freeze_codebook:
        m.quant.codebook.requires_grad_(False)
    return m


def _tiles(count, seed=13):
    g = _gen(seed)
    return [torch.randn(2, 5, 16, 16, 64, generator=g).to(BF).to(DEV) for _ in range(count)]


def _count_prepares(monkeypatch):
    from frl_hip import ops
    calls, real = [], ops.vq_prepare

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "vq_prepare", counting)
    return calls


def _assert_image_current(m, calls):
    """What the next forward would assign through the quantizer's cached image == through a fresh stand-alone image.  Returns the
    stand-alone prepares that `prepared()` launched to get there."""
    from frl_hip import ops
    q = m.quant
    cb = q.codebook.detach()
    z = torch.randn(512, 64, generator=_gen(99)).to(BF).to(DEV)
    before = len(calls)
    img = q.prepared(BF, 512)
    launched = len(calls) - before
    fresh = _fresh_image(cb, 512, BF)
    a, b = ops.vq_assign(z, cb, img), ops.vq_assign(z, cb, fresh)
    for x, y, name in zip(a, b, ("idx", "z_q", "stats", "counts")):
        assert torch.equal(x, y), name
    return launched


@pytest.mark.parametrize("event", ["none", "init_from_tiles", "copy_", "load_state_dict", "skipped_step", "frozen_codebook"])
def test_stale_image_is_never_used(event, monkeypatch):
    from frl_hip.training.trainer import VQVAETrainer
    tiles = _tiles(4)
    m = _model(freeze_codebook=event == "frozen_codebook")
    tr = VQVAETrainer(m, lr=1e-2, total_steps=10)
    tr.step(tiles[0])                                                # first step: the forward prepares on its own, the job is registered
    calls = _count_prepares(monkeypatch)
    tr.step(tiles[1])
    assert not calls, "a steady-state step launched a stand-alone vq_prepare"
    expect_fallback = True
    if event == "init_from_tiles":
        m.init_codebook_from_tiles(tiles[2], seed=5)
    elif event == "copy_":
        with torch.no_grad():
            m.quant.codebook.copy_(torch.randn(64, 64, generator=_gen(21)))
    elif event == "load_state_dict":
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        sd["quant.codebook"] = torch.randn(64, 64, generator=_gen(22)).to(DEV)
        m.load_state_dict(sd)
    elif event == "skipped_step":
        bad = tiles[2].clone()
        bad[0, 0, 0, 0, 0] = float("nan")
        cb0 = m.quant.codebook.detach().clone()
        tr.step(bad)
        assert tr.opt.applied_and_skipped[1] == 1 and torch.equal(m.quant.codebook.detach(), cb0)
        expect_fallback = False                                      # the job rewrote the image of the unchanged codebook
    else:
        expect_fallback = False
    assert bool(_assert_image_current(m, calls)) == expect_fallback, event
    tr.step(tiles[3])                                                # and the steps after it run on the job again
    del calls[:]
    tr.step(tiles[0])
    assert not calls
    assert _assert_image_current(m, calls) == 0


def _run_steps(monkeypatch, lean, graphed, tiles):
    from frl_hip.training.trainer import VQVAETrainer
    if lean:
        monkeypatch.delenv("FRL_HIP_DISABLE", raising=False)
    else:
        monkeypatch.setenv("FRL_HIP_DISABLE", "launches")
    m = _model()
    m.lean_step = lean
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    trace = []
    for t in tiles:
        out = tr.step_graphed(t) if graphed else tr.step(t)
        trace.append(dict(loss=out["loss"].detach().clone(), perplexity=out["perplexity"].detach().clone(), idx=out["idx"].clone(),
                          params=[p.detach().clone() for p in m.parameters()]))
    torch.cuda.synchronize()
    assert tr.opt.applied_and_skipped == (len(tiles), 0)
    return trace


def _same(a, b, what):
    for s, (x, y) in enumerate(zip(a, b)):
        for key in ("loss", "perplexity", "idx"):
            assert torch.equal(x[key], y[key]), (what, s, key)
        for i, (p, r) in enumerate(zip(x["params"], y["params"])):
            assert torch.equal(p, r), (what, s, i)


def test_step_is_the_same_with_and_without_the_framework_launches(monkeypatch):
    tiles = _tiles(3)
    on = _run_steps(monkeypatch, True, False, tiles)
    off = _run_steps(monkeypatch, False, False, tiles)
    _same(on, off, "switches on / off")
    graphed = _run_steps(monkeypatch, True, True, tiles)
    _same(graphed, on, "step_graphed / step")


def test_eager_step_issues_no_framework_launch():
    """One eager train step under torch.profiler: device events that are not kernels of the library (ATen kernels, memcpy, memset)."""
    from torch.profiler import ProfilerActivity, profile
    from frl_hip.training.trainer import VQVAETrainer
    tiles = _tiles(3)
    m = _model()
    m.concurrent_phase = False
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    tr.step(tiles[0])
    tr.step(tiles[1])
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        tr.step(tiles[2])
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    assert names, "torch.profiler reported no device events on this machine: the launch count cannot be checked here"
    foreign = [n for n in names if n.startswith("void at::") or "at::native" in n or n.startswith("Memcpy") or n.startswith("Memset")
               or "rocclr" in n]
    print(f"device events {len(names)}, not from the library {len(foreign)}: {sorted(set(foreign))}")
    assert not any("vq_prepare_kernel" in n for n in names)
    assert len(foreign) <= FRAMEWORK_LAUNCHES_LEFT, foreign
