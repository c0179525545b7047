"""Raw (non-autograd) Python bindings over the C ABI: torch tensors in, torch tensors out.

torch is used for device memory, the current stream and dtype bookkeeping only; every computation
below is a HIP kernel of libfrlhip.so.  All activation tensors are NHWC "rows": [..., C] contiguous.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F32, check  # noqa: F401

_WS = {}

# ----------------------------------------------------------------------------------------------
# optional per-op HIP-event timing (bench.py roofline): events are recorded on the stream the kernels are launched on
# ----------------------------------------------------------------------------------------------
_TIMING = {"on": False, "events": {}}


def set_timing(on: bool) -> None:
    _TIMING["on"] = bool(on)
    _TIMING["events"] = {}


def timing_summary():
    """name -> (calls, total_ms); synchronises the device."""
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in _TIMING["events"].items()}


def kernel_timing(on: bool) -> None:
    """Library-side HIP-event pair around every kernel launch (see include/frl_hip.h: frl_kernel_timing_enable)."""
    _lib.load().frl_kernel_timing_enable(1 if on else 0)


def kernel_timing_report():
    """kernel expression -> (calls, total_ms) since the last report; synchronises the recorded events."""
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.load().frl_kernel_timing_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, calls, ms = line.rsplit("\t", 2)
        out[name] = (int(calls), float(ms))
    return out


# ----------------------------------------------------------------------------------------------
# Index validation of the sparse ops (gathers, pair lists).  The reference's advanced indexing raises on an out-of-range index; the
# kernels take device pointers and would read out of bounds.  The Python wrappers therefore wrap negative indices, clamp the rest into
# range and OR "something was out of range" into a device flag without a host synchronisation; `index_errors()` reads it, and with
# FRL_HIP_CHECK_INDICES=1 the wrappers raise IndexError on the spot (one sync per call: debugging).
# ----------------------------------------------------------------------------------------------
_INDEX_FLAG = {}


def sanitize_indices(idx: torch.Tensor, n: int, what: str) -> torch.Tensor:
    """idx int64 (any shape) addressing n rows -> indices in [0, n): negatives wrapped as torch indexing does, out-of-range clamped and flagged."""
    import os
    bad = ((idx < -n) | (idx >= n)).any()
    flag = _INDEX_FLAG.get(idx.device)
    if flag is None:
        flag = _INDEX_FLAG[idx.device] = torch.zeros(1, dtype=torch.int32, device=idx.device)
    flag |= bad.to(torch.int32)
    if os.environ.get("FRL_HIP_CHECK_INDICES", "0") == "1" and bool(bad.item()):
        raise IndexError(f"{what}: index out of range for {n} rows")
    return torch.where(idx < 0, idx + n, idx).clamp_(0, max(n - 1, 0))


def index_errors(device=None, reset: bool = True) -> bool:
    """True when any sparse op since the last call saw an out-of-range index on `device` (all devices when None); synchronises."""
    hit = False
    for dev, flag in _INDEX_FLAG.items():
        if device is None or torch.device(device) == dev:
            hit |= bool(flag.item())
            if reset:
                flag.zero_()
    return hit


class PackCache:
    """Weight-image cache of a trainer (include/frl_hip.h: frl_pack_cache_*): the packed MFMA fragment images of the model's weights live
    in an arena owned by this object; `with cache:` makes the conv-like calls use them, `refresh()` rewrites all of them in one launch."""

    def __init__(self, device, nbytes: int = 64 << 20):
        lib = _lib.load()
        self.arena = torch.empty(int(nbytes) + lib.frl_pack_cache_table_bytes(), dtype=torch.uint8, device=device)
        self.handle = lib.frl_pack_cache_create(ctypes.c_void_p(self.arena.data_ptr()), self.arena.numel())
        if self.handle <= 0:
            check(self.handle, "frl_pack_cache_create")
        self._prev = 0
        self._quantizers = {}                               # (id(quantizer), image address, dtype) -> (quantizer, dtype, image, codebook)

    def add_quantizer(self, quantizer) -> bool:
        """The prepared codebook image of `quantizer` (models.vqvae.VectorQuantizer.prepared) becomes a job of refresh(): the launch that
        rewrites the weight images behind the optimizer writes norms, fragments and control block of the image too, with the arithmetic
        of `vq_prepare`, and refresh() then marks the image as current for the codebook version it read.  Needs an image to exist (one
        forward has run); False when there is none yet.  Registering again is free."""
        prep = quantizer._prepared
        if prep is None or prep[0][2] is None:
            return False
        dtype, buf, cb = prep[0][2], prep[1], quantizer.codebook
        key = (id(quantizer), buf.data_ptr(), cb.data_ptr(), dtype)
        if key not in self._quantizers:
            if cb.dtype != torch.float32 or not cb.is_contiguous() or cb.device != self.arena.device:
                return False
            if any(k[1] == key[1] for k in self._quantizers):   # one job per image: a second row dtype keeps the stand-alone prepare
                return False
            k, d = cb.shape
            check(_lib.load().frl_pack_cache_add_vq(self.handle, _p(cb), k, d, BF16 if dtype == torch.bfloat16 else F32, _p(buf), buf.numel()),
                  "frl_pack_cache_add_vq")
            self._quantizers[key] = (quantizer, dtype, buf, cb)
        return True

    def __enter__(self):
        self._prev = _lib.load().frl_pack_cache_activate(self.handle)
        return self

    def __exit__(self, *a):
        _lib.load().frl_pack_cache_activate(self._prev)
        return False

    def refresh(self) -> None:
        check(_lib.load().frl_pack_cache_refresh(self.handle, _stream()), "frl_pack_cache_refresh")
        for qz, dtype, buf, cb in self._quantizers.values():
            if qz._prepared is None or qz._prepared[1] is not buf:
                continue                                    # the quantizer moved on to another image: this job writes a buffer nobody reads
            # the launch read the codebook as it is now: the image is current for this version (any later in-place change bumps the
            # version and `prepared()` falls back to the stand-alone prepare).  A codebook that changed its storage since the
            # registration was NOT what the job read: the image is then unknown.
            same = qz.codebook is cb or qz.codebook.data_ptr() == cb.data_ptr()
            qz._prepared = ((cb.data_ptr(), qz.codebook._version, dtype) if same else (None, None, dtype), buf)

    @property
    def images(self) -> int:
        return _lib.load().frl_pack_cache_images(self.handle)

    def close(self) -> None:
        if self.handle > 0:
            _lib.load().frl_pack_cache_destroy(self.handle)
            self.handle = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class span:
    """with ops.span("name"): ...  -- HIP-event timing of a sub-range (used for single-kernel roofline numbers)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if _TIMING["on"]:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if _TIMING["on"]:
            self.e1.record()
            _TIMING["events"].setdefault(self.name, []).append((self.e0, self.e1))
        return False


def _timed(name):
    def deco(fn):
        def wrapper(*a, **kw):
            if not _TIMING["on"]:
                return fn(*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            _TIMING["events"].setdefault(name, []).append((e0, e1))
            return out
        wrapper.__name__ = fn.__name__
        wrapper.__doc__ = fn.__doc__
        return wrapper
    return deco


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"frl_hip supports float32 and bfloat16 activations, got {t.dtype}")


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk_rows(t: torch.Tensor, c: int, name: str):
    if not t.is_cuda:
        raise _lib.FrlHipError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if not t.is_contiguous() or t.shape[-1] != c:
        raise ValueError(f"{name}: expected contiguous [..., {c}] rows, got {tuple(t.shape)} stride {t.stride()}")


def _chk_like(t: torch.Tensor, ref: torch.Tensor, name: str):
    """An epilogue operand read at the addresses the kernel writes: same shape, dtype and device, contiguous, not the output itself."""
    if t.shape != ref.shape or t.dtype != ref.dtype or t.device != ref.device or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {tuple(ref.shape)} {ref.dtype} tensor on {ref.device}, got "
                         f"{tuple(t.shape)} {t.dtype} stride {t.stride()}")


def _f32(t: Optional[torch.Tensor], name: str):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{name}: parameters are passed as contiguous float32 CUDA tensors")
    return t


def _chk_f32_on(op: str, anchor: str, device, *operands):
    """Each (tensor, shape, name): a contiguous float32 tensor of exactly that shape on `device`, the device of the operand called `anchor`."""
    for t, shape, name in operands:
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
            raise ValueError(f"{op}: {name} must be a contiguous float32 {shape} tensor on the device of {anchor}")


def _chk_tensor_on(name: str, what: str, t: torch.Tensor, shape, dtype, device):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{name}: {what} must be a contiguous {dtype} {tuple(shape)} tensor on {device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


def _chk_one_device(name: str, first: torch.Tensor, *rest):
    """Every tensor given (None: skipped) lives on the GPU (FrlHipError) and on the device of the first (ValueError)."""
    for s in (first,) + rest:
        if s is not None and not s.is_cuda:
            raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
        if s is not None and s.device != first.device:
            raise ValueError(f"{name}: all tensors must be on one device")


MAX_WORKGROUPS = 4096   # gmm.hip, probe.hip, strata.hip: one slab per workgroup, in a workspace the caller owns


def chk_workgroups(name: str, workgroups: int, hint: str = " (0: the library's choice)"):
    if not 0 <= int(workgroups) <= MAX_WORKGROUPS:
        raise ValueError(f"{name}: workgroups must be in 0..{MAX_WORKGROUPS}{hint}, got {workgroups}")


def _owned_workspace(name: str, nbytes, device) -> torch.Tensor:
    """It carries partial sums from one call to the next: not the shared scratch buffer.  nbytes(lib) is asked once the device is a GPU."""
    if not torch.device(device).type == "cuda":
        raise _lib.FrlHipError(f"{name}: the device must be a GPU (no CPU fallback)")
    return torch.empty(max(nbytes(_lib.load()), 256), dtype=torch.uint8, device=device)


def _pair_outputs(b: int, width: int, device):
    """pairstat f32 [B, width], out2 f32 [2], stats f64 [8] of the pair losses (soft neighbourhood, spread ranking)."""
    return (torch.empty(b, width, dtype=torch.float32, device=device), torch.empty(2, dtype=torch.float32, device=device),
            torch.empty(8, dtype=torch.float64, device=device))


_DEFER = {"on": False, "keep": [], "dest": {}, "drop": set()}


class deferred_reductions:
    """`with deferred_reductions(params): loss.backward()` -- the slab reductions behind the weight-gradient kernels of the backward pass
    (csrc/defer.hip, include/frl_hip.h) are parked and run in ONE launch when the block ends, on the current stream.  While it is open every
    kernel call gets a workspace of its own (the parked slabs live in them), kept until the flush, and the storage of every gradient tensor
    the kernel wrappers allocate (`grad_empty`) is held until the flush as well, so that no parked destination can be freed and its address
    handed to another tensor.  Before the flush the block checks that every parked destination lies inside one of those held gradients,
    and that the gradient either was handed to `discard` (a gradient autograd drops: a frozen parameter) or is the .grad of one of `params`:
    autograd must have adopted the tensors the kernels' wrappers returned, not copies of them (a parameter used twice, a gradient
    accumulated into an existing .grad, or a hook that clones gradients, would read a tensor nothing has written yet).  When the check
    fails, autograd has already summed or copied the unwritten gradient: the .grad of the parameters involved is invalid and must be zeroed
    (or set to None) before the backward is repeated without deferral.  The held gradients are marked as used on the current stream, so
    that one allocated on a side stream is not reused before the flush has written it."""

    def __init__(self, params):
        self.params = list(params)

    def __enter__(self):
        check(_lib.load().frl_defer_begin(), "frl_defer_begin")
        _DEFER.update(keep=[], dest={}, drop=set(), on=True)
        return self

    def __exit__(self, et, ev, tb):
        lib = _lib.load()
        _DEFER["on"] = False
        keep, dest, drop = _DEFER["keep"], _DEFER["dest"], _DEFER["drop"]
        _DEFER.update(keep=[], dest={}, drop=set())
        if et is not None:
            lib.frl_defer_abort()
            return False
        try:
            import bisect
            buf = (ctypes.c_void_p * 512)()
            n = lib.frl_defer_destinations(ctypes.cast(buf, ctypes.c_void_p), 512)
            held = sorted((a, a + s.nbytes()) for a, s in dest.items())
            spans = sorted((g.data_ptr(), g.data_ptr() + g.numel() * g.element_size())
                           for g in (p.grad for p in self.params) if g is not None)
            for i in range(n):
                d = int(buf[i])
                k = bisect.bisect_right(held, (d, float("inf"))) - 1
                if k < 0 or not (held[k][0] <= d < held[k][1]):
                    raise RuntimeError("deferred_reductions: a parked gradient was not allocated by the kernel wrappers inside this block")
                if held[k][0] in drop:
                    continue
                k = bisect.bisect_right(spans, (d, float("inf"))) - 1
                if k < 0 or not (spans[k][0] <= d < spans[k][1]):
                    raise RuntimeError("deferred_reductions: a parked gradient is not the .grad of any parameter (autograd copied or summed "
                                       "it: a parameter used twice, a gradient accumulated into an existing .grad, or a gradient hook); "
                                       "the .grad of the parameters involved is now invalid: zero it, then run this backward without deferral")
        except Exception:
            lib.frl_defer_abort()
            raise
        rc = lib.frl_defer_flush(_stream())
        if rc < 0:
            check(rc, "frl_defer_flush")
        cur = torch.cuda.current_stream()
        for t in keep:                                          # slabs written on a side stream, read by the flush on this one
            t.record_stream(cur)
        for st in dest.values():                                # gradients written by the flush: not reused before it has run
            torch.empty(0, dtype=torch.uint8, device=cur.device).set_(st).record_stream(cur)
        return False


def grad_empty(shape, device) -> torch.Tensor:
    """A float32 parameter-gradient tensor for a weight-gradient kernel to fill.  Inside `deferred_reductions` its STORAGE is held until the
    flush (not the tensor: an extra reference to the tensor would make autograd clone it instead of adopting it as the .grad)."""
    g = torch.empty(shape, dtype=torch.float32, device=device)
    if _DEFER["on"]:
        st = g.untyped_storage()
        _DEFER["dest"][st.data_ptr()] = st
    return g


def discard(*grads) -> None:
    """Gradients a kernel computed that autograd will not receive (the parameter is frozen, and the kernel has no way to skip them): inside
    `deferred_reductions` their parked reductions still write them at the flush; they stay held and are exempt from the .grad check.  Only
    gradients that `grad_empty` allocated in this block are exempted (both are alive, so an equal address is the same storage); others
    are never parked and need nothing."""
    if _DEFER["on"]:
        for g in grads:
            if g is not None and g.untyped_storage().data_ptr() in _DEFER["dest"]:
                _DEFER["drop"].add(g.untyped_storage().data_ptr())


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only per-(device, stream) scratch buffer handed to kernels that need one (inside `deferred_reductions`: a buffer per call)."""
    if _DEFER["on"]:
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
        _DEFER["keep"].append(ws)
        return ws
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _WS[key] = ws
    return ws


# ----------------------------------------------------------------------------------------------
# pointwise convolution (reference: nn.Conv2d(.,.,1) call sites, see csrc/pw_conv.hip)
# ----------------------------------------------------------------------------------------------
@_timed("conv1x1_fwd")
def conv1x1_fwd(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int = ACT_NONE) -> torch.Tensor:
    cout, cin = w.shape[0], w.shape[1]
    _chk_rows(x, cin, "conv1x1_fwd.x")
    w = _f32(w.reshape(cout, cin), "w")
    y = torch.empty(x.shape[:-1] + (cout,), dtype=x.dtype, device=x.device)
    p = x.numel() // cin
    lib = _lib.load()
    ws = workspace(lib.frl_conv_workspace_bytes(cin, cout, 1), x.device)
    check(lib.frl_conv1x1_fwd(_p(x), _p(w), _p(_f32(bias, "bias")), _p(y), p, cin, cout, act, _dt(x), _p(ws), ws.numel(),
                              _stream()), "frl_conv1x1_fwd")
    return y


@_timed("conv1x1_bwd_data")
def conv1x1_bwd_data(dy: torch.Tensor, w: torch.Tensor, y: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                     add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = (dy .* act'(y)) W (+ add: a second gradient stream of x, accumulated in the kernel's epilogue)."""
    cout, cin = w.shape[0], w.shape[1]
    _chk_rows(dy, cout, "conv1x1_bwd_data.dy")
    w = _f32(w.reshape(cout, cin), "w")
    dx = torch.empty(dy.shape[:-1] + (cin,), dtype=dy.dtype, device=dy.device)
    p = dy.numel() // cout
    lib = _lib.load()
    ws = workspace(lib.frl_conv_workspace_bytes(cin, cout, 1), dy.device)
    if add is not None:
        _chk_like(add, dx, "conv1x1_bwd_data.add")
        check(lib.frl_conv1x1_bwd_data_add(_p(dy), _p(y), act, _p(w), _p(dx), _p(add), p, cin, cout, _dt(dy), _p(ws), ws.numel(),
                                           _stream()), "frl_conv1x1_bwd_data_add")
        return dx
    check(lib.frl_conv1x1_bwd_data(_p(dy), _p(y), act, _p(w), _p(dx), p, cin, cout, _dt(dy), _p(ws), ws.numel(), _stream()),
          "frl_conv1x1_bwd_data")
    return dx


def _conv1x1_bwd_weight_impl(dy: torch.Tensor, x: torch.Tensor, y: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                       want_bias: bool = True, scalar_frags: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    cout, cin = dy.shape[-1], x.shape[-1]
    _chk_rows(dy, cout, "bwd_weight.dy")
    _chk_rows(x, cin, "bwd_weight.x")
    p = dy.numel() // cout
    lib = _lib.load()
    nbytes = lib.frl_conv1x1_bwd_weight_workspace_bytes(p, cin, cout)
    ws = workspace(nbytes, dy.device)
    dw = grad_empty((cout, cin), dy.device)
    db = grad_empty((cout,), dy.device) if want_bias else None
    check(lib.frl_conv_tap_bwd_weight(_p(dy), _p(y), act, _p(x), _p(dw), cin, 1, _p(db), p, cin, cout, 1, 1, 0,
                                      _dt(dy), _p(ws), ws.numel(), 1 if scalar_frags else 0, _stream()),
          "frl_conv_tap_bwd_weight")
    return dw, db


conv1x1_bwd_weight = _timed("conv1x1_bwd_weight")(_conv1x1_bwd_weight_impl)


def wgrad_thin(on: bool) -> bool:
    """A/B hook (include/frl_hip.h: frl_wgrad_thin): True (default) = eligible thin-output bf16 weight gradients (the 64 -> 12 phase head)
    take the streaming kernel, False = every call takes the generic kernel; same bits.  Returns the previous setting."""
    return bool(_lib.load().frl_wgrad_thin(1 if on else 0))


# ----------------------------------------------------------------------------------------------
# vector quantizer (csrc/vq.hip)
# ----------------------------------------------------------------------------------------------
def vq_stream_tiles(nt: int) -> int:
    """A/B hook (include/frl_hip.h: frl_vq_stream_tiles): tiles per wave and batch of the streaming assignment kernel, 0 = the resident
    kernel, -1 = default.  Returns the previous setting."""
    return int(_lib.load().frl_vq_stream_tiles(int(nt)))


@_timed("vq_prepare")
def vq_prepare(codebook: torch.Tensor, n_rows: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prepared image of the codebook (norms + packed MFMA fragments) for `vq_assign(..., prep=)`; valid until the codebook changes."""
    k, d = codebook.shape
    cb = _f32(codebook, "codebook")
    lib = _lib.load()
    nbytes = lib.frl_vq_prepared_bytes(k, d)
    if out is None or out.numel() < nbytes or out.device != cb.device:
        out = torch.empty(nbytes, dtype=torch.uint8, device=cb.device)
    check(lib.frl_vq_prepare(_p(cb), int(n_rows), k, d, BF16 if dtype == torch.bfloat16 else F32, _p(out), out.numel(), _stream()),
          "frl_vq_prepare")
    return out


@_timed("vq_assign")
def vq_assign(z: torch.Tensor, codebook: torch.Tensor, prep: Optional[torch.Tensor] = None, stats_copy: bool = False):
    """z [N,d] rows, codebook [K,d] f32 -> (idx int32 [N], z_q [N,d], stats f32 [4], counts int32 [K]).
    prep: image from `vq_prepare` for this codebook content and z.dtype (None: built inside the call).
    stats_copy: a fifth result, a second float32 [4] tensor with the bits of `stats`, stored by the kernel that writes `stats` (what
    `stats.clone()` gives, without the copy launch)."""
    k, d = codebook.shape
    _chk_rows(z, d, "vq_assign.z")
    cb = _f32(codebook, "codebook")
    n = z.numel() // d
    lib = _lib.load()
    ws = workspace(lib.frl_vq_workspace_bytes(n, k, d), z.device)
    idx = torch.empty(n, dtype=torch.int32, device=z.device)
    zq = torch.empty_like(z)
    stats = torch.empty(4, dtype=torch.float32, device=z.device)
    counts = torch.empty(k, dtype=torch.int32, device=z.device)
    if prep is not None and (prep.dtype != torch.uint8 or prep.device != z.device or prep.numel() < lib.frl_vq_prepared_bytes(k, d)):
        raise ValueError("vq_assign: prep is not a prepared-codebook image for this codebook")
    if stats_copy:
        stats2 = torch.empty(4, dtype=torch.float32, device=z.device)
        check(lib.frl_vq_assign_fwd_stats2(_p(z), _p(cb), _p(prep), n, k, d, _p(idx), _p(zq), _p(stats), _p(stats2), _p(counts), _dt(z), _p(ws),
                                           ws.numel(), _stream()), "frl_vq_assign_fwd")
        return idx, zq, stats, counts, stats2
    check(lib.frl_vq_assign_fwd_prepared(_p(z), _p(cb), _p(prep), n, k, d, _p(idx), _p(zq), _p(stats), _p(counts), _dt(z), _p(ws),
                                         ws.numel(), _stream()), "frl_vq_assign_fwd")
    return idx, zq, stats, counts


@_timed("vq_bwd")
def vq_bwd(g_out: Optional[torch.Tensor], z: torch.Tensor, codebook: torch.Tensor, idx: torch.Tensor,
           counts: torch.Tensor, gscale: Optional[torch.Tensor], beta: float, want_gz: bool = True,
           want_ge: bool = True, want_sums: bool = False, zq: Optional[torch.Tensor] = None, scalars=None):
    """g_z = g_out + gscale[0] beta 2/(N d) (z - e_idx), g_E = gscale[1] 2/(N d) (n_k e_k - S_k), S_k = per-code sums of z.  The kernels
    read every operand as raw rows of z's dtype / int32 / float32, so anything else is refused here, before the launch.
    scalars = (g_commit, g_codebook) instead of gscale: the two upstream gradients as separate float32 device scalars, read where they
    lie (no stacking launch); a None entry means that no gradient arrives for that term (the bits a zero scalar gives)."""
    if codebook.dim() != 2:
        raise ValueError(f"vq_bwd: codebook must be [K, d], got {tuple(codebook.shape)}")
    k, d = codebook.shape
    if not z.is_cuda:
        raise ValueError("vq_bwd.z: tensor must live on the GPU (no CPU fallback)")
    if z.dim() < 1 or z.shape[-1] != d or not z.is_contiguous():
        raise ValueError(f"vq_bwd.z: expected contiguous [..., {d}] rows, got {tuple(z.shape)} stride {z.stride()}")
    n = z.numel() // d
    if g_out is not None:
        _chk_like(g_out, z, "vq_bwd.g_out")
    if zq is not None:
        _chk_like(zq, z, "vq_bwd.zq")
    for t, m, name in ((idx, n, "idx"), (counts, k, "counts")):
        if t.dtype != torch.int32 or t.numel() != m or not t.is_contiguous() or t.device != z.device:
            raise ValueError(f"vq_bwd.{name}: expected a contiguous int32 tensor of {m} elements on {z.device}, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
    if gscale is not None and (gscale.dtype != torch.float32 or gscale.device != z.device or gscale.numel() < 2
                               or not gscale.is_contiguous()):
        raise ValueError("vq_bwd.gscale: expected a contiguous float32 tensor of at least 2 elements on the device of z")
    if codebook.device != z.device:
        raise ValueError("vq_bwd: codebook and z live on different devices")
    if scalars is not None:
        if gscale is not None or len(scalars) != 2:
            raise ValueError("vq_bwd: scalars is a pair (g_commit, g_codebook) and replaces gscale")
        for s in scalars:
            if s is not None and (s.dtype != torch.float32 or s.device != z.device or s.numel() != 1):
                raise ValueError("vq_bwd.scalars: expected float32 scalars on the device of z (or None)")
    lib = _lib.load()
    ws = workspace(lib.frl_vq_workspace_bytes(n, k, d), z.device)
    gz = torch.empty_like(z) if want_gz else None
    ge = grad_empty((k, d), z.device) if want_ge else None
    sums = torch.empty(k, d, dtype=torch.float32, device=z.device) if want_sums else None
    cb32 = _f32(codebook, "codebook")
    if _DEFER["on"]:                                            # the parked codebook-gradient reduction reads these when the flush runs
        _DEFER["keep"] += [t for t in (counts, gscale, cb32) + tuple(scalars or ()) if t is not None]
    if scalars is not None:
        check(lib.frl_vq_bwd_scalars(_p(g_out), _p(z), _p(zq), _p(cb32), _p(idx), _p(counts), _p(scalars[0]), _p(scalars[1]), float(beta),
                                     n, k, d, _p(gz), _p(ge), _p(sums), _dt(z), _p(ws), ws.numel(), _stream()), "frl_vq_bwd_scalars")
        return gz, ge, sums
    check(lib.frl_vq_bwd(_p(g_out), _p(z), _p(zq), _p(cb32), _p(idx), _p(counts), _p(gscale), float(beta),
                         n, k, d, _p(gz), _p(ge), _p(sums), _dt(z), _p(ws), ws.numel(), _stream()), "frl_vq_bwd")
    return gz, ge, sums


def vq_ema_update(sums, counts, ema_count, ema_sum, codebook, decay: float, eps: float, ok: Optional[torch.Tensor] = None):
    """EMA codebook update in place; `ok` (device float [1]) <= 0 skips it on the device (isfinite guard, no host sync)."""
    k, d = codebook.shape
    if ok is not None and (ok.dtype != torch.float32 or not ok.is_cuda or ok.numel() < 1):
        raise ValueError("vq_ema_update: ok must be a float32 CUDA tensor")
    check(_lib.load().frl_vq_ema_update(_p(sums), _p(counts), k, d, float(decay), float(eps), _p(ema_count),
                                        _p(ema_sum), _p(codebook), _p(ok), _stream()), "frl_vq_ema_update")


# ----------------------------------------------------------------------------------------------
# GroupNorm over NHWC rows (csrc/norm.hip)
# ----------------------------------------------------------------------------------------------
def _mult_ptrs(mults, n):
    if mults is None or all(m is None for m in mults):
        return None
    for m in mults:
        if m is not None and (m.dtype != torch.float32 or m.numel() != 1 or not m.is_cuda):
            raise ValueError("scalar_combine: multipliers are float32 CUDA scalars")
    return (ctypes.c_void_p * n)(*[0 if m is None else m.data_ptr() for m in mults])


def scalar_combine(terms, coefs, mults=None, aux_coefs=None):
    """[device float scalars], [host floats](, [device float scalars | None]) -> (value [] f32 = sum coef_i * mult_i * term_i, ok [1] f32 = 1.0 if
    the value is finite else 0.0[, aux [] f32 = sum aux_coef_i * term_i]).  A multiplier is read on the device at run time (a scheduled loss
    weight inside a captured graph); aux_coefs adds a second combination of the same terms to the launch (a reported sub-total)."""
    n = len(terms)
    dev = terms[0].device
    for t in terms:
        if t.dtype != torch.float32 or t.numel() != 1 or not t.is_cuda:
            raise ValueError("scalar_combine: terms are float32 CUDA scalars")
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in terms])
    cf = (ctypes.c_float * n)(*[float(c) for c in coefs])
    out = torch.empty((), dtype=torch.float32, device=dev)
    ok = torch.empty(1, dtype=torch.float32, device=dev)
    if aux_coefs is None:
        check(_lib.load().frl_scalar_combine_dev(ptrs, cf, _mult_ptrs(mults, n), n, _p(out), _p(ok), _stream()), "frl_scalar_combine")
        return out, ok
    ac = (ctypes.c_float * n)(*[float(c) for c in aux_coefs])
    aux = torch.empty((), dtype=torch.float32, device=dev)
    check(_lib.load().frl_scalar_combine_aux(ptrs, cf, _mult_ptrs(mults, n), ac, n, _p(out), _p(ok), _p(aux), _stream()), "frl_scalar_combine_aux")
    return out, ok, aux


def scalar_fanout(g, coefs, mults=None, promises=None):
    """g device float scalar -> out [n] f32 with out[i] = g * coef_i (* mult_i).  promises: per term None or the device float scalar the
    term's gradient was promised to equal at forward time (decoder_mse_fwd_bwd); a mismatch raises the flag behind `grad_scale_errors()`."""
    n = len(coefs)
    cf = (ctypes.c_float * n)(*[float(c) for c in coefs])
    out = torch.empty(n, dtype=torch.float32, device=g.device)
    if promises is None or all(p is None for p in promises):
        check(_lib.load().frl_scalar_fanout_dev(_p(g), cf, _mult_ptrs(mults, n), n, _p(out), _stream()), "frl_scalar_fanout")
        return out
    for p in promises:
        if p is not None and (p.dtype != torch.float32 or p.numel() != 1 or p.device != g.device):
            raise ValueError("scalar_fanout: promises are float32 scalars on the gradient's device")
    pp = (ctypes.c_void_p * n)(*[0 if p is None else p.data_ptr() for p in promises])
    check(_lib.load().frl_scalar_fanout_guard(_p(g), cf, _mult_ptrs(mults, n), pp, n, _p(out), _p(_grad_scale_flag(g.device)), _stream()),
          "frl_scalar_fanout_guard")
    return out


# ----------------------------------------------------------------------------------------------
# The promise behind the one-pass decoder loss (decoder_mse_fwd_bwd): its gradients are computed in the forward with the upstream
# gradient the caller announced.  The backward compares what arrives with the promise on the device (inside the launch that computes the
# term gradients: no extra launch, no host sync) and raises a sticky per-device flag; `grad_scale_errors()` reads it where the host
# synchronises anyway (the trainer's logging path), as `index_errors()` does for the sparse ops.
# ----------------------------------------------------------------------------------------------
_GRAD_SCALE_FLAG = {}


def _grad_scale_flag(device) -> torch.Tensor:
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    flag = _GRAD_SCALE_FLAG.get(device)
    if flag is None:
        flag = _GRAD_SCALE_FLAG[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return flag


def grad_scale_errors(device=None, reset: bool = True) -> bool:
    """True when a loss computed with a promised upstream gradient (decoder_mse(..., grad_scale=)) received another one in a backward since
    the last call on `device` (all devices when None): the gradients of that backward are wrongly scaled.  Synchronises."""
    hit = False
    for dev, flag in _GRAD_SCALE_FLAG.items():
        if device is None or torch.device(device) == dev:
            hit |= bool(flag.item())
            if reset:
                flag.zero_()
    return hit


def check_grad_scale(device=None) -> None:
    """Raises when `grad_scale_errors()` reports a broken promise (and clears the flag)."""
    if grad_scale_errors(device):
        raise RuntimeError("decoder_mse: a loss whose gradients were computed in the forward for a promised upstream gradient (grad_scale) "
                           "received a different one in the backward -- the decoder gradients of that step are wrongly scaled.  Scale the "
                           "loss through the promised coefficient, or switch the one-pass path off (VQVAE.onepass_decoder = False)")


def encoder2_supported(c0: int, c1: int, c2: int, g1: int, g2: int, hw: int, dtype) -> bool:
    return bool(_lib.load().frl_encoder2_supported(c0, c1, c2, g1, g2, hw, 1 if dtype == torch.bfloat16 else 0))


@_timed("encoder2_fwd")
def encoder2_fwd(x, w1, g1, b1, w2, g2, b2, eps: float = 1e-5):
    """Fused conv1x1 -> GroupNorm -> ReLU -> conv1x1 -> GroupNorm (csrc/enc_fused.hip).  x [B, ..., 64] bf16 -> (z, stats [B, 32])."""
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    _chk_rows(x, c, "encoder2.x")
    lib = _lib.load()
    z = torch.empty(x.shape[:-1] + (w2.shape[0],), dtype=x.dtype, device=x.device)
    stats = torch.empty(b, 32, dtype=torch.float32, device=x.device)
    ws = workspace(lib.frl_encoder2_workspace_bytes(b), x.device)
    check(lib.frl_encoder2_fwd(_p(x), _p(_f32(w1, "w1")), _p(_f32(g1, "g1")), _p(_f32(b1, "b1")), _p(_f32(w2, "w2")), _p(_f32(g2, "g2")),
                               _p(_f32(b2, "b2")), _p(z), _p(stats), b, hw, float(eps), _p(ws), ws.numel(), _stream()), "frl_encoder2_fwd")
    return z, stats


@_timed("encoder2_bwd")
def encoder2_bwd(x, dz, w1, g1, b1, w2, g2, b2, stats):
    """-> (dw1, dg1, db1, dw2, dg2, db2): parameter gradients of the fused encoder (its input is data: no dx)."""
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    lib = _lib.load()
    dw1, dg1, db1, dw2, dg2, db2 = (grad_empty(t.shape, x.device) for t in (w1, g1, b1, w2, g2, b2))
    ws = workspace(lib.frl_encoder2_workspace_bytes(b), x.device)
    check(lib.frl_encoder2_bwd(_p(x), _p(dz), _p(_f32(w1, "w1")), _p(g1), _p(b1), _p(_f32(w2, "w2")), _p(g2), _p(b2), _p(stats), _p(dw1), _p(dg1),
                               _p(db1), _p(dw2), _p(dg2), _p(db2), b, hw, _p(ws), ws.numel(), _stream()), "frl_encoder2_bwd")
    return dw1, dg1, db1, dw2, dg2, db2


@_timed("groupnorm_fwd")
def groupnorm_fwd(x: torch.Tensor, gamma, beta, groups: int, eps: float = 1e-5, relu: bool = False):
    """x [B, ..., C] -> (y, mean [B,G], rstd [B,G])."""
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    _chk_rows(x, c, "groupnorm.x")
    y = torch.empty_like(x)
    mean = torch.empty(b, groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    check(_lib.load().frl_groupnorm_fwd(_p(x), _p(_f32(gamma, "gamma")), _p(_f32(beta, "beta")), _p(y), _p(mean), _p(rstd),
                                        b, hw, c, groups, float(eps), int(relu), _dt(x), _stream()), "frl_groupnorm_fwd")
    return y, mean, rstd


@_timed("groupnorm_bwd")
def groupnorm_bwd(dy, x, gamma, beta, mean, rstd, groups: int, relu: bool = False):
    b, c = x.shape[0], x.shape[-1]
    hw = x.numel() // (b * c)
    lib = _lib.load()
    ws = workspace(lib.frl_groupnorm_bwd_workspace_bytes(b, c, groups), x.device)
    dx = torch.empty_like(x)
    dg = torch.empty(c, dtype=torch.float32, device=x.device)
    db = torch.empty(c, dtype=torch.float32, device=x.device)
    check(lib.frl_groupnorm_bwd(_p(dy), _p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), b, hw, c,
                                groups, int(relu), _dt(x), _p(ws), ws.numel(), _stream()), "frl_groupnorm_bwd")
    return dx, dg, db


# ----------------------------------------------------------------------------------------------
# streaming elementwise ops (csrc/elementwise.hip)
# ----------------------------------------------------------------------------------------------
@_timed("mse_fwd")
def mse_fwd(pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Returns stats f32 [2] = {mean squared error over valid elements, number of valid elements}."""
    c = pred.shape[-1]
    _chk_rows(pred, c, "mse.pred")
    _chk_rows(target, c, "mse.target")
    lib = _lib.load()
    ws = workspace(lib.frl_mse_workspace_bytes(), pred.device)
    out = torch.empty(2, dtype=torch.float32, device=pred.device)
    check(lib.frl_mse_fwd(_p(pred), _p(target), _p(mask), pred.numel() // c, c, _p(out), _dt(pred), _p(ws), ws.numel(),
                          _stream()), "frl_mse_fwd")
    return out


@_timed("mse_bwd")
def mse_bwd(pred, target, mask, gscale: Optional[torch.Tensor], stats) -> torch.Tensor:
    c = pred.shape[-1]
    d = torch.empty_like(pred)
    check(_lib.load().frl_mse_bwd(_p(pred), _p(target), _p(mask), _p(gscale), _p(stats), pred.numel() // c, c, _p(d),
                                  _dt(pred), _stream()), "frl_mse_bwd")
    return d


@_timed("film_modulate_fwd")
def film_modulate_fwd(h: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    """h [B,T,HW..,C], gamma/beta [B,HW..,C]."""
    b, t, c = h.shape[0], h.shape[1], h.shape[-1]
    hw = h.numel() // (b * t * c)
    out = torch.empty_like(h)
    check(_lib.load().frl_film_modulate_fwd(_p(h), _p(gamma), _p(beta), _p(out), b, t, hw, c, _dt(h), _stream()),
          "frl_film_modulate_fwd")
    return out


@_timed("film_modulate_bwd")
def film_modulate_bwd(dout, h, gamma):
    b, t, c = h.shape[0], h.shape[1], h.shape[-1]
    hw = h.numel() // (b * t * c)
    dh = torch.empty_like(h)
    dg = torch.empty_like(gamma)
    db = torch.empty_like(gamma)
    check(_lib.load().frl_film_modulate_bwd(_p(dout), _p(h), _p(gamma), _p(dh), _p(dg), _p(db), b, t, hw, c, _dt(h),
                                            _stream()), "frl_film_modulate_bwd")
    return dh, dg, db


def film_fused_supported(z_type: torch.Tensor, h: torch.Tensor, hidden: int) -> bool:
    """True when the FiLM nets and the modulation run as one launch per direction (csrc/film_fused.hip): bf16, 64 -> 32 -> 12."""
    return bool(z_type.is_cuda and h.dim() >= 3 and fusion_enabled("film") and _lib.load().frl_film_fused_supported(z_type.shape[-1], hidden, h.shape[-1], _dt(h))
                and z_type.dtype == h.dtype)


def _film_params(params):
    """(w1g, b1g, w2g, b2g, w1b, b1b, w2b, b2b) float32 parameters of FiLMLayer.gamma_network / beta_network"""
    if len(params) != 8:
        raise ValueError("film_fused: expected (w1g, b1g, w2g, b2g, w1b, b1b, w2b, b2b)")
    return [_p(_f32(t, "film parameter")) for t in params]


@_timed("film_fused_fwd")
def film_fused_fwd(z_type: torch.Tensor, h: torch.Tensor, params):
    """z_type [B,HW..,64], h [B,T,HW..,12] -> (z = gamma * h + beta, gamma [B,HW..,12], beta)."""
    b, t, c = h.shape[0], h.shape[1], h.shape[-1]
    hw = h.numel() // (b * t * c)
    _chk_rows(z_type, z_type.shape[-1], "film_fused_fwd.z_type")
    _chk_rows(h, c, "film_fused_fwd.h")
    if z_type.numel() // z_type.shape[-1] != b * hw:
        raise ValueError("film_fused_fwd: z_type must hold one row per (sample, pixel) of h")
    lib = _lib.load()
    ws = workspace(lib.frl_film_fused_workspace_bytes(), h.device)
    z = torch.empty_like(h)
    gamma = torch.empty(tuple(z_type.shape[:-1]) + (c,), dtype=h.dtype, device=h.device)
    beta = torch.empty_like(gamma)
    check(lib.frl_film_fused_fwd(_p(z_type), _p(h), *_film_params(params), _p(z), _p(gamma), _p(beta), b, t, hw, _p(ws), ws.numel(), _stream()),
          "frl_film_fused_fwd")
    return z, gamma, beta


@_timed("film_fused_bwd")
def film_fused_bwd(z_type: torch.Tensor, h: torch.Tensor, dz: torch.Tensor, params):
    """-> (dh, [dw1g, db1g, dw2g, db2g, dw1b, db1b, dw2b, db2b])"""
    b, t, c = h.shape[0], h.shape[1], h.shape[-1]
    hw = h.numel() // (b * t * c)
    _chk_like(dz, h, "film_fused_bwd.dz")
    lib = _lib.load()
    ws = workspace(lib.frl_film_fused_workspace_bytes(), h.device)
    dh = torch.empty_like(h)
    grads = [grad_empty(p.shape, h.device) for p in params]
    check(lib.frl_film_fused_bwd(_p(z_type), _p(h), _p(dz), *_film_params(params), _p(dh), *[_p(g) for g in grads], b, t, hw, _p(ws), ws.numel(),
                                 _stream()), "frl_film_fused_bwd")
    return dh, grads


@_timed("gate_blend_fwd")
def gate_blend_fwd(smoothed, residual, gate_raw, min_gate: float):
    out = torch.empty_like(smoothed)
    gate = torch.empty_like(smoothed)
    check(_lib.load().frl_gate_blend_fwd(_p(smoothed), _p(residual), _p(gate_raw), float(min_gate), _p(out), _p(gate),
                                         smoothed.numel(), _dt(smoothed), _stream()), "frl_gate_blend_fwd")
    return out, gate


@_timed("gate_blend_bwd")
def gate_blend_bwd(dout, dgate_ext, residual, gate_raw, min_gate: float, sigmoid_mask: bool = False, want_dres: bool = True):
    """-> (d residual, d gate_raw); sigmoid_mask: d gate_raw comes back multiplied by gate_raw (1 - gate_raw) (gradient w.r.t. the pre-activation).
    want_dres=False: d residual is neither stored nor returned (None): conv3x3_bwd_data(gate=...) forms it in its epilogue."""
    dres = torch.empty_like(dout) if want_dres else None
    dgraw = torch.empty_like(dout)
    check(_lib.load().frl_gate_blend_bwd_masked(_p(dout), _p(dgate_ext), _p(residual), _p(gate_raw), float(min_gate), _p(dres),
                                                _p(dgraw), dout.numel(), _dt(dout), int(sigmoid_mask), _stream()), "frl_gate_blend_bwd_masked")
    return dres, dgraw


@_timed("mean_time")
def mean_time(tile: torch.Tensor) -> torch.Tensor:
    """tile [B,T,H,W,C] -> [B,H,W,C]."""
    b, t = tile.shape[0], tile.shape[1]
    out = torch.empty((b,) + tuple(tile.shape[2:]), dtype=tile.dtype, device=tile.device)
    check(_lib.load().frl_mean_time_fwd(_p(tile), _p(out), b, t, out.numel() // b, _dt(tile), _stream()), "frl_mean_time_fwd")
    return out


@_timed("vq_revive_dead_codes")
def vq_revive_dead_codes(codebook: torch.Tensor, window_counts: torch.Tensor, min_count: int, z_rows: torch.Tensor, seed: int,
                         exp_avg: Optional[torch.Tensor] = None, exp_avg_sq: Optional[torch.Tensor] = None,
                         revived: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: codebook[k] = z_rows[splitmix64(seed + k) % N] for every code with window_counts[k] < min_count; clears the AdamW
    moment rows of those codes; returns the device int32 counter `revived` (incremented).  No host synchronisation."""
    k, d = codebook.shape
    if codebook.dtype != torch.float32 or not codebook.is_contiguous():
        raise ValueError("vq_revive_dead_codes: codebook must be contiguous float32 [K, d]")
    if window_counts.dtype != torch.int64 or window_counts.numel() != k or window_counts.device != codebook.device:
        raise ValueError("vq_revive_dead_codes: window_counts must be int64 [K] on the codebook's device")
    if z_rows.dim() != 2 or z_rows.shape[1] != d or not z_rows.is_contiguous() or z_rows.device != codebook.device:
        raise ValueError("vq_revive_dead_codes: z_rows must be contiguous [N, d] on the codebook's device")
    for mom in (exp_avg, exp_avg_sq):
        if mom is not None and (mom.dtype != torch.float32 or mom.shape != codebook.shape or not mom.is_contiguous()):
            raise ValueError("vq_revive_dead_codes: AdamW moments must match the codebook")
    if revived is None:
        revived = torch.zeros(1, dtype=torch.int32, device=codebook.device)
    check(_lib.load().frl_vq_revive_dead_codes(_p(codebook), _p(window_counts), int(min_count), _p(z_rows), z_rows.shape[0], k, d,
                                               int(seed) & 0xFFFFFFFFFFFFFFFF, _p(exp_avg), _p(exp_avg_sq), _p(revived), _dt(z_rows),
                                               _stream()), "frl_vq_revive_dead_codes")
    return revived


@_timed("mutual_knn")
def mutual_knn(features: torch.Tensor, patch_id: torch.Tensor, coords: torch.Tensor, k: int, pos_min_spatial: float):
    """features [N, D] float32, patch_id [N] int32, coords [N, 2] float32 -> (knn_idx [N, k] int32, mutual [N, k] uint8)."""
    n, d = features.shape
    if features.dtype != torch.float32 or not features.is_contiguous():
        raise ValueError("mutual_knn: features must be contiguous float32 [N, D]")
    if patch_id.dtype != torch.int32 or patch_id.numel() != n or coords.dtype != torch.float32 or tuple(coords.shape) != (n, 2) \
            or not coords.is_contiguous() or not patch_id.is_contiguous():
        raise ValueError("mutual_knn: patch_id must be int32 [N], coords float32 [N, 2]")
    if d % 16 or d > 256:
        if d > 256:
            raise ValueError("mutual_knn: at most 256 feature channels")
        # zero columns add exactly nothing to a squared distance (and leave the summation order of the real ones untouched)
        features = torch.nn.functional.pad(features, (0, (-d) % 16)).contiguous()
        d = features.shape[1]
    knn = torch.empty((n, k), dtype=torch.int32, device=features.device)
    mutual = torch.empty((n, k), dtype=torch.uint8, device=features.device)
    check(_lib.load().frl_mutual_knn(_p(features), n, d, _p(patch_id), _p(coords), float(pos_min_spatial), int(k), _p(knn), _p(mutual),
                                     _stream()), "frl_mutual_knn")
    return knn, mutual


@_timed("phase_pairs")
def phase_pairs(spec: torch.Tensor, ysfc: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor, k: int, min_overlap: int, min_pairs: int,
                sigma: float):
    """spec [N, D] float32, ysfc [N, T] float32, seg int32 [S + 1] row offsets on the device and seg_host the same on the host (validated
    there) -> dict of knn_idx / overlap int32 [N, k], keep / keep_overlap uint8 [N, k], weight / dist float32 [N, k], anchor_ok uint8 [N]
    and meta int32 [4 S + 1]: the [S, 4] counters (candidates, passing the overlap, cross pairs kept, anchors surviving) followed by the
    invalid-ysfc flag.  include/frl_hip.h (frl_phase_pairs) has the definitions.  No host read."""
    if spec.dim() != 2 or ysfc.dim() != 2 or ysfc.shape[0] != spec.shape[0] or spec.shape[0] == 0 or ysfc.shape[1] == 0:
        raise ValueError(f"phase_pairs: expected spec [N, D] and ysfc [N, T] with N, T > 0, got {tuple(spec.shape)} and {tuple(ysfc.shape)}")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"phase_pairs: k must be in 1..64 (one lane per neighbour), got {k}")
    if not float(sigma) > 0.0:
        raise ValueError(f"phase_pairs: sigma must be positive, got {sigma}")
    n, d = spec.shape
    if d > 256:
        raise ValueError("phase_pairs: at most 256 feature channels")
    if not spec.is_cuda or not ysfc.is_cuda:
        raise _lib.FrlHipError("phase_pairs: tensors must live on the GPU (no CPU fallback)")
    if spec.dtype != torch.float32 or ysfc.dtype != torch.float32 or not spec.is_contiguous() or not ysfc.is_contiguous() \
            or ysfc.device != spec.device:
        raise ValueError("phase_pairs: spec and ysfc must be contiguous float32 tensors on one device")
    if seg_host.is_cuda or seg_host.dtype != torch.int32 or seg_host.dim() != 1 or seg_host.numel() < 2 or not seg_host.is_contiguous():
        raise ValueError("phase_pairs: the host segment offsets must be a contiguous int32 [segments + 1] CPU tensor")
    if seg.dtype != torch.int32 or seg.shape != seg_host.shape or not seg.is_contiguous() or seg.device != spec.device:
        raise ValueError(f"phase_pairs: the device segment offsets must be a contiguous int32 [{seg_host.numel()}] tensor on the device of spec")
    width = min(w for w in (16, 32, 48, 64, 96, 128, 256) if w >= d)     # the widths the kernel is compiled for
    if width != d:
        # zero columns add exactly nothing to a squared distance (and leave the summation order of the real ones untouched)
        spec = torch.nn.functional.pad(spec, (0, width - d)).contiguous()
        d = width
    s, dev, k = seg_host.numel() - 1, spec.device, int(k)
    out = {"knn_idx": torch.empty((n, k), dtype=torch.int32, device=dev), "overlap": torch.empty((n, k), dtype=torch.int32, device=dev),
           "keep": torch.empty((n, k), dtype=torch.uint8, device=dev), "keep_overlap": torch.empty((n, k), dtype=torch.uint8, device=dev),
           "weight": torch.empty((n, k), dtype=torch.float32, device=dev), "dist": torch.empty((n, k), dtype=torch.float32, device=dev),
           "anchor_ok": torch.empty(n, dtype=torch.uint8, device=dev), "meta": torch.zeros(4 * s + 1, dtype=torch.int32, device=dev)}
    masks = torch.empty((n, 4), dtype=torch.int64, device=dev)
    meta = out["meta"]
    check(_lib.load().frl_phase_pairs(_p(spec), _p(ysfc), n, d, ysfc.shape[1], _p(seg_host), _p(seg), s, k, int(min_overlap), int(min_pairs),
                                      float(sigma), _p(masks), _p(out["knn_idx"]), _p(out["overlap"]), _p(out["keep"]),
                                      _p(out["keep_overlap"]), _p(out["weight"]), _p(out["dist"]), _p(out["anchor_ok"]), _p(meta),
                                      ctypes.c_void_p(meta.data_ptr() + 16 * s), _stream()), "frl_phase_pairs")
    return out


def _at(t: torch.Tensor, element: int):
    return ctypes.c_void_p(t.data_ptr() + element * t.element_size())


def _chk_spatial(bits, anchors, seg, seg_host, what):
    if not bits.is_cuda or not anchors.is_cuda:
        raise _lib.FrlHipError(f"{what}: tensors must live on the GPU (no CPU fallback)")
    if bits.dtype != torch.int32 or bits.dim() != 3 or not bits.is_contiguous():
        raise ValueError(f"{what}: the packed masks must be a contiguous int32 [S, H, ceil(W / 32)] tensor (spatial_pack_mask)")
    if anchors.dtype != torch.int32 or anchors.dim() != 2 or anchors.shape[1] != 2 or anchors.shape[0] == 0 or not anchors.is_contiguous():
        raise ValueError(f"{what}: anchors must be a contiguous int32 [N, 2] tensor with N > 0, got {tuple(anchors.shape)} {anchors.dtype}")
    if seg_host.is_cuda or seg_host.dtype != torch.int32 or seg_host.shape != (bits.shape[0] + 1,) or not seg_host.is_contiguous():
        raise ValueError(f"{what}: the host segment offsets must be a contiguous int32 [{bits.shape[0] + 1}] CPU tensor")
    if seg.dtype != torch.int32 or seg.shape != seg_host.shape or not seg.is_contiguous() or seg.device != anchors.device:
        raise ValueError(f"{what}: the device segment offsets must be a contiguous int32 [{seg_host.numel()}] tensor on the device of anchors")


@_timed("spatial_pack_mask")
def spatial_pack_mask(masks: torch.Tensor) -> torch.Tensor:
    """masks [S, H, W] bool -> int32 [S, H, ceil(W / 32)]: bit c % 32 of word c / 32 is pixel (r, c).  No host read."""
    if masks.dim() != 3 or masks.dtype != torch.bool or 0 in masks.shape:
        raise ValueError(f"spatial_pack_mask: expected a bool [S, H, W] tensor, got {tuple(masks.shape)} {masks.dtype}")
    if not masks.is_cuda:
        raise _lib.FrlHipError("spatial_pack_mask: tensors must live on the GPU (no CPU fallback)")
    masks = masks.contiguous()
    s, h, w = masks.shape
    bits = torch.empty((s, h, (w + 31) // 32), dtype=torch.int32, device=masks.device)
    check(_lib.load().frl_spatial_pack_mask(_p(masks), s, h, w, _p(bits), _stream()), "frl_spatial_pack_mask")
    return bits


@_timed("spatial_knn")
def spatial_knn(bits: torch.Tensor, w: int, anchors: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor, offsets: torch.Tensor,
                meta: torch.Tensor, counters_at: int, flag_at: int):
    """bits from spatial_pack_mask of masks [S, H, w], anchors int32 [N, 2], offsets int32 [k, 2] on the device -> (pos_rc int32 [N, k, 2],
    pos_valid uint8 [N, k]); meta[counters_at : counters_at + S] += valid slots per segment, meta[flag_at] |= 1 for an anchor outside the
    grid.  include/frl_hip.h (frl_spatial_knn) has the definitions.  No host read."""
    _chk_spatial(bits, anchors, seg, seg_host, "spatial_knn")
    k, n, dev = offsets.shape[0], anchors.shape[0], anchors.device
    if offsets.dtype != torch.int32 or offsets.dim() != 2 or offsets.shape[1] != 2 or not 1 <= k <= 64 or not offsets.is_contiguous() \
            or offsets.device != dev:
        raise ValueError("spatial_knn: offsets must be a contiguous int32 [k, 2] tensor on the device of anchors, 1 <= k <= 64")
    pos_rc = torch.empty((n, k, 2), dtype=torch.int32, device=dev)
    pos_valid = torch.empty((n, k), dtype=torch.uint8, device=dev)
    check(_lib.load().frl_spatial_knn(_p(bits), bits.shape[0], bits.shape[1], int(w), _p(anchors), n, _p(seg_host), _p(seg), _p(offsets), k,
                                      _p(pos_rc), _p(pos_valid), _at(meta, counters_at), _at(meta, flag_at), _stream()), "frl_spatial_knn")
    return pos_rc, pos_valid


@_timed("spatial_negatives")
def spatial_negatives(bits: torch.Tensor, w: int, anchors: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor, lo: int, hi: int,
                      draws: torch.Tensor, meta: torch.Tensor, counters_at: int, flag_at: int):
    """draws int32 [N, n_per_anchor] in [0, 2^31) -> (neg_rc int32 [N, n_per_anchor, 2], neg_count int32 [N]); lo / hi: the integer bounds on
    the squared distance.  meta[counters_at : counters_at + S] += negatives per segment, meta[flag_at] |= 1 for an anchor outside the grid,
    |= 2 for a negative draw.  include/frl_hip.h (frl_spatial_negatives) has the definitions.  No host read."""
    _chk_spatial(bits, anchors, seg, seg_host, "spatial_negatives")
    n, dev = anchors.shape[0], anchors.device
    if draws.dtype != torch.int32 or draws.dim() != 2 or draws.shape[0] != n or not 1 <= draws.shape[1] <= 64 or not draws.is_contiguous() \
            or draws.device != dev:
        raise ValueError(f"spatial_negatives: draws must be a contiguous int32 [{n}, n_per_anchor] tensor on the device of anchors, "
                         "1 <= n_per_anchor <= 64")
    n_per = draws.shape[1]
    neg_rc = torch.empty((n, n_per, 2), dtype=torch.int32, device=dev)
    neg_count = torch.empty(n, dtype=torch.int32, device=dev)
    check(_lib.load().frl_spatial_negatives(_p(bits), bits.shape[0], bits.shape[1], int(w), _p(anchors), n, _p(seg_host), _p(seg), int(lo),
                                            int(hi), n_per, _p(draws), _p(neg_rc), _p(neg_count), _at(meta, counters_at), _at(meta, flag_at),
                                            _stream()), "frl_spatial_negatives")
    return neg_rc, neg_count


@_timed("spatial_pair_index")
def spatial_pair_index(h: int, w: int, anchors: torch.Tensor, seg: torch.Tensor, seg_host: torch.Tensor, pos_rc: torch.Tensor,
                       pos_valid: torch.Tensor, neg_rc: torch.Tensor, neg_count: torch.Tensor, feat: torch.Tensor, tau: float, min_w: float,
                       meta: torch.Tensor, unique_seg_at: int):
    """The outputs of spatial_knn and spatial_negatives and feat float32 [S, C, H, W] -> dict of unique_rc int32 [N (1 + k + n), 2] (the
    first meta[unique_seg_at + S] rows are written), anchor_idx [N], pos_idx [N, k], neg_idx [N, n] int32 (-1: the slot holds nothing),
    pos_w / pos_d [N, k], neg_w / neg_d [N, n] float32; meta[unique_seg_at : unique_seg_at + S + 1] = the segments' offsets in unique_rc.
    include/frl_hip.h (frl_spatial_pair_index) has the definitions.  No host read."""
    n, dev, s = anchors.shape[0], anchors.device, seg_host.numel() - 1
    k, n_per = pos_valid.shape[1], neg_rc.shape[1]
    if feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[0] != s or tuple(feat.shape[2:]) != (h, w) or not feat.is_contiguous() \
            or not 1 <= feat.shape[1] <= 256 or feat.device != dev:
        raise ValueError(f"spatial_pair_index: feat must be a contiguous float32 [{s}, C <= 256, {h}, {w}] tensor on the device of anchors")
    if not float(tau) > 0.0:
        raise ValueError(f"spatial_pair_index: tau must be positive, got {tau}")
    nwb = (h * w + 31) // 32
    bitmap = torch.empty(s * nwb, dtype=torch.int32, device=dev)
    wordpre = torch.empty(s * (nwb + 1), dtype=torch.int32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    out = {"unique_rc": torch.empty((n * (1 + k + n_per), 2), **i32), "anchor_idx": torch.empty(n, **i32), "pos_idx": torch.empty((n, k), **i32),
           "neg_idx": torch.empty((n, n_per), **i32), "pos_w": torch.empty((n, k), **f32), "pos_d": torch.empty((n, k), **f32),
           "neg_w": torch.empty((n, n_per), **f32), "neg_d": torch.empty((n, n_per), **f32)}
    check(_lib.load().frl_spatial_pair_index(s, int(h), int(w), _p(anchors), n, _p(seg_host), _p(seg), _p(pos_rc), _p(pos_valid), k, _p(neg_rc),
                                             _p(neg_count), n_per, _p(feat), feat.shape[1], float(tau), float(min_w), _p(bitmap), _p(wordpre),
                                             _at(meta, unique_seg_at), _p(out["unique_rc"]), _p(out["anchor_idx"]), _p(out["pos_idx"]),
                                             _p(out["neg_idx"]), _p(out["pos_w"]), _p(out["pos_d"]), _p(out["neg_w"]), _p(out["neg_d"]),
                                             _stream()), "frl_spatial_pair_index")
    return out


def _chk_anchor_bits(bits: torch.Tensor, w: int, what: str):
    if not bits.is_cuda:
        raise _lib.FrlHipError(f"{what}: tensors must live on the GPU (no CPU fallback)")
    if bits.dtype != torch.int32 or bits.dim() != 3 or not bits.is_contiguous() or bits.shape[2] != (int(w) + 31) // 32:
        raise ValueError(f"{what}: the packed masks must be a contiguous int32 [S, H, ceil(W / 32)] tensor (spatial_pack_mask)")


def _chk_anchor_map(t: torch.Tensor, bits: torch.Tensor, w: int, name: str, what: str):
    shape = (bits.shape[0], bits.shape[1], int(w))
    if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != bits.device:
        raise ValueError(f"{what}: {name} must be a contiguous float32 {list(shape)} tensor on the device of the masks, got "
                         f"{tuple(t.shape)} {t.dtype}")


@_timed("anchor_grid")
def anchor_grid(bits: torch.Tensor, w: int, stride: int, border: int, jitter_radius: int, jitter: torch.Tensor, gmax: int,
                meta: torch.Tensor, counts_at: int, flag_at: int) -> torch.Tensor:
    """bits from spatial_pack_mask of masks [S, H, w], jitter int32 [S, 2] on the device -> grid_rc int32 [S, gmax, 2] (-1 beyond the
    count); meta[counts_at : counts_at + S] = grid points per sample, meta[flag_at] |= 1 for a jitter out of range.  gmax is at least
    frl_anchor_grid_max.  include/frl_hip.h (frl_anchor_grid) has the definitions.  No host read."""
    _chk_anchor_bits(bits, w, "anchor_grid")
    s, dev = bits.shape[0], bits.device
    if jitter.dtype != torch.int32 or tuple(jitter.shape) != (s, 2) or not jitter.is_contiguous() or jitter.device != dev:
        raise ValueError(f"anchor_grid: jitter must be a contiguous int32 [{s}, 2] tensor on the device of the masks")
    grid_rc = torch.empty((s, int(gmax), 2), dtype=torch.int32, device=dev)
    check(_lib.load().frl_anchor_grid(_p(bits), s, bits.shape[1], int(w), int(stride), int(border), int(jitter_radius), _p(jitter), int(gmax),
                                      _p(grid_rc), _at(meta, counts_at), _at(meta, flag_at), _stream()), "frl_anchor_grid")
    return grid_rc


@_timed("anchor_supplement")
def anchor_supplement(bits: torch.Tensor, w: int, weights: Optional[torch.Tensor], noise: Optional[torch.Tensor], supplement_n: int,
                      meta: torch.Tensor, counts_at: int, valid_at: int, flag_at: int) -> torch.Tensor:
    """weights float32 [S, H, w] or None, noise float32 [S, H, w] >= 0 (None only with supplement_n = 0) -> sup_rc int32
    [S, supplement_n, 2]: the min(supplement_n, eligible) eligible pixels of smallest (noise / weight, pixel index), ascending, -1 beyond;
    meta[counts_at : + S] = picks per sample, meta[valid_at : + S] = valid pixels per sample, meta[flag_at] |= 2 for a non-finite weight,
    |= 4 for a negative or NaN noise at a valid pixel.  include/frl_hip.h (frl_anchor_supplement) has the definitions.  No host read."""
    _chk_anchor_bits(bits, w, "anchor_supplement")
    n = int(supplement_n)
    if not 0 <= n <= 1024:
        raise ValueError(f"anchor_supplement: supplement_n must be in 0..1024, got {supplement_n}")
    if weights is not None:
        _chk_anchor_map(weights, bits, w, "weights", "anchor_supplement")
    if noise is not None:
        _chk_anchor_map(noise, bits, w, "noise", "anchor_supplement")
    elif n > 0:
        raise ValueError("anchor_supplement: noise is required when supplement_n > 0")
    s = bits.shape[0]
    sup_rc = torch.empty((s, n, 2), dtype=torch.int32, device=bits.device)
    keys = torch.empty((s, bits.shape[1], int(w)), dtype=torch.int32, device=bits.device) if n else None     # workspace: the key patterns
    check(_lib.load().frl_anchor_supplement(_p(bits), s, bits.shape[1], int(w), _p(weights), _p(noise), n, _p(keys), _p(sup_rc) if n else _p(None),
                                            _at(meta, counts_at), _at(meta, valid_at), _at(meta, flag_at), _stream()), "frl_anchor_supplement")
    return sup_rc


@_timed("anchor_inverse_frequency")
def anchor_inverse_frequency(data: torch.Tensor, bits: torch.Tensor, valid_values: Optional[torch.Tensor], flag: torch.Tensor) -> torch.Tensor:
    """data float32 [S, H, W], bits the packed valid masks, valid_values a sorted int32 list on the device (possibly empty) or None ->
    float32 [S, H, W]: 1 / (eligible pixels of the sample with the same value), 0 at ineligible pixels, 1 at the valid pixels of a sample
    without an eligible one; flag[0] |= 8 for more than 4096 distinct values.  include/frl_hip.h (frl_anchor_inverse_frequency).  No host read."""
    if data.dim() != 3:
        raise ValueError(f"anchor_inverse_frequency: data must be [S, H, W], got {tuple(data.shape)}")
    _chk_anchor_bits(bits, data.shape[2], "anchor_inverse_frequency")
    _chk_anchor_map(data, bits, data.shape[2], "data", "anchor_inverse_frequency")
    n_values = 0
    if valid_values is not None:
        if valid_values.dtype != torch.int32 or valid_values.dim() != 1 or valid_values.numel() > 4096 or not valid_values.is_contiguous() \
                or valid_values.device != data.device:
            raise ValueError("anchor_inverse_frequency: valid_values must be a contiguous int32 list of at most 4096 entries on the device")
        n_values = valid_values.numel()
        if n_values == 0:
            valid_values = torch.zeros(1, dtype=torch.int32, device=data.device)          # a list that holds nothing is still a list
    out = torch.empty_like(data)
    s, h, w = data.shape
    check(_lib.load().frl_anchor_inverse_frequency(_p(data), _p(bits), s, h, w, _p(valid_values), n_values, _p(out), _p(flag), _stream()),
          "frl_anchor_inverse_frequency")
    return out


@_timed("normalize_tiles")
def normalize_tiles(raw: torch.Tensor, table: torch.Tensor, valid: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.bfloat16,
                    out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Chunk-store rows [..., F] (float16 | float32, NaN = no data) -> normalised rows (bf16 | f32) + validity bytes [...].

    `table` is the device image of the per-feature records (`data.normalization.norm_table`, 8 x 4 bytes per feature);
    `valid` an optional uint8/bool tensor over the leading dims.  See include/frl_hip.h (frl_normalize_tiles)."""
    if raw.dtype not in (torch.float16, torch.float32) or not raw.is_contiguous():
        raise ValueError("normalize_tiles: raw rows must be contiguous float16 or float32")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("normalize_tiles: output must be bfloat16 or float32")
    f = raw.shape[-1]
    rows = raw.numel() // f if f else 0
    if table.dtype != torch.uint8 or table.numel() != 32 * f or table.device != raw.device:
        raise ValueError("normalize_tiles: table must be the 32-byte-per-feature record image on the device of the rows")
    if valid is not None:
        if valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        if valid.dtype != torch.uint8 or valid.numel() != rows or not valid.is_contiguous() or valid.device != raw.device:
            raise ValueError("normalize_tiles: valid must be one contiguous byte per row")
    if out is None:
        out = torch.empty(raw.shape, dtype=out_dtype, device=raw.device)
    if mask_out is None:
        mask_out = torch.empty(raw.shape[:-1], dtype=torch.uint8, device=raw.device)
    if out.shape != raw.shape or out.dtype != out_dtype or not out.is_contiguous() or mask_out.numel() != rows:
        raise ValueError("normalize_tiles: output buffers do not match the rows")
    check(_lib.load().frl_normalize_tiles(_p(raw), _lib.F16 if raw.dtype == torch.float16 else F32, _p(valid) if valid is not None else None,
                                          _p(table), _p(out), _dt(out), _p(mask_out), rows, f, _stream()), "frl_normalize_tiles")
    return out, mask_out


@_timed("normalize_chunk_tiles")
def normalize_chunk_tiles(chunk: torch.Tensor, desc: torch.Tensor, tile: int, table: torch.Tensor, out_dtype: torch.dtype = torch.bfloat16,
                          out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One stored chunk [T, CY, CX, F] (float16 | float32) + tile descriptors [B, 4] int32 {y0, x0, h, w} ->
    normalised tiles [B, T, tile, tile, F] + validity bytes [B, T, tile, tile]; the tile cut and the zero padding of partial
    patches happen on the device (frl_normalize_chunk_tiles)."""
    if chunk.dim() != 4 or chunk.dtype not in (torch.float16, torch.float32) or not chunk.is_contiguous():
        raise ValueError("normalize_chunk_tiles: chunk must be a contiguous float16/float32 [T, CY, CX, F] tensor")
    t_, cy, cx, f = chunk.shape
    if desc.dtype != torch.int32 or desc.dim() != 2 or desc.shape[1] != 4 or not desc.is_contiguous() or desc.device != chunk.device:
        raise ValueError("normalize_chunk_tiles: desc must be a contiguous int32 [B, 4] tensor on the chunk's device")
    if table.dtype != torch.uint8 or table.numel() != 32 * f or table.device != chunk.device:
        raise ValueError("normalize_chunk_tiles: table must be the 32-byte-per-feature record image on the chunk's device")
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError("normalize_chunk_tiles: output must be bfloat16 or float32")
    b = desc.shape[0]
    shape = (b, t_, tile, tile, f)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=chunk.device)
    if mask_out is None:
        mask_out = torch.empty(shape[:-1], dtype=torch.uint8, device=chunk.device)
    if tuple(out.shape) != shape or out.dtype != out_dtype or not out.is_contiguous() or mask_out.numel() != b * t_ * tile * tile \
            or not mask_out.is_contiguous():
        raise ValueError("normalize_chunk_tiles: output buffers do not match the tiles")
    check(_lib.load().frl_normalize_chunk_tiles(_p(chunk), _lib.F16 if chunk.dtype == torch.float16 else F32, t_, cy, cx, f, _p(desc), b, int(tile),
                                                _p(table), _p(out), _dt(out), _p(mask_out), _stream()), "frl_normalize_chunk_tiles")
    return out, mask_out


@_timed("add")
def add(a: torch.Tensor, b: torch.Tensor, scale_b: float = 1.0) -> torch.Tensor:
    """out = a + scale_b * b"""
    out = torch.empty_like(a)
    check(_lib.load().frl_add(_p(a), _p(b), float(scale_b), _p(out), a.numel(), _dt(a), _stream()), "frl_add")
    return out


# ----------------------------------------------------------------------------------------------
# 3x3 convolution (csrc/conv3x3.hip); x [B,H,W,Cin], w [Cout,Cin,3,3]
# ----------------------------------------------------------------------------------------------
@_timed("conv3x3_fwd")
def conv3x3_fwd(x, w, bias, act: int = ACT_NONE):
    b, h, wd, cin = x.shape
    cout = w.shape[0]
    _chk_rows(x, cin, "conv3x3.x")
    y = torch.empty(b, h, wd, cout, dtype=x.dtype, device=x.device)
    lib = _lib.load()
    ws = workspace(lib.frl_conv_workspace_bytes(cin, cout, 9), x.device)
    check(lib.frl_conv3x3_fwd(_p(x), _p(_f32(w, "w")), _p(_f32(bias, "bias")), _p(y), b, h, wd, cin, cout, act, _dt(x), _p(ws),
                              ws.numel(), _stream()), "frl_conv3x3_fwd")
    return y


@_timed("conv3x3_fwd_gate_blend")
def conv3x3_fwd_gate_blend(x, w, bias, smoothed, residual):
    """-> (out = smoothed + gate * residual, gate = sigmoid(conv3x3(x, w) + bias)): the blend of spatial.py:332-335 (min_gate = 0) in the
    convolution's epilogue."""
    b, h, wd, cin = x.shape
    cout = w.shape[0]
    _chk_rows(x, cin, "conv3x3.x")
    gate = torch.empty(b, h, wd, cout, dtype=x.dtype, device=x.device)
    _chk_like(smoothed, gate, "conv3x3_fwd_gate_blend.smoothed")
    _chk_like(residual, gate, "conv3x3_fwd_gate_blend.residual")
    out = torch.empty_like(gate)
    lib = _lib.load()
    ws = workspace(lib.frl_conv_workspace_bytes(cin, cout, 9), x.device)
    check(lib.frl_conv3x3_fwd_gate_blend(_p(x), _p(_f32(w, "w")), _p(_f32(bias, "bias")), _p(smoothed), _p(residual), _p(gate), _p(out), b, h, wd,
                                         cin, cout, _dt(x), _p(ws), ws.numel(), _stream()), "frl_conv3x3_fwd_gate_blend")
    return out, gate


@_timed("conv3x3_bwd_data")
def conv3x3_bwd_data(dy, w, y=None, act: int = ACT_NONE, add=None, sub_from=None, out_y=None, out_act: int = ACT_NONE, gate=None):
    """dx = conv3x3^T(dy .* act'(y)) (+ add).  With sub_from the call returns (dx, sub_from - dx): both extras ride in the epilogue.
    out_y / out_act (instead of add / sub_from): dx .* out_act'(out_y) -- the gradient arrives at the next backward step already masked.
    gate (with sub_from, instead of add): add = sub_from * gate rounded to the tensor dtype, formed in the epilogue (the gate blend's d residual)."""
    b, h, wd, cout = dy.shape
    cin = w.shape[1]
    dx = torch.empty(b, h, wd, cin, dtype=dy.dtype, device=dy.device)
    lib = _lib.load()
    ws = workspace(lib.frl_conv_workspace_bytes(cin, cout, 9), dy.device)
    if gate is not None:
        if add is not None or out_y is not None or sub_from is None:
            raise ValueError("conv3x3_bwd_data: gate needs sub_from and combines with neither add nor out_y")
        _chk_like(gate, dx, "conv3x3_bwd_data.gate")
        _chk_like(sub_from, dx, "conv3x3_bwd_data.sub_from")
        out2 = torch.empty_like(dx)
        check(lib.frl_conv3x3_bwd_data_blend(_p(dy), _p(y), act, _p(_f32(w, "w")), _p(dx), _p(gate), _p(sub_from), _p(out2), b, h, wd,
                                             cin, cout, _dt(dy), _p(ws), ws.numel(), _stream()), "frl_conv3x3_bwd_data_blend")
        return dx, out2
    if out_y is not None:
        if add is not None or sub_from is not None:
            raise ValueError("conv3x3_bwd_data: out_y does not combine with add / sub_from")
        _chk_like(out_y, dx, "conv3x3_bwd_data.out_y")
        check(lib.frl_conv3x3_bwd_data_outmask(_p(dy), _p(y), act, _p(_f32(w, "w")), _p(dx), _p(out_y), out_act, b, h, wd, cin, cout, _dt(dy),
                                               _p(ws), ws.numel(), _stream()), "frl_conv3x3_bwd_data_outmask")
        return dx
    if add is not None or sub_from is not None:
        out2 = None
        if add is not None:
            _chk_like(add, dx, "conv3x3_bwd_data.add")
        if sub_from is not None:
            _chk_like(sub_from, dx, "conv3x3_bwd_data.sub_from")
            out2 = torch.empty_like(dx)
        check(lib.frl_conv3x3_bwd_data_fused(_p(dy), _p(y), act, _p(_f32(w, "w")), _p(dx), _p(add), _p(sub_from), _p(out2), b, h, wd,
                                             cin, cout, _dt(dy), _p(ws), ws.numel(), _stream()), "frl_conv3x3_bwd_data_fused")
        return dx if sub_from is None else (dx, out2)
    check(lib.frl_conv3x3_bwd_data(_p(dy), _p(y), act, _p(_f32(w, "w")), _p(dx), b, h, wd, cin, cout, _dt(dy), _p(ws),
                                   ws.numel(), _stream()), "frl_conv3x3_bwd_data")
    return dx


@_timed("conv3x3_bwd_weight")
def conv3x3_bwd_weight(dy, x, y=None, act: int = ACT_NONE, scalar_frags: bool = False, want_bias: bool = True):
    b, h, wd, cout = dy.shape
    cin = x.shape[-1]
    lib = _lib.load()
    ws = workspace(lib.frl_conv3x3_bwd_weight_workspace_bytes(b, h, wd, cin, cout), dy.device)
    dw = grad_empty((cout, cin, 3, 3), dy.device)
    db = grad_empty((cout,), dy.device) if want_bias else None
    check(lib.frl_conv3x3_bwd_weight(_p(dy), _p(y), act, _p(x), _p(dw), _p(db), b, h, wd, cin, cout, _dt(dy), _p(ws),
                                     ws.numel(), 1 if scalar_frags else 0, _stream()), "frl_conv3x3_bwd_weight")
    return dw, db


def conv3x3_wgrad_multi(on: bool) -> bool:
    """A/B hook (include/frl_hip.h: frl_conv3x3_wgrad_multi): False makes conv3x3_bwd_weight_multi run job by job.  Returns the previous setting."""
    return bool(_lib.load().frl_conv3x3_wgrad_multi(1 if on else 0))


def conv3x3_wgrad_multi_supported(jobs) -> bool:
    """True when the jobs [(dy, x, y, act, want_weight, want_bias), ...] can share ONE launch of the band kernel (csrc/conv3x3_wgrad.hip):
    at most 4 contiguous bf16 jobs on one device over images of one shape, H % 8 == 0, W % 32 == 0, Cin % 64 == 0, Cout == 64, and a
    tile count for which the merged launch keeps the single calls' bits (wgrad_split.eligible)."""
    from . import wgrad_split
    if not 1 <= len(jobs) <= wgrad_split.MAX_JOBS:
        return False
    dy0 = jobs[0][0]
    for dy, x, y, act, _, _ in jobs:
        ts = [t for t in (dy, x, y) if t is not None]
        if any(t.dim() != 4 or not t.is_cuda or t.dtype != torch.bfloat16 or not t.is_contiguous() or t.device != dy0.device for t in ts):
            return False
        if dy.shape[:3] != dy0.shape[:3] or x.shape[:3] != dy0.shape[:3] or (y is not None and y.shape != dy.shape):
            return False
        if act != ACT_NONE and y is None:
            return False
    b, h, w = dy0.shape[:3]
    return wgrad_split.eligible(b, h, w, [j[1].shape[-1] for j in jobs], [j[0].shape[-1] for j in jobs])


@_timed("conv3x3_bwd_weight_multi")
def conv3x3_bwd_weight_multi(jobs):
    """jobs: [(dy, x, y, act, want_weight, want_bias), ...] over images of one shape -> [(dw | None, db | None), ...] from one call
    (frl_conv3x3_bwd_weight_multi): one launch of the band kernel where conv3x3_wgrad_multi_supported holds, else job by job."""
    n = len(jobs)
    dy0 = jobs[0][0]
    b, h, wd = dy0.shape[:3]
    for dy, x, y, act, ww, wb in jobs:
        if dy.shape[:3] != dy0.shape[:3] or x.shape[:3] != dy0.shape[:3] or dy.dtype != dy0.dtype or x.dtype != dy0.dtype:
            raise ValueError("conv3x3_bwd_weight_multi: the jobs share B, H, W and the dtype")
        _chk_rows(dy, dy.shape[-1], "conv3x3_bwd_weight_multi.dy")
        _chk_rows(x, x.shape[-1], "conv3x3_bwd_weight_multi.x")
        if act != ACT_NONE:
            if y is None:
                raise ValueError("conv3x3_bwd_weight_multi: an activation mask needs y")
            _chk_like(y, dy, "conv3x3_bwd_weight_multi.y")
        if not (ww or wb):
            raise ValueError("conv3x3_bwd_weight_multi: a job wants its weight gradient, its bias gradient or both")
    lib = _lib.load()
    cin = (ctypes.c_int * n)(*[j[1].shape[-1] for j in jobs])
    cout = (ctypes.c_int * n)(*[j[0].shape[-1] for j in jobs])
    acts = (ctypes.c_int * n)(*[int(j[3]) for j in jobs])
    ws = workspace(lib.frl_conv3x3_bwd_weight_multi_workspace_bytes(n, b, h, wd, cin, cout, _dt(dy0)), dy0.device)
    out = [(grad_empty((j[0].shape[-1], j[1].shape[-1], 3, 3), dy0.device) if j[4] else None,
            grad_empty((j[0].shape[-1],), dy0.device) if j[5] else None) for j in jobs]

    def ptrs(ts):
        return (ctypes.c_void_p * n)(*[0 if t is None else t.data_ptr() for t in ts])

    check(lib.frl_conv3x3_bwd_weight_multi(n, ptrs([j[0] for j in jobs]), ptrs([j[2] if j[3] != ACT_NONE else None for j in jobs]), acts,
                                           ptrs([j[1] for j in jobs]), ptrs([o[0] for o in out]), ptrs([o[1] for o in out]), b, h, wd, cin, cout,
                                           _dt(dy0), _p(ws), ws.numel(), _stream()), "frl_conv3x3_bwd_weight_multi")
    return out


# ----------------------------------------------------------------------------------------------
# fixed stencils of EdgeAwareSmoothingConv2D (csrc/stencil.hip)
# ----------------------------------------------------------------------------------------------
def sobel_stream(on: bool) -> bool:
    """A/B hook (include/frl_hip.h: frl_sobel_stream): True (default) = bf16 Sobel calls with W * C / 8 == 256 take the row-band streaming
    kernels, False = every call takes the gather kernels; same bits.  Returns the previous setting."""
    return bool(_lib.load().frl_sobel_stream(1 if on else 0))


def sobel_stream_band(rows: int = 0) -> int:
    """Rows per workgroup of the streaming Sobel route (1..64); returns the previous height, rows=0 only reads it."""
    return int(_lib.load().frl_sobel_stream_band(int(rows)))


@_timed("sobel_fwd")
def sobel_fwd(x):
    b, h, w, c = x.shape
    g = torch.empty(b, h, w, 2 * c, dtype=x.dtype, device=x.device)
    check(_lib.load().frl_sobel_fwd(_p(x), _p(g), b, h, w, c, _dt(x), _stream()), "frl_sobel_fwd")
    return g


@_timed("sobel_bwd")
def sobel_bwd(dg, add=None):
    b, h, w, c2 = dg.shape
    dx = torch.empty(b, h, w, c2 // 2, dtype=dg.dtype, device=dg.device)
    if add is not None:
        _chk_like(add, dx, "sobel_bwd.add")
        check(_lib.load().frl_sobel_bwd_add(_p(dg), _p(dx), _p(add), b, h, w, c2 // 2, _dt(dg), _stream()), "frl_sobel_bwd_add")
        return dx
    check(_lib.load().frl_sobel_bwd(_p(dg), _p(dx), b, h, w, c2 // 2, _dt(dg), _stream()), "frl_sobel_bwd")
    return dx


@_timed("edge_smooth_fwd")
def edge_smooth_fwd(x, a_logit, b_logit, rank: int, coarse_dilation: int):
    b, h, w, c = x.shape
    sm, res = torch.empty_like(x), torch.empty_like(x)
    a_soft, b_soft = torch.empty_like(a_logit), torch.empty_like(b_logit)
    check(_lib.load().frl_edge_smooth_stencil_fwd(_p(x), _p(a_logit), _p(b_logit), _p(sm), _p(res), _p(a_soft), _p(b_soft),
                                                  b, h, w, c, rank, coarse_dilation, _dt(x), _stream()),
          "frl_edge_smooth_stencil_fwd")
    return sm, res, a_soft, b_soft


@_timed("edge_smooth_bwd")
def edge_smooth_bwd(d_smoothed, x, a_soft, b_soft, rank: int, coarse_dilation: int, dx_add: Optional[torch.Tensor] = None):
    """dx_add (optional, same shape and dtype as x): added to dx inside the kernel's store (the residual branch's gradient)."""
    b, h, w, c = x.shape
    dx = torch.empty_like(x)
    da, db = torch.empty_like(a_soft), torch.empty_like(b_soft)
    if dx_add is not None and (dx_add.shape != x.shape or dx_add.dtype != x.dtype or not dx_add.is_contiguous()):
        raise ValueError("edge_smooth_bwd: dx_add must match x")
    check(_lib.load().frl_edge_smooth_stencil_bwd(_p(d_smoothed), _p(x), _p(a_soft), _p(b_soft), _p(dx), _p(da), _p(db), _p(dx_add),
                                                  b, h, w, c, rank, coarse_dilation, _dt(x), _stream()),
          "frl_edge_smooth_stencil_bwd")
    return dx, da, db


_LEAN = {"on": True}


def set_lean(on: bool) -> bool:
    """Process-wide (the backward runs on autograd's worker threads): False makes the autograd nodes issue the framework launches they
    issued before `functional._lean` existed (zero-filled gradients, the statistics clone, the stacked scalars).  A trainer with an active
    data-parallel reducer switches it off for its steps: that step is left exactly as it was.  Returns the previous setting."""
    was, _LEAN["on"] = _LEAN["on"], bool(on)
    return was


def lean_enabled() -> bool:
    return _LEAN["on"] and fusion_enabled("launches")


def fusion_enabled(name: str) -> bool:
    """A/B switch for measurements: FRL_HIP_DISABLE=chain,film,heads routes the named fusions through their modular kernels."""
    import os
    return name not in os.environ.get("FRL_HIP_DISABLE", "").split(",")


def smooth_heads_supported(x: torch.Tensor, hidden: int, rank: int, wa, ba, wb, bb) -> bool:
    """True when the two mixing heads, their softmaxes and the directional bank run as ONE kernel per direction (csrc/smooth_fused.hip):
    bf16 rows of 64 channels, 64 hidden features, rank 4, both heads with a bias."""
    if ba is None or bb is None or x.dim() != 4 or not x.is_cuda or not fusion_enabled("heads"):
        return False
    if tuple(wa.shape[:2]) != (8 * rank, hidden) or tuple(wb.shape[:2]) != (x.shape[-1] * rank, hidden):
        return False
    return bool(_lib.load().frl_smooth_heads_supported(x.shape[-1], hidden, rank, _dt(x)))


@_timed("smooth_heads_fwd")
def smooth_heads_fwd(x, feat, wa, ba, wb, bb, coarse_dilation: int):
    """x, feat [B,H,W,64] bf16; wa [32,64(,1,1)], wb [256,64(,1,1)] f32 -> (smoothed, residual)."""
    b, h, w, c = x.shape
    _chk_rows(x, c, "smooth_heads_fwd.x")
    _chk_like(feat, x, "smooth_heads_fwd.feat")
    lib = _lib.load()
    ws = workspace(lib.frl_smooth_heads_workspace_bytes(b * h * w), x.device)
    sm, res = torch.empty_like(x), torch.empty_like(x)
    check(lib.frl_smooth_heads_fwd(_p(x), _p(feat), _p(_f32(wa, "wa")), _p(_f32(ba, "ba")), _p(_f32(wb, "wb")), _p(_f32(bb, "bb")), _p(sm), _p(res),
                                   b, h, w, coarse_dilation, _p(ws), ws.numel(), _stream()), "frl_smooth_heads_fwd")
    return sm, res


@_timed("smooth_heads_bwd")
def smooth_heads_bwd(d_smoothed, x, feat, wa, ba, wb, bb, coarse_dilation: int, dx_add: Optional[torch.Tensor] = None, dfeat_relu: bool = False):
    """-> (dx, dfeat [B,H,W,64] bf16, dwa, dba, dwb, dbb f32).  d_smoothed: gradient w.r.t. `smoothed` with the residual path folded in
    (d smoothed - d residual); dx_add: added to dx inside the kernel's store; dfeat_relu: dfeat comes back multiplied by [feat > 0]."""
    b, h, w, c = x.shape
    for t, n in ((d_smoothed, "d_smoothed"), (feat, "feat")):
        _chk_like(t, x, f"smooth_heads_bwd.{n}")
    if dx_add is not None:
        _chk_like(dx_add, x, "smooth_heads_bwd.dx_add")
    lib = _lib.load()
    npix = b * h * w
    ws = workspace(lib.frl_smooth_heads_workspace_bytes(npix), x.device)
    scratch = torch.empty(lib.frl_smooth_heads_bwd_scratch_bytes(npix), dtype=torch.uint8, device=x.device)
    dx, dfeat = torch.empty_like(x), torch.empty_like(feat)
    dwa, dba, dwb, dbb = (grad_empty(t.shape, x.device) for t in (wa, ba, wb, bb))
    check(lib.frl_smooth_heads_bwd_masked(_p(d_smoothed), _p(x), _p(feat), _p(_f32(wa, "wa")), _p(_f32(ba, "ba")), _p(_f32(wb, "wb")),
                                          _p(_f32(bb, "bb")), _p(dx_add), _p(dx), _p(dfeat), _p(dwa), _p(dba), _p(dwb), _p(dbb), _p(scratch),
                                          scratch.numel(), b, h, w, coarse_dilation, int(dfeat_relu), _p(ws), ws.numel(), _stream()),
          "frl_smooth_heads_bwd_masked")
    return dx, dfeat, dwa, dba, dwb, dbb


# ----------------------------------------------------------------------------------------------
# fused TCN block (csrc/tcn_fwd.hip, tcn_bwd.hip; hot configuration: tcn_hot.hip, tcn_hot_bwd4.hip); x [B,T,HW..,Cin]
# ----------------------------------------------------------------------------------------------
def tcn_hot_supported(x: torch.Tensor, cin: int, cout: int, groups: int, dilation: int, has_projection: bool) -> bool:
    """True when the block on x [B,T,..,Cin] runs on the specialised `tcn_hot_*` kernels (the only ones that take a Dropout1d mask)."""
    return bool(_lib.load().frl_tcn_hot_supported(x.shape[1], cin, cout, groups, dilation, int(has_projection), _dt(x)))


def _check_drop_mask(drop_mask, x, hot: bool):
    if drop_mask is None:
        return
    if not hot:
        raise NotImplementedError("the generic TCN kernels take no Dropout1d mask (only the hot configuration: bf16, 64 channels, T = 5, "
                                  "8 groups, dilation 1/2/4); GatedResidualBlock routes other shapes through its two-input formulation")
    b, t, c = x.shape[0], x.shape[1], x.shape[-1]
    if drop_mask.dtype != x.dtype or not drop_mask.is_contiguous() or drop_mask.numel() != x.numel() // t:
        raise ValueError("drop_mask must be a contiguous [B, HW.., C] tensor of x's dtype")


@_timed("tcn_block_fwd")
def tcn_block_fwd(x, conv_w, conv_b, gn_w, gn_b, gate_w, gate_b, proj_w, proj_b, dilation: int, groups: int,
                  eps: float = 1e-5, allow_hot: bool = True, drop_mask=None):
    b, t, cin = x.shape[0], x.shape[1], x.shape[-1]
    cout = conv_w.shape[0]
    hw = x.numel() // (b * t * cin)
    y = torch.empty(x.shape[:-1] + (cout,), dtype=x.dtype, device=x.device)
    lib = _lib.load()
    hot = bool(allow_hot and lib.frl_tcn_hot_supported(t, cin, cout, groups, dilation, int(proj_w is not None), _dt(x)))
    _check_drop_mask(drop_mask, x, hot)
    if hot:
        ws = workspace(lib.frl_tcn_hot_fwd_workspace_bytes(), x.device)
        check(lib.frl_tcn_hot_fwd(_p(x), _p(drop_mask), _p(_f32(conv_w, "conv_w")), _p(conv_b), _p(gn_w), _p(gn_b),
                                  _p(_f32(gate_w.reshape(cout, cout), "gate_w")), _p(gate_b), _p(y), b * hw, hw, dilation, float(eps),
                                  _p(ws), ws.numel(), _stream()), "frl_tcn_hot_fwd")
        return y
    ws = workspace(lib.frl_conv_workspace_bytes(max(cin, cout), cout, 6), x.device)
    check(lib.frl_tcn_block_fwd(_p(x), _p(_f32(conv_w, "conv_w")), _p(conv_b), _p(gn_w), _p(gn_b),
                                _p(_f32(gate_w.reshape(cout, cout), "gate_w")), _p(gate_b), _p(proj_w), _p(proj_b),
                                _p(y), b * hw, hw, t, cin, cout, dilation, groups, float(eps), _dt(x), _p(ws), ws.numel(),
                                _stream()), "frl_tcn_block_fwd")
    return y


def tcn_chain_supported(x: torch.Tensor, blocks, head_w: torch.Tensor) -> bool:
    """True when three blocks (dilation 1, 2, 4; hot configuration each) and the 1x1 head run as ONE forward launch (tcn_chain_fwd_kernel).
    blocks: three tuples (conv_w, conv_b, gn_w, gn_b, gate_w, gate_b, dilation, groups, has_projection)."""
    if len(blocks) != 3 or x.dim() < 3 or not x.is_cuda or not fusion_enabled("chain"):
        return False
    lib = _lib.load()
    t, c = x.shape[1], x.shape[-1]
    for blk, dil in zip(blocks, (1, 2, 4)):
        if blk[6] != dil or not lib.frl_tcn_hot_supported(t, c, blk[0].shape[0], blk[7], dil, int(blk[8]), _dt(x)):
            return False
    ch = head_w.shape[0]
    return head_w.shape[1] == 64 and ch in (4, 8, 12, 16)


@_timed("tcn_chain_fwd")
def tcn_chain_fwd(x, blocks, head_w, head_b, eps: float = 1e-5, keep_intermediates: bool = True, want_xtype: bool = False):
    """x [B,5,HW..,64] -> (y1, y2, y3 [same shape], h [B,5,HW..,Ch]).  keep_intermediates=False runs the inference variant of the
    launch: y1, y2, y3 (kept for the backward only) are neither allocated nor written and come back as None; h is the same, bit for bit.
    want_xtype=True: the launch also writes the time mean of x ([B,HW..,64], bit for bit mean_time(x): the rows are in its registers
    anyway) and the result is (y1, y2, y3, h, x_type); a tensor instead of True is the buffer to write x_type into (>= B*HW*64 elements)."""
    b, t, c = x.shape[0], x.shape[1], x.shape[-1]
    hw = x.numel() // (b * t * c)
    _chk_rows(x, c, "tcn_chain_fwd.x")
    ch = head_w.shape[0]
    lib = _lib.load()
    ws = workspace(lib.frl_tcn_chain_fwd_workspace_bytes(), x.device)
    ys = [torch.empty_like(x) for _ in range(3)] if keep_intermediates else [None] * 3
    h = torch.empty(x.shape[:-1] + (ch,), dtype=x.dtype, device=x.device)
    if torch.is_tensor(want_xtype):
        xt, want_xtype = want_xtype, True
        if xt.dtype != x.dtype or xt.device != x.device or not xt.is_contiguous() or xt.numel() < b * hw * c:
            raise ValueError("tcn_chain_fwd: the x_type buffer must be contiguous, of x's dtype and device, with >= B*HW*C elements")
    else:
        xt = torch.empty((b,) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device) if want_xtype else None
    arr = ctypes.c_void_p * 3
    cols = [arr(*[_f32(blk[i] if i != 4 else blk[i].reshape(c, c), "tcn parameter").data_ptr() for blk in blocks]) for i in range(6)]
    check(lib.frl_tcn_chain_fwd_xt(_p(x), *[ctypes.cast(a, ctypes.c_void_p) for a in cols], _p(_f32(head_w.reshape(ch, c), "head_w")),
                                   _p(_f32(head_b, "head_b")), _p(ys[0]), _p(ys[1]), _p(ys[2]), _p(h), _p(xt), b * hw, hw, ch, float(eps),
                                   _p(ws), ws.numel(), _stream()), "frl_tcn_chain_fwd_xt")
    return (ys[0], ys[1], ys[2], h, xt) if want_xtype else (ys[0], ys[1], ys[2], h)


@_timed("tcn_block_bwd")
def tcn_block_bwd_head_supported(x, dh, head_w, dilation: int) -> bool:
    """True when the last phase block's backward can take the head's output gradient dh directly (csrc/tcn_hot_bwd4.hip, HEAD variant)."""
    b, t, cin = x.shape[0], x.shape[1], x.shape[-1]
    hw = x.numel() // (b * t * cin)
    lib = _lib.load()
    return bool(fusion_enabled("headbwd") and dilation == 4 and x.dtype == torch.bfloat16 and dh.dtype == torch.bfloat16 and
                lib.frl_tcn_hot_supported(t, cin, cin, 8, dilation, 0, _dt(x)) and
                lib.frl_tcn_hot_bwd_head_supported(b * hw, hw, int(head_w.shape[0])))


@_timed("tcn_block_bwd")
def tcn_block_bwd_head(x, dh, head_w, conv_w, conv_b, gn_w, gn_b, gate_w, gate_b, dilation: int, eps: float = 1e-5):
    """Backward of the last hot block fed with dh [B,T,HW..,Ch] (gradient of the 1x1 phase head's output) and head_w [Ch,64]: dy = dh head_w is
    formed inside the kernel.  Returns the dict of tcn_block_bwd."""
    b, t, cin = x.shape[0], x.shape[1], x.shape[-1]
    cout = conv_w.shape[0]
    hw = x.numel() // (b * t * cin)
    npix = b * hw
    ch = int(head_w.shape[0])
    _chk_rows(dh, ch, "tcn_block_bwd_head.dh")
    lib = _lib.load()
    dx = torch.empty_like(x)
    g = {k: grad_empty(v.shape, x.device) for k, v in
         dict(conv_w=conv_w, conv_b=conv_b, gn_w=gn_w, gn_b=gn_b, gate_w=gate_w, gate_b=gate_b).items()}
    ws = workspace(lib.frl_tcn_hot_bwd_head_workspace_bytes(npix), x.device)
    with span("tcn_block_bwd.main"):
        check(lib.frl_tcn_hot_bwd_head(_p(x), _p(dh), _p(_f32(head_w.reshape(ch, cin), "head_w")), ch, _p(conv_w), _p(conv_b), _p(gn_w), _p(gn_b),
                                       _p(gate_w.reshape(cout, cout)), _p(gate_b), _p(dx), _p(g["conv_w"]), _p(g["conv_b"]), _p(g["gn_w"]),
                                       _p(g["gn_b"]), _p(g["gate_w"]), _p(g["gate_b"]), npix, hw, dilation, float(eps), _p(ws), ws.numel(),
                                       _stream()), "frl_tcn_hot_bwd_head")
    g["dx"] = dx
    return g


def tcn_block_bwd(x, dy, conv_w, conv_b, gn_w, gn_b, gate_w, gate_b, proj_w, proj_b, dilation: int, groups: int,
                  eps: float = 1e-5, allow_fused: bool = True, allow_hot: bool = True, drop_mask=None, want_dx: bool = True):
    """Returns dict(dx, conv_w, conv_b, gn_w, gn_b, gate_w, gate_b[, proj_w, proj_b]) gradients.  want_dx=False (the block's input
    needs no gradient): dx is None where the kernel can skip it (hot configuration without mask), otherwise computed as usual."""
    b, t, cin = x.shape[0], x.shape[1], x.shape[-1]
    cout = conv_w.shape[0]
    hw = x.numel() // (b * t * cin)
    npix = b * hw
    lib = _lib.load()
    dev = x.device
    hot = bool(allow_fused and allow_hot and lib.frl_tcn_hot_supported(t, cin, cout, groups, dilation, int(proj_w is not None), _dt(x)))
    _check_drop_mask(drop_mask, x, hot)
    if hot:
        skip_dx = (not want_dx) and drop_mask is None and bool(lib.frl_tcn_hot_bwd_nodx_supported(npix, hw))
        dx = None if skip_dx else torch.empty_like(x)
        g = {k: grad_empty(v.shape, x.device) for k, v in
             dict(conv_w=conv_w, conv_b=conv_b, gn_w=gn_w, gn_b=gn_b, gate_w=gate_w, gate_b=gate_b).items()}
        ws = workspace(lib.frl_tcn_hot_bwd_workspace_bytes(npix), dev)
        with span("tcn_block_bwd.main"):
            check(lib.frl_tcn_hot_bwd(_p(x), _p(drop_mask), _p(dy), _p(conv_w), _p(conv_b), _p(gn_w), _p(gn_b), _p(gate_w.reshape(cout, cout)), _p(gate_b),
                                      _p(dx), _p(g["conv_w"]), _p(g["conv_b"]), _p(g["gn_w"]), _p(g["gn_b"]), _p(g["gate_w"]),
                                      _p(g["gate_b"]), npix, hw, dilation, float(eps), _p(ws), ws.numel(), _stream()), "frl_tcn_hot_bwd")
        g["dx"] = dx
        return g
    if allow_fused and lib.frl_tcn_block_bwd_fused_supported(t, cin, cout, groups, int(proj_w is not None), _dt(x)):
        dx = torch.empty_like(x)
        g = {k: grad_empty(v.shape, x.device) for k, v in
             dict(conv_w=conv_w, conv_b=conv_b, gn_w=gn_w, gn_b=gn_b, gate_w=gate_w, gate_b=gate_b).items()}
        ws = workspace(lib.frl_tcn_block_bwd_fused_workspace_bytes(npix), dev)
        with span("tcn_block_bwd.main"):
            check(lib.frl_tcn_block_bwd_fused(_p(x), _p(dy), _p(conv_w), _p(conv_b), _p(gn_w), _p(gn_b),
                                              _p(gate_w.reshape(cout, cout)), _p(gate_b), _p(dx), _p(g["conv_w"]), _p(g["conv_b"]),
                                              _p(g["gn_w"]), _p(g["gn_b"]), _p(g["gate_w"]), _p(g["gate_b"]), npix, hw, t, dilation,
                                              groups, float(eps), _p(ws), ws.numel(), _stream()), "frl_tcn_block_bwd_fused")
        g["dx"] = dx
        return g
    oshape = x.shape[:-1] + (cout,)
    dconv = torch.empty(oshape, dtype=x.dtype, device=dev)
    dgpre, normed, dres = torch.empty_like(dconv), torch.empty_like(dconv), torch.empty_like(dconv)
    dgam, dbet = grad_empty((cout,), dev), grad_empty((cout,), dev)
    gate_w2 = gate_w.reshape(cout, cout)
    ws = workspace(lib.frl_tcn_block_bwd_workspace_bytes(npix, cout), dev)
    with span("tcn_block_bwd.main"):
        check(lib.frl_tcn_block_bwd(_p(x), _p(dy), _p(conv_w), _p(conv_b), _p(gn_w), _p(gn_b), _p(gate_w2), _p(gate_b), _p(proj_w),
                                    _p(proj_b), _p(dconv), _p(dgpre), _p(normed), _p(dres), _p(dgam), _p(dbet), npix, hw, t, cin,
                                    cout, dilation, groups, float(eps), _dt(x), _p(ws), ws.numel(), _stream()), "frl_tcn_block_bwd")
    dx = torch.empty_like(x)
    ws1 = workspace(lib.frl_conv_workspace_bytes(max(cin, cout), max(cin, cout), 6), dev)
    check(lib.frl_tcn_block_bwd_data(_p(dconv), _p(dres), _p(conv_w), _p(proj_w), _p(dx), npix, hw, t, cin, cout, dilation,
                                     _dt(x), _p(ws1), ws1.numel(), _stream()), "frl_tcn_block_bwd_data")
    p = b * t * hw
    dw, dcb = grad_empty((cout, cin, 3), dev), grad_empty((cout,), dev)
    ws2 = workspace(lib.frl_conv1x1_bwd_weight_workspace_bytes(p, max(cin, cout), cout), dev)
    for k in range(3):
        check(lib.frl_conv_tap_bwd_weight(_p(dconv), None, 0, _p(x), ctypes.c_void_p(dw.data_ptr() + 4 * k), cin * 3, 3,
                                          _p(dcb) if k == 1 else None, p, cin, cout, hw, t, (k - 1) * dilation, _dt(x),
                                          _p(ws2), ws2.numel(), 0, _stream()), "frl_conv_tap_bwd_weight")
    dgw, dgb = _conv1x1_bwd_weight_impl(dgpre, normed)
    out = dict(dx=dx, conv_w=dw, conv_b=dcb, gn_w=dgam, gn_b=dbet, gate_w=dgw.reshape(gate_w.shape), gate_b=dgb)
    if proj_w is not None:
        dpw, dpb = _conv1x1_bwd_weight_impl(dres, x)
        out.update(proj_w=dpw.reshape(proj_w.shape), proj_b=dpb)
    return out


# ----------------------------------------------------------------------------------------------
# fused decoder + reconstruction loss (csrc/dec_fused.hip)
# ----------------------------------------------------------------------------------------------
def decoder_mse_supported(cz: int, hidden: int, features: int, t: torch.Tensor) -> bool:
    return bool(_lib.load().frl_decoder_mse_fused_supported(cz, hidden, features, _dt(t)))


@_timed("decoder_mse_fwd")
def decoder_mse_fwd(z, w1, b1, w2, b2, target, mask=None, want_xhat: bool = False):
    """z [..., Cz], target [..., 64] -> (stats f32 [2] = {mse, n_valid}, xhat or None)."""
    cz = z.shape[-1]
    p = z.numel() // cz
    lib = _lib.load()
    ws = workspace(lib.frl_decoder_mse_workspace_bytes(p, cz), z.device)
    out = torch.empty(2, dtype=torch.float32, device=z.device)
    xhat = torch.empty_like(target) if want_xhat else None
    check(lib.frl_decoder_mse_fwd(_p(z), _p(w1), _p(b1), _p(w2), _p(b2), _p(target), _p(mask), _p(xhat), _p(out), p, cz, _p(ws),
                                  ws.numel(), _stream()), "frl_decoder_mse_fwd")
    return out, xhat


@_timed("decoder_mse_bwd")
def decoder_mse_bwd(z, w1, b1, w2, b2, target, mask, gscale, stats):
    cz = z.shape[-1]
    p = z.numel() // cz
    lib = _lib.load()
    ws = workspace(lib.frl_decoder_mse_workspace_bytes(p, cz), z.device)
    dz = torch.empty_like(z)
    dw1, db1, dw2, db2 = (grad_empty(t.shape, z.device) for t in (w1, b1, w2, b2))
    check(lib.frl_decoder_mse_bwd(_p(z), _p(w1), _p(b1), _p(w2), _p(b2), _p(target), _p(mask), _p(gscale), _p(stats), _p(dz), _p(dw1),
                                  _p(db1), _p(dw2), _p(db2), p, cz, _p(ws), ws.numel(), _stream()), "frl_decoder_mse_bwd")
    return dz, dw1, db1, dw2, db2


_DEC_CTL = {}


def _dec_ctl(device) -> torch.Tensor:
    """Zeroed control words of the one-pass decoder kernels, one set per (device, stream): calls on one stream are ordered and every call
    leaves them zero."""
    key = (str(device), torch.cuda.current_stream().cuda_stream)
    c = _DEC_CTL.get(key)
    if c is None:
        c = _DEC_CTL[key] = torch.zeros(4, dtype=torch.int32, device=device)
    return c


@_timed("decoder_mse_fwd_bwd")
def decoder_mse_fwd_bwd(z, w1, b1, w2, b2, target, mask, grad_scale):
    """Loss and gradients in one pass (train step): -> (stats f32 [2] = {mse, n_valid}, dz, slabs).  grad_scale: device float32 scalar, the
    gradient the loss will receive (None: 1).  `slabs` = (buffer, count) goes to `decoder_mse_reduce` for the weight gradients."""
    cz = z.shape[-1]
    p = z.numel() // cz
    lib = _lib.load()
    if grad_scale is not None and (grad_scale.dtype != torch.float32 or grad_scale.numel() != 1 or grad_scale.device != z.device):
        raise ValueError("decoder_mse_fwd_bwd: grad_scale is a float32 scalar on the input's device")
    buf = torch.empty(lib.frl_decoder_mse_onepass_bytes(p, cz), dtype=torch.uint8, device=z.device)     # (its own: it outlives the call)
    out = torch.empty(2, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    nslab = ctypes.c_int(0)
    check(lib.frl_decoder_mse_fwd_bwd(_p(z), _p(w1), _p(b1), _p(w2), _p(b2), _p(target), _p(mask), _p(grad_scale), _p(out), _p(dz), _p(buf),
                                      buf.numel(), _p(_dec_ctl(z.device)), ctypes.cast(ctypes.byref(nslab), ctypes.c_void_p), p, cz, _stream()),
          "frl_decoder_mse_fwd_bwd")
    return out, dz, (buf, int(nslab.value))


@_timed("decoder_mse_reduce")
def decoder_mse_reduce(slabs, w1, b1, w2, b2):
    """The weight gradients of a `decoder_mse_fwd_bwd` call from its slabs: parked inside `deferred_reductions` (no launch), else one launch."""
    buf, nslab = slabs
    cz = w1.shape[-1]
    if _DEFER["on"]:
        _DEFER["keep"].append(buf)                              # read by the flush
    dw1, db1, dw2, db2 = (grad_empty(t.shape, buf.device) for t in (w1, b1, w2, b2))
    check(_lib.load().frl_decoder_mse_reduce(_p(buf), nslab, _p(dw1), _p(db1), _p(dw2), _p(db2), cz, _stream()), "frl_decoder_mse_reduce")
    return dw1, db1, dw2, db2


# ----------------------------------------------------------------------------------------------
# code-map decoding (csrc/codes.hip)
# ----------------------------------------------------------------------------------------------
def _index_flag(device) -> torch.Tensor:
    """The per-device word that `index_errors()` reads (see sanitize_indices)."""
    device = torch.device(device)
    flag = _INDEX_FLAG.get(device)
    if flag is None:
        flag = _INDEX_FLAG[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return flag


@_timed("decode_codes")
def decode_codes(idx: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """idx [...] int32 | int64 codes, table [K, F] float32 | bfloat16 (decoded codebook rows) -> table[idx] [..., F] in table.dtype.
    Out-of-range indices follow the sparse-op convention (sanitize_indices), inside the kernel: [-K, 0) wraps, anything else is clamped
    and flagged for `index_errors()`; with FRL_HIP_CHECK_INDICES=1 this call raises IndexError on the spot (one sync per call)."""
    import os
    if table.dim() != 2:
        raise ValueError(f"decode_codes: table must be [K, F], got {tuple(table.shape)}")
    k, f = table.shape
    _chk_rows(table, f, "decode_codes.table")
    if not idx.is_cuda or idx.device != table.device:
        raise _lib.FrlHipError("decode_codes: idx must live on the table's GPU (no CPU fallback)")
    if idx.dtype == torch.int64:
        idx = idx.clamp(-k - 1, k).to(torch.int32)                  # (out-of-range stays out of range, and fits int32)
    elif idx.dtype != torch.int32:
        raise TypeError(f"decode_codes: idx must be int32 or int64, got {idx.dtype}")
    idx = idx.contiguous()
    out = torch.empty(tuple(idx.shape) + (f,), dtype=table.dtype, device=table.device)
    p = idx.numel()
    if p == 0:
        return out
    check_now = os.environ.get("FRL_HIP_CHECK_INDICES", "0") == "1"
    flag = torch.zeros(1, dtype=torch.int32, device=table.device) if check_now else _index_flag(table.device)
    check(_lib.load().frl_decode_codes(_p(idx), _p(table), _p(out), p, k, f, _dt(table), _p(flag), _stream()), "frl_decode_codes")
    if check_now:
        _index_flag(table.device).bitwise_or_(flag)
        if bool(flag.item()):
            raise IndexError(f"decode_codes: code index out of range for {k} codes")
    return out


# ----------------------------------------------------------------------------------------------
# sparse-location gather + InfoNCE over mined pairs (csrc/contrastive.hip)
# ----------------------------------------------------------------------------------------------
@_timed("gather_locations")
def gather_locations(feature: torch.Tensor, coords: torch.Tensor) -> torch.Tensor:
    """feature [C, H, W] with any strides (float32 | bfloat16), coords int64 [N, 2] (row, col) -> [N, C] contiguous."""
    if not feature.is_cuda:
        raise _lib.FrlHipError("gather_locations: tensor must live on the GPU (no CPU fallback)")
    c, h, w = feature.shape
    if coords.dtype != torch.int64 or not coords.is_contiguous() or coords.device != feature.device:
        raise ValueError("gather_locations: coords must be a contiguous int64 [N, 2] tensor on the feature's device")
    n = coords.shape[0]
    out = torch.empty(n, c, dtype=feature.dtype, device=feature.device)
    sc, sh, sw = feature.stride()
    check(_lib.load().frl_gather_locations_fwd(_p(feature), sc, sh, sw, c, h, w, _p(coords), n, _p(out), _dt(feature), _stream()),
          "frl_gather_locations_fwd")
    return out


@_timed("segment_sum_rows")
def segment_sum_rows(vals: torch.Tensor, order: Optional[torch.Tensor], keys_sorted: torch.Tensor, out: torch.Tensor, accumulate: bool = False):
    """out[key] (+)= sum of vals[order[i]] over each run of equal keys_sorted[i]; rows are summed in list order (reproducible)."""
    m, d = vals.shape
    if vals.dtype != torch.float32 or not vals.is_contiguous() or out.dtype != torch.float32 or not out.is_contiguous() or out.shape[-1] != d:
        raise ValueError("segment_sum_rows: vals [M, D] and out [.., D] must be contiguous float32")
    for t in (order, keys_sorted):
        if t is not None and (t.dtype != torch.int64 or not t.is_contiguous() or t.numel() != m):
            raise ValueError("segment_sum_rows: order / keys must be contiguous int64 [M]")
    check(_lib.load().frl_segment_sum_rows(_p(vals), _p(order), _p(keys_sorted), m, d, _p(out), d, int(accumulate), _stream()),
          "frl_segment_sum_rows")
    return out


@_timed("infonce_fwd")
def infonce_fwd(emb, pairs, weights, is_pos, seg, temperature: float, sim: int, want_coef: bool = True):
    """Pairs sorted by anchor with segment bounds `seg` -> (loss f32 [1], sims [T], coef [T] or None)."""
    t, d = pairs.shape[0], emb.shape[1]
    sims = torch.empty(t, dtype=torch.float32, device=emb.device)
    logits = torch.empty_like(sims)
    nseg = seg.numel() - 1
    loss_a = torch.empty(nseg, dtype=torch.float32, device=emb.device)
    coef = torch.empty_like(sims) if want_coef else None
    loss = torch.empty(1, dtype=torch.float32, device=emb.device)
    check(_lib.load().frl_infonce_fwd(_p(emb), d, _p(pairs), _p(weights), _p(is_pos), t, _p(seg), nseg, float(temperature), int(sim),
                                      _p(sims), _p(logits), _p(loss_a), _p(coef), _p(loss), _stream()), "frl_infonce_fwd")
    return loss, sims, coef


@_timed("infonce_bwd")
def infonce_pair_grads(emb, pairs, sims, coef, gscale, nseg: int, temperature: float, sim: int):
    t, d = pairs.shape[0], emb.shape[1]
    ga = torch.empty(t, d, dtype=torch.float32, device=emb.device)
    gb = torch.empty_like(ga)
    check(_lib.load().frl_infonce_pair_grads(_p(emb), d, _p(pairs), _p(sims), _p(coef), _p(gscale), t, nseg, float(temperature), int(sim),
                                             _p(ga), _p(gb), _stream()), "frl_infonce_pair_grads")
    return ga, gb


# ----------------------------------------------------------------------------------------------
# cross-patch spectral negatives and pair similarities (csrc/spectral_negatives.hip)
# ----------------------------------------------------------------------------------------------
SPECTRAL_NEG_MAX_WIDTH = 256


def _flag_for(device):
    """(flag word handed to the kernel, check_now): a private word with FRL_HIP_CHECK_INDICES=1, the shared one otherwise."""
    import os
    check_now = os.environ.get("FRL_HIP_CHECK_INDICES", "0") == "1"
    return (torch.zeros(1, dtype=torch.int32, device=device) if check_now else _index_flag(device)), check_now


def _flag_done(flag: torch.Tensor, check_now: bool, what: str) -> None:
    if check_now:
        _index_flag(flag.device).bitwise_or_(flag)
        if bool(flag.item()):
            raise IndexError(what)


@_timed("spectral_negatives")
def spectral_negatives(spec: torch.Tensor, offsets: torch.Tensor, n_patches: int, n_per: int, draws: torch.Tensor, tau: float, min_w: float):
    """spec [N, C] float32 (C <= 256), offsets [S + 1] int32 on the device, draws [Q, 2] int32 with Q = n_per S (S - 1) -> (pairs [Q, 2] int64,
    dist [Q], weights [Q]) in one launch; include/frl_hip.h (frl_spectral_negatives) has the definitions.  A negative draw is taken as 0
    and flagged for `index_errors()` (FRL_HIP_CHECK_INDICES=1: IndexError on the spot, one sync).  No host read."""
    if not spec.is_cuda:
        raise _lib.FrlHipError("spectral_negatives: tensors must live on the GPU (no CPU fallback)")
    if spec.dim() != 2 or spec.dtype != torch.float32 or not spec.is_contiguous():
        raise ValueError(f"spectral_negatives: spec must be a contiguous float32 [N, C] tensor, got {tuple(spec.shape)} {spec.dtype}")
    n, c = spec.shape
    s, n_per = int(n_patches), int(n_per)
    q = n_per * s * (s - 1)
    for t, shape, name in ((offsets, (s + 1,), "offsets"), (draws, (q, 2), "draws")):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != spec.device:
            raise ValueError(f"spectral_negatives: {name} must be a contiguous int32 {list(shape)} tensor on the GPU of spec")
    pairs = torch.empty(q, 2, dtype=torch.int64, device=spec.device)
    dist = torch.empty(q, dtype=torch.float32, device=spec.device)
    weights = torch.empty_like(dist)
    if q == 0:
        return pairs, dist, weights
    flag, check_now = _flag_for(spec.device)
    check(_lib.load().frl_spectral_negatives(_p(spec), n, c, _p(offsets), s, n_per, _p(draws), q, float(tau), float(min_w), _p(pairs), _p(dist),
                                             _p(weights), _p(flag), _stream()), "frl_spectral_negatives")
    _flag_done(flag, check_now, "spectral_negatives: a draw outside [0, 2^31) or patch bounds outside the spectral rows")
    return pairs, dist, weights


@_timed("pair_sims")
def pair_sims(emb: torch.Tensor, pairs: torch.Tensor, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """emb [N, D] float32 (D <= 256), pairs [T, 2] int64 -> sims [T] = -|emb[a] - emb[b]|^2 / D.  stats: 4 float64 on the device that
    receive (T, mean, unbiased std, 0) when T > 0; include/frl_hip.h (frl_pair_sims).  Rows out of range follow `sanitize_indices`,
    inside the kernel.  No host read."""
    if not emb.is_cuda:
        raise _lib.FrlHipError("pair_sims: tensors must live on the GPU (no CPU fallback)")
    if emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous():
        raise ValueError(f"pair_sims: emb must be a contiguous float32 [N, D] tensor, got {tuple(emb.shape)} {emb.dtype}")
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64 or not pairs.is_contiguous() or pairs.device != emb.device:
        raise ValueError("pair_sims: pairs must be a contiguous int64 [T, 2] tensor on the GPU of emb")
    if stats is not None and (stats.dtype != torch.float64 or stats.numel() != 4 or not stats.is_contiguous() or stats.device != emb.device):
        raise ValueError("pair_sims: stats must be 4 contiguous float64 on the GPU of emb")
    n, d = emb.shape
    t = pairs.shape[0]
    sims = torch.empty(t, dtype=torch.float32, device=emb.device)
    if t == 0:
        return sims
    lib = _lib.load()
    nbytes = lib.frl_pair_sims_workspace_bytes(t) if stats is not None else 0
    ws = workspace(nbytes, emb.device) if nbytes else None
    flag, check_now = _flag_for(emb.device)
    check(lib.frl_pair_sims(_p(emb), n, d, _p(pairs), t, _p(sims), _p(stats), _p(flag), _p(ws), nbytes, _stream()), "frl_pair_sims")
    _flag_done(flag, check_now, f"pair_sims: pair row out of range for {n} rows")
    return sims


# ----------------------------------------------------------------------------------------------
# VICReg variance-covariance loss (csrc/vicreg.hip)
# ----------------------------------------------------------------------------------------------
def _chk_vicreg(x: torch.Tensor, name: str):
    if not x.is_cuda:
        raise _lib.FrlHipError(f"{name}: tensor must live on the GPU (no CPU fallback)")
    if x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 2 or not (1 <= x.shape[1] <= 128):
        raise ValueError(f"{name}: expected contiguous rows [N >= 2, 1 <= D <= 128], got {tuple(x.shape)} stride {x.stride()}")


@_timed("vicreg_fwd")
def vicreg_fwd(x: torch.Tensor, variance_weight: float = 1.0, covariance_weight: float = 1.0, variance_target: float = 1.0,
               eps: float = 1e-4, want_grad: bool = True):
    """x [N, D] (float32 | bfloat16) -> (losses f32 [3] = total, variance_loss, covariance_loss; cov f32 [D, D]; centre f32 [2, D] = the
    pivot p (mean of the first 64 rows) | mean - p); cov and centre (what vicreg_bwd reads) are None unless want_grad."""
    _chk_vicreg(x, "vicreg_fwd")
    n, d = x.shape
    losses = torch.empty(3, dtype=torch.float32, device=x.device)
    cov = torch.empty(d, d, dtype=torch.float32, device=x.device) if want_grad else None
    centre = torch.empty(2, d, dtype=torch.float32, device=x.device) if want_grad else None
    lib = _lib.load()
    ws = workspace(lib.frl_vicreg_workspace_bytes(n, d), x.device)
    check(lib.frl_vicreg_fwd(_p(x), n, d, _dt(x), float(variance_weight), float(covariance_weight), float(variance_target), float(eps),
                             _p(losses), _p(cov), _p(centre), _p(ws), ws.numel(), _stream()), "frl_vicreg_fwd")
    return losses, cov, centre


@_timed("vicreg_bwd")
def vicreg_bwd(x: torch.Tensor, cov: torch.Tensor, centre: torch.Tensor, g3: torch.Tensor, variance_weight: float = 1.0,
               covariance_weight: float = 1.0, variance_target: float = 1.0, eps: float = 1e-4) -> torch.Tensor:
    """dx [N, D] in the dtype of x for the upstream gradients g3 f32 [3] of (total, variance_loss, covariance_loss), read on the device."""
    _chk_vicreg(x, "vicreg_bwd")
    n, d = x.shape
    _chk_f32_on("vicreg_bwd", "x", x.device, (cov, (d, d), "cov"), (centre, (2, d), "centre"), (g3, (3,), "g3"))
    dx = torch.empty_like(x)
    check(_lib.load().frl_vicreg_bwd(_p(x), _p(cov), _p(centre), _p(g3), n, d, _dt(x), float(variance_weight), float(covariance_weight),
                                     float(variance_target), float(eps), _p(dx), _stream()), "frl_vicreg_bwd")
    return dx


# ----------------------------------------------------------------------------------------------
# type-local spectral baseline (csrc/type_baseline.hip)
# ----------------------------------------------------------------------------------------------
TYPE_BASELINE_MAX_K, TYPE_BASELINE_MAX_NBRS, TYPE_BASELINE_MAX_C = 64, 64, 256


def chk_type_baseline(z_k: torch.Tensor, spec: torch.Tensor, k_nbrs: int) -> int:
    """Every limit of frl_type_baseline that needs no device (ValueError); -> k = min(k_nbrs, N - 1)."""
    if z_k.dim() != 2 or spec.dim() != 3:
        raise ValueError(f"type_baseline: expected z_k [N, K] and spec [N, T, C], got {tuple(z_k.shape)} and {tuple(spec.shape)}")
    if z_k.shape[0] != spec.shape[0]:
        raise ValueError(f"type_baseline: z_k has {z_k.shape[0]} rows and spec {spec.shape[0]}")
    n, kw = z_k.shape
    t, c = spec.shape[1], spec.shape[2]
    if n < 2:
        raise ValueError("type_baseline: needs N >= 2 anchors (an anchor is never its own neighbour; the reference gives NaN at N = 1)")
    if not 1 <= kw <= TYPE_BASELINE_MAX_K:
        raise ValueError(f"type_baseline: the projected width K must be in 1..{TYPE_BASELINE_MAX_K}, got {kw}")
    if not 1 <= int(k_nbrs) <= TYPE_BASELINE_MAX_NBRS:
        raise ValueError(f"type_baseline: k_nbrs must be in 1..{TYPE_BASELINE_MAX_NBRS} (one lane per neighbour), got {k_nbrs}")
    if not 1 <= c <= TYPE_BASELINE_MAX_C:
        raise ValueError(f"type_baseline: 1 <= C <= {TYPE_BASELINE_MAX_C} spectral channels, got {c}")
    if t < 1 or t * c >= 2 ** 31 or n * max(kw, c) >= 2 ** 31:
        raise ValueError(f"type_baseline: T must be positive and T * C, N * K and N * C below 2^31, got {tuple(spec.shape)}")
    for x, name in ((z_k, "z_k"), (spec, "spec")):
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"type_baseline: {name} must be a contiguous float32 tensor, got {x.dtype} stride {x.stride()}")
    return min(int(k_nbrs), n - 1)


@_timed("type_baseline")
def type_baseline(z_k: torch.Tensor, spec: torch.Tensor, k_nbrs: int = 20):
    """z_k [N, K] float32, spec [N, T, C] float32 -> (spec - s_hat [N, T, C] float32, s_hat [N, C] float32, topk_idx [N, k] int64),
    k = min(k_nbrs, N - 1).  include/frl_hip.h (frl_type_baseline) has the definitions.  No host read."""
    k = chk_type_baseline(z_k, spec, k_nbrs)
    if not z_k.is_cuda or not spec.is_cuda:
        raise _lib.FrlHipError("type_baseline: tensors must live on the GPU (no CPU fallback)")
    if z_k.device != spec.device:
        raise ValueError("type_baseline: z_k and spec must be on one device")
    n, kw = z_k.shape
    t, c = spec.shape[1], spec.shape[2]
    out = torch.empty_like(spec)
    s_hat = torch.empty((n, c), dtype=torch.float32, device=spec.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=spec.device)
    lib = _lib.load()
    ws = workspace(lib.frl_type_baseline_workspace_bytes(n, c), spec.device)
    check(lib.frl_type_baseline(_p(z_k), _p(spec), n, kw, t, c, k, _p(out), _p(s_hat), _p(idx), _p(ws), ws.numel(), _stream()),
          "frl_type_baseline")
    return out, s_hat, idx


# ----------------------------------------------------------------------------------------------
# phase-type leakage loss (csrc/leakage.hip)
# ----------------------------------------------------------------------------------------------
LEAKAGE_MAX_P, LEAKAGE_MAX_DZ = 64, 128


def chk_leakage(h: torch.Tensor, z: torch.Tensor, name: str = "leakage"):
    """Every limit of frl_leakage_fwd that needs no device (ValueError)."""
    if h.dim() != 2 or z.dim() != 2 or h.shape[0] != z.shape[0] or h.shape[0] < 1:
        raise ValueError(f"{name}: expected h [N, P] and z [N, Dz] with N >= 1, got {tuple(h.shape)} and {tuple(z.shape)}")
    if not 1 <= h.shape[1] <= LEAKAGE_MAX_P:
        raise ValueError(f"{name}: supports 1 <= P <= {LEAKAGE_MAX_P} columns of h, got {h.shape[1]}")
    if not 1 <= z.shape[1] <= LEAKAGE_MAX_DZ:
        raise ValueError(f"{name}: supports 1 <= Dz <= {LEAKAGE_MAX_DZ} columns of z, got {z.shape[1]}")
    for x, what in ((h, "h"), (z, "z")):
        if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous float32 or bfloat16 tensor, got {x.dtype} stride {x.stride()}")


def _chk_leakage_dev(h_like: torch.Tensor, z: torch.Tensor, name: str):
    if not h_like.is_cuda or not z.is_cuda:
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    if h_like.device != z.device:
        raise ValueError(f"{name}: h and z must be on one device")


@_timed("leakage_fwd")
def leakage_fwd(h: torch.Tensor, z: torch.Tensor, want_grad: bool = True):
    """h [N, P], z [N, Dz] (float32 | bfloat16 each) -> (stats f32 [2] = loss, 1 / (max(N-1, 1) loss) or 0; cmat f32 [P, Dz] = the
    cross-covariance; centre f32 [2, Dz] = the pivot of z | mean - pivot); cmat and centre (what leakage_bwd reads) are None unless
    want_grad."""
    chk_leakage(h, z, "leakage_fwd")
    _chk_leakage_dev(h, z, "leakage_fwd")
    n, p = h.shape
    dz = z.shape[1]
    stats = torch.empty(2, dtype=torch.float32, device=h.device)
    cmat = torch.empty(p, dz, dtype=torch.float32, device=h.device) if want_grad else None
    centre = torch.empty(2, dz, dtype=torch.float32, device=h.device) if want_grad else None
    lib = _lib.load()
    ws = workspace(lib.frl_leakage_workspace_bytes(n, p, dz), h.device)
    check(lib.frl_leakage_fwd(_p(h), _dt(h), _p(z), _dt(z), n, p, dz, _p(stats), _p(cmat), _p(centre), _p(ws), ws.numel(), _stream()),
          "frl_leakage_fwd")
    return stats, cmat, centre


@_timed("leakage_bwd")
def leakage_bwd(z: torch.Tensor, cmat: torch.Tensor, centre: torch.Tensor, stats: torch.Tensor, g: torch.Tensor, p: int,
                dtype: torch.dtype) -> torch.Tensor:
    """dh [N, p] in `dtype` for the upstream gradient g f32 [1], read on the device; zeros where the loss is zero."""
    n, dz = z.shape
    dh = torch.empty((n, p), dtype=dtype, device=z.device)
    chk_leakage(dh, z, "leakage_bwd")
    _chk_leakage_dev(dh, z, "leakage_bwd")
    _chk_f32_on("leakage_bwd", "z", z.device, (cmat, (p, dz), "cmat"), (centre, (2, dz), "centre"), (stats, (2,), "stats"), (g, (1,), "g"))
    check(_lib.load().frl_leakage_bwd(_p(z), _dt(z), _p(cmat), _p(centre), _p(stats), _p(g), n, p, dz, _p(dh), _dt(dh), _stream()),
          "frl_leakage_bwd")
    return dh


# ----------------------------------------------------------------------------------------------
# soft-neighbourhood matching loss (csrc/soft_neighborhood.hip)
# ----------------------------------------------------------------------------------------------
SOFT_NBR_MAX_M, SOFT_NBR_MAX_WIDTH = 32, 256


def _chk_soft_nbr(name: str, tau_ref: float, tau_learned: float, min_valid_per_row: int):
    if int(min_valid_per_row) < 2:
        raise ValueError(f"min_valid_per_row must be >= 2, got {min_valid_per_row}")
    if not (tau_ref > 0 and tau_learned > 0):
        raise ValueError(f"{name}: temperatures must be positive, got tau_ref={tau_ref} tau_learned={tau_learned}")


def _soft_nbr_weights(weights: Optional[torch.Tensor], b: int, device, name: str):
    if weights is None:
        return None
    if weights.dtype != torch.float32 or not weights.is_contiguous() or weights.shape != (b,) or weights.device != device:
        raise ValueError(f"{name}: pair weights must be a contiguous float32 [{b}] tensor on the device of the inputs")
    return weights


@_timed("soft_nbr_fwd")
def soft_nbr_fwd(d_reference: torch.Tensor, d_learned: torch.Tensor, mask: torch.Tensor, weights: Optional[torch.Tensor] = None,
                 tau_ref: float = 1.0, tau_learned: float = 1.0, min_valid_per_row: int = 2, want_coef: bool = True):
    """d_reference, d_learned [B, M, M] float32, mask [B, M, M] bool, weights [B] float32 or None -> (out2 f32 [2] = loss, sum of the
    active pairs' weights; stats f64 [8] = loss, sum_w, active pairs, contributing rows, sum of their unmasked counts, sum H(p), sum H(q), 0;
    pairstat f32 [B, 6] = L_b, rows_b, ...; coef f32 [B, M, M] = (p - q) / tau_learned, None unless want_coef)."""
    _chk_soft_nbr("soft_nbr_fwd", tau_ref, tau_learned, min_valid_per_row)
    if not (d_reference.is_cuda and d_learned.is_cuda and mask.is_cuda):
        raise _lib.FrlHipError("soft_nbr_fwd: tensors must live on the GPU (no CPU fallback)")
    if d_reference.dim() != 3 or d_reference.shape[1] != d_reference.shape[2] or d_reference.shape[0] < 1 or d_reference.shape[1] < 1:
        raise ValueError(f"soft_nbr_fwd: expected [B >= 1, M >= 1, M] distances, got {tuple(d_reference.shape)}")
    for t, dt, name in ((d_reference, torch.float32, "d_reference"), (d_learned, torch.float32, "d_learned"), (mask, torch.bool, "mask")):
        if t.dtype != dt or t.shape != d_reference.shape or not t.is_contiguous() or t.device != d_reference.device:
            raise ValueError(f"soft_nbr_fwd: {name} must be a contiguous {dt} {tuple(d_reference.shape)} tensor on {d_reference.device}")
    b, m, _ = d_reference.shape
    weights = _soft_nbr_weights(weights, b, d_reference.device, "soft_nbr_fwd")
    pairstat, out2, stats = _pair_outputs(b, 6, d_reference.device)
    coef = torch.empty_like(d_learned) if want_coef else None
    check(_lib.load().frl_soft_nbr_fwd(_p(d_reference), _p(d_learned), _p(mask), _p(weights), b, m, 1.0 / float(tau_ref), 1.0 / float(tau_learned),
                                       int(min_valid_per_row), _p(pairstat), _p(coef), _p(out2), _p(stats), _stream()), "frl_soft_nbr_fwd")
    return out2, stats, pairstat, coef


@_timed("soft_nbr_bwd")
def soft_nbr_bwd(coef: torch.Tensor, pairstat: torch.Tensor, weights: Optional[torch.Tensor], out2: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """d loss / d d_learned [B, M, M] = g[0] * w_b / (sum_w * rows_b) * coef for the outputs of soft_nbr_fwd; g: float32 [1] on the device."""
    if not coef.is_cuda:
        raise _lib.FrlHipError("soft_nbr_bwd: tensors must live on the GPU (no CPU fallback)")
    b, m, _ = coef.shape
    _chk_f32_on("soft_nbr_bwd", "coef", coef.device, (coef, (b, m, m), "coef"), (pairstat, (b, 6), "pairstat"), (out2, (2,), "out2"), (g, (1,), "g"))
    weights = _soft_nbr_weights(weights, b, coef.device, "soft_nbr_bwd")
    grad = torch.empty_like(coef)
    check(_lib.load().frl_soft_nbr_bwd(_p(coef), _p(pairstat), _p(weights), _p(out2), _p(g), b, m, _p(grad), _stream()), "frl_soft_nbr_bwd")
    return grad


def _chk_soft_nbr_gathered(name: str, ref, emb, rows, lengths, checked: bool):
    """Shape limits first (they hold on any device), then the device, then the layouts -> (B, M, rows [4, B, M] inside [0, R))."""
    if ref.dim() != 2 or emb.dim() != 2 or ref.shape[0] != emb.shape[0]:
        raise ValueError(f"{name}: expected ref [R, C] and emb [R, D], got {tuple(ref.shape)} and {tuple(emb.shape)}")
    if rows.dim() != 3 or rows.shape[0] != 4:
        raise ValueError(f"{name}: the row indices come stacked as [4, B, M] (ref a, ref b, emb a, emb b), got {tuple(rows.shape)}")
    _, b, m = rows.shape
    if m > SOFT_NBR_MAX_M:
        raise ValueError(f"{name}: the gathered form supports M <= {SOFT_NBR_MAX_M} positions per pair, got M = {m}")
    if ref.shape[1] > SOFT_NBR_MAX_WIDTH or emb.shape[1] > SOFT_NBR_MAX_WIDTH:
        raise ValueError(f"{name}: the gathered form supports C <= {SOFT_NBR_MAX_WIDTH} and D <= {SOFT_NBR_MAX_WIDTH}, got C = {ref.shape[1]}, "
                         f"D = {emb.shape[1]}")
    if not (ref.is_cuda and emb.is_cuda and rows.is_cuda and lengths.is_cuda):
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    if b < 1 or m < 1 or ref.shape[0] < 1 or ref.shape[1] < 1 or emb.shape[1] < 1:
        raise ValueError(f"{name}: needs at least one pair, position, row and column")
    if ref.dtype != torch.float32 or not ref.is_contiguous() or emb.dtype not in (torch.float32, torch.bfloat16) or not emb.is_contiguous():
        raise ValueError(f"{name}: ref must be contiguous float32 rows and emb contiguous float32 or bfloat16 rows")
    if rows.dtype != torch.int64 or not rows.is_contiguous() or lengths.dtype != torch.int64 or not lengths.is_contiguous() or lengths.shape != (b,):
        raise ValueError(f"{name}: row indices [4, {b}, {m}] and lengths [{b}] must be contiguous int64")
    if not checked:
        rows = sanitize_indices(rows, ref.shape[0], name + ": row indices")
    return b, m, rows


@_timed("soft_nbr_gathered_fwd")
def soft_nbr_gathered_fwd(ref: torch.Tensor, emb: torch.Tensor, rows: torch.Tensor, lengths: torch.Tensor, exclude_diagonal: bool,
                          weights: Optional[torch.Tensor] = None, tau_ref: float = 1.0, tau_learned: float = 1.0, min_valid_per_row: int = 2,
                          checked: bool = False):
    """ref [R, C] float32, emb [R, D] float32 | bfloat16, rows [4, B, M] int64 (ref a, ref b, emb a, emb b), lengths [B] int64 ->
    (out2, stats, pairstat as soft_nbr_fwd, rows sanitised into [0, R)).  M <= 32, C <= 256, D <= 256."""
    _chk_soft_nbr("soft_nbr_gathered_fwd", tau_ref, tau_learned, min_valid_per_row)
    b, m, rows = _chk_soft_nbr_gathered("soft_nbr_gathered_fwd", ref, emb, rows, lengths, checked)
    weights = _soft_nbr_weights(weights, b, ref.device, "soft_nbr_gathered_fwd")
    pairstat, out2, stats = _pair_outputs(b, 6, ref.device)
    check(_lib.load().frl_soft_nbr_gathered_fwd(_p(ref), ref.shape[1], _p(emb), emb.shape[1], _dt(emb), _p(rows[0]), _p(rows[1]), _p(rows[2]),
                                                _p(rows[3]), _p(lengths), _p(weights), b, m, int(bool(exclude_diagonal)), 1.0 / float(tau_ref),
                                                1.0 / float(tau_learned), int(min_valid_per_row), _p(pairstat), _p(out2), _p(stats), _stream()),
          "frl_soft_nbr_gathered_fwd")
    return out2, stats, pairstat, rows


@_timed("soft_nbr_gathered_bwd")
def soft_nbr_gathered_bwd(ref: torch.Tensor, emb: torch.Tensor, rows: torch.Tensor, lengths: torch.Tensor, exclude_diagonal: bool,
                          weights: Optional[torch.Tensor], tau_ref: float, tau_learned: float, min_valid_per_row: int, pairstat: torch.Tensor,
                          out2: torch.Tensor, g: torch.Tensor, checked: bool = False) -> torch.Tensor:
    """Gradient rows float32 [2, B, M, D] (role a = rows[2], then role b = rows[3]) for the outputs of soft_nbr_gathered_fwd; fold them
    into d emb with segment_sum_rows.  g: float32 [1] on the device."""
    _chk_soft_nbr("soft_nbr_gathered_bwd", tau_ref, tau_learned, min_valid_per_row)
    b, m, rows = _chk_soft_nbr_gathered("soft_nbr_gathered_bwd", ref, emb, rows, lengths, checked)
    _chk_f32_on("soft_nbr_gathered_bwd", "ref", ref.device, (pairstat, (b, 6), "pairstat"), (out2, (2,), "out2"), (g, (1,), "g"))
    weights = _soft_nbr_weights(weights, b, ref.device, "soft_nbr_gathered_bwd")
    grows = torch.empty(2, b, m, emb.shape[1], dtype=torch.float32, device=ref.device)
    check(_lib.load().frl_soft_nbr_gathered_bwd(_p(ref), ref.shape[1], _p(emb), emb.shape[1], _dt(emb), _p(rows[0]), _p(rows[1]), _p(rows[2]),
                                                _p(rows[3]), _p(lengths), _p(weights), b, m, int(bool(exclude_diagonal)), 1.0 / float(tau_ref),
                                                1.0 / float(tau_learned), int(min_valid_per_row), _p(pairstat), _p(out2), _p(g), _p(grows),
                                                _stream()), "frl_soft_nbr_gathered_bwd")
    return grows


# ----------------------------------------------------------------------------------------------
# EVT soft-neighbourhood loss (csrc/evt_soft_neighborhood.hip)
# ----------------------------------------------------------------------------------------------
EVT_SOFT_NBR_MAX_WIDTH = 256


def _chk_evt_soft_nbr(name: str, emb, idx, table, code_weights, seg, seg_host, tau_ref: float, tau_learned: float):
    """Shape limits first (they hold on any device), then the device, then the layouts -> (N, D, K, segments)."""
    if emb.dim() != 2 or idx.dim() != 1 or idx.shape[0] != emb.shape[0]:
        raise ValueError(f"{name}: expected emb [N, D] and idx [N], got {tuple(emb.shape)} and {tuple(idx.shape)}")
    n, d = emb.shape
    if d > EVT_SOFT_NBR_MAX_WIDTH:
        raise ValueError(f"{name}: supports D <= {EVT_SOFT_NBR_MAX_WIDTH}, got D = {d}")
    if not (tau_ref > 0 and tau_learned > 0):
        raise ValueError(f"{name}: temperatures must be positive, got tau_ref={tau_ref} tau_learned={tau_learned}")
    if not (emb.is_cuda and idx.is_cuda and table.is_cuda and code_weights.is_cuda and seg.is_cuda):
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    if n < 1 or d < 1:
        raise ValueError(f"{name}: needs at least one row and one column")
    if emb.dtype not in (torch.float32, torch.bfloat16) or not emb.is_contiguous():
        raise ValueError(f"{name}: emb must be contiguous float32 or bfloat16 rows")
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.device != emb.device:
        raise ValueError(f"{name}: idx must be a contiguous int32 [{n}] tensor on the device of emb")
    k = table.shape[0] if table.dim() == 2 else 0
    if table.dim() != 2 or table.shape[1] != k or k < 1 or table.dtype != torch.float32 or not table.is_contiguous() or table.device != emb.device:
        raise ValueError(f"{name}: the similarity table must be a contiguous float32 [K, K] tensor on the device of emb")
    if code_weights.dtype != torch.float32 or code_weights.shape != (k,) or not code_weights.is_contiguous() or code_weights.device != emb.device:
        raise ValueError(f"{name}: the code weights must be a contiguous float32 [{k}] tensor on the device of emb")
    if seg_host.is_cuda or seg_host.dtype != torch.int32 or seg_host.dim() != 1 or seg_host.numel() < 2 or not seg_host.is_contiguous():
        raise ValueError(f"{name}: the host segment offsets must be a contiguous int32 [segments + 1] CPU tensor")
    if seg.dtype != torch.int32 or seg.shape != seg_host.shape or not seg.is_contiguous() or seg.device != emb.device:
        raise ValueError(f"{name}: the device segment offsets must be a contiguous int32 [{seg_host.numel()}] tensor on the device of emb")
    return n, d, k, seg_host.numel() - 1


@_timed("evt_soft_nbr_fwd")
def evt_soft_nbr_fwd(emb: torch.Tensor, idx: torch.Tensor, table: torch.Tensor, code_weights: torch.Tensor, seg: torch.Tensor,
                     seg_host: torch.Tensor, tau_ref: float = 0.5, tau_learned: float = 0.5, min_valid_anchors: int = 4):
    """emb [N, D] float32 | bfloat16, idx [N] int32 code indices (-1 = unknown; >= K is treated as unknown and flagged for
    `index_errors()`), table [K, K] float32, code_weights [K] float32, seg int32 [S + 1] row offsets on the device and seg_host the same
    on the host (validated there) -> (segout f32 [S, 2] = per-segment loss, active weight; segstat f64 [S, 12]; rowstat f32 [N, 10]):
    include/frl_hip.h names the columns.  With FRL_HIP_CHECK_INDICES=1 an idx >= K raises IndexError on the spot (one sync per call)."""
    import os
    n, d, k, s = _chk_evt_soft_nbr("evt_soft_nbr_fwd", emb, idx, table, code_weights, seg, seg_host, tau_ref, tau_learned)
    dev = emb.device
    rowstat = torch.empty(n, 10, dtype=torch.float32, device=dev)
    segout = torch.empty(s, 2, dtype=torch.float32, device=dev)
    segstat = torch.empty(s, 12, dtype=torch.float64, device=dev)
    check_now = os.environ.get("FRL_HIP_CHECK_INDICES", "0") == "1"
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if check_now else _index_flag(dev)
    check(_lib.load().frl_evt_soft_nbr_fwd(_p(emb), _dt(emb), n, d, _p(idx), _p(table), _p(code_weights), k, _p(seg), _p(seg_host), s,
                                           1.0 / float(tau_ref), 1.0 / float(tau_learned), int(min_valid_anchors), _p(rowstat), _p(segout),
                                           _p(segstat), _p(flag), _stream()), "frl_evt_soft_nbr_fwd")
    if check_now:
        _index_flag(dev).bitwise_or_(flag)
        if bool(flag.item()):
            raise IndexError(f"evt_soft_nbr_fwd: code index out of range for {k} codes")
    return segout, segstat, rowstat


@_timed("evt_soft_nbr_bwd")
def evt_soft_nbr_bwd(emb: torch.Tensor, idx: torch.Tensor, table: torch.Tensor, code_weights: torch.Tensor, seg: torch.Tensor,
                     seg_host: torch.Tensor, tau_ref: float, tau_learned: float, rowstat: torch.Tensor, segout: torch.Tensor, gup: torch.Tensor,
                     seg_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d emb [N, D] in emb's dtype for the outputs of evt_soft_nbr_fwd: the sum over segments of gup[s] * seg_weights[s] * d loss_s / d emb
    (gup, seg_weights: float32 [S] on the device; seg_weights None = ones).  Every row is written once."""
    n, d, k, s = _chk_evt_soft_nbr("evt_soft_nbr_bwd", emb, idx, table, code_weights, seg, seg_host, tau_ref, tau_learned)
    for t, shape, name in ((rowstat, (n, 10), "rowstat"), (segout, (s, 2), "segout"), (gup, (s,), "gup"), (seg_weights, (s,), "seg_weights")):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != emb.device):
            raise ValueError(f"evt_soft_nbr_bwd: {name} must be a contiguous float32 {shape} tensor on the device of emb")
    grad = torch.empty_like(emb)
    check(_lib.load().frl_evt_soft_nbr_bwd(_p(emb), _dt(emb), n, d, _p(idx), _p(table), _p(code_weights), k, _p(seg), _p(seg_host), s,
                                           1.0 / float(tau_ref), 1.0 / float(tau_learned), _p(rowstat), _p(segout), _p(gup), _p(seg_weights),
                                           _p(grad), _stream()), "frl_evt_soft_nbr_bwd")
    return grad


# ----------------------------------------------------------------------------------------------
# phase margin losses: recovery discrimination and spread ranking (csrc/phase_margin.hip)
# ----------------------------------------------------------------------------------------------
PHASE_MARGIN_MAX_T, PHASE_MARGIN_MAX_WIDTH = 32, 256


def _chk_recovery_disc(name: str, z: torch.Tensor, ysfc: torch.Tensor):
    """Shape limits first (they hold on any device), then the device, then the layouts -> (N, T, D)."""
    if z.dim() != 3 or ysfc.dim() != 2 or tuple(ysfc.shape) != tuple(z.shape[:2]):
        raise ValueError(f"{name}: expected z [N, T, D] and ysfc [N, T], got {tuple(z.shape)} and {tuple(ysfc.shape)}")
    n, t, d = z.shape
    if t > PHASE_MARGIN_MAX_T:
        raise ValueError(f"{name}: supports T <= {PHASE_MARGIN_MAX_T} timesteps, got T = {t}")
    if d > PHASE_MARGIN_MAX_WIDTH:
        raise ValueError(f"{name}: supports D <= {PHASE_MARGIN_MAX_WIDTH}, got D = {d}")
    if not (z.is_cuda and ysfc.is_cuda):
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    if n < 1 or t < 1 or d < 1:
        raise ValueError(f"{name}: needs at least one pixel, timestep and column")
    if z.dtype not in (torch.float32, torch.bfloat16) or not z.is_contiguous():
        raise ValueError(f"{name}: z must be a contiguous float32 or bfloat16 tensor")
    if ysfc.dtype != torch.float32 or not ysfc.is_contiguous() or ysfc.device != z.device:
        raise ValueError(f"{name}: ysfc must be a contiguous float32 [{n}, {t}] tensor on the device of z")
    return n, t, d


@_timed("recovery_disc_fwd")
def recovery_disc_fwd(z: torch.Tensor, ysfc: torch.Tensor, margin: float = 0.5, low_ysfc_max: float = 1.0, high_ysfc_min: float = 5.0):
    """z [N, T, D] float32 | bfloat16, ysfc [N, T] float32 (NaN / negative = invalid) -> (out2 f32 [2] = loss, n_pairs; stats f64 [4] =
    loss, n_pairs, active pixels, 0).  T <= 32, D <= 256."""
    n, t, d = _chk_recovery_disc("recovery_disc_fwd", z, ysfc)
    partial = torch.empty(n, 2, dtype=torch.float32, device=z.device)
    out2 = torch.empty(2, dtype=torch.float32, device=z.device)
    stats = torch.empty(4, dtype=torch.float64, device=z.device)
    check(_lib.load().frl_recovery_disc_fwd(_p(z), _dt(z), _p(ysfc), n, t, d, float(margin), float(low_ysfc_max), float(high_ysfc_min),
                                            _p(partial), _p(out2), _p(stats), _stream()), "frl_recovery_disc_fwd")
    return out2, stats


@_timed("recovery_disc_bwd")
def recovery_disc_bwd(z: torch.Tensor, ysfc: torch.Tensor, margin: float, low_ysfc_max: float, high_ysfc_min: float, out2: torch.Tensor,
                      g: torch.Tensor) -> torch.Tensor:
    """d z [N, T, D] in z's dtype for the outputs of recovery_disc_fwd, every row written; g: float32 [1] on the device."""
    n, t, d = _chk_recovery_disc("recovery_disc_bwd", z, ysfc)
    _chk_f32_on("recovery_disc_bwd", "z", z.device, (out2, (2,), "out2"), (g, (1,), "g"))
    grad = torch.empty_like(z)
    check(_lib.load().frl_recovery_disc_bwd(_p(z), _dt(z), _p(ysfc), n, t, d, float(margin), float(low_ysfc_max), float(high_ysfc_min),
                                            _p(out2), _p(g), _p(grad), _stream()), "frl_recovery_disc_bwd")
    return grad


def _chk_spread_ref_diff(name: str, ref_diff: torch.Tensor, b: int, device):
    if ref_diff.dtype != torch.float32 or tuple(ref_diff.shape) != (b,) or not ref_diff.is_contiguous() or ref_diff.device != device:
        raise ValueError(f"{name}: ref_diff must be a contiguous float32 [{b}] tensor on the device of the inputs")


def _chk_spread_rank(name: str, mask: torch.Tensor, ref_diff: torch.Tensor, blocks):
    if mask.dim() != 3 or mask.shape[1] != mask.shape[2] or any(x.shape != mask.shape for x in blocks):
        raise ValueError(f"{name}: expected distance blocks and mask of one shape [B, M, M], got {[tuple(x.shape) for x in blocks]} and "
                         f"{tuple(mask.shape)}")
    if tuple(ref_diff.shape) != (mask.shape[0],):
        raise ValueError(f"{name}: ref_diff must have shape [{mask.shape[0]}], got {tuple(ref_diff.shape)}")
    if not (mask.is_cuda and ref_diff.is_cuda and all(x.is_cuda for x in blocks)):
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    b, m, _ = mask.shape
    if b < 1 or m < 1:
        raise ValueError(f"{name}: needs at least one pair and position")
    if mask.dtype != torch.bool or not mask.is_contiguous():
        raise ValueError(f"{name}: mask must be a contiguous bool tensor")
    for x in blocks:
        if x.dtype != torch.float32 or not x.is_contiguous() or x.device != mask.device:
            raise ValueError(f"{name}: the distance blocks must be contiguous float32 tensors on the device of mask")
    _chk_spread_ref_diff(name, ref_diff, b, mask.device)
    return b, m


@_timed("spread_rank_fwd")
def spread_rank_fwd(d_i: torch.Tensor, d_j: torch.Tensor, mask: torch.Tensor, ref_diff: torch.Tensor, margin: float = 0.1,
                    delta: float = 0.5):
    """d_i, d_j [B, M, M] float32, mask [B, M, M] bool, ref_diff [B] float32 -> (out2 f32 [2] = loss, B; stats f64 [8] = loss, constrained i,
    constrained j, satisfied, sum spread_i, sum spread_j, sum |ref_diff|, B; pairstat f32 [B, 3] = spread_i, spread_j, n_b)."""
    b, m = _chk_spread_rank("spread_rank_fwd", mask, ref_diff, (d_i, d_j))
    pairstat, out2, stats = _pair_outputs(b, 3, mask.device)
    check(_lib.load().frl_spread_rank_fwd(_p(d_i), _p(d_j), _p(mask), _p(ref_diff), b, m, float(margin), float(delta), _p(pairstat), _p(out2),
                                          _p(stats), _stream()), "frl_spread_rank_fwd")
    return out2, stats, pairstat


@_timed("spread_rank_bwd")
def spread_rank_bwd(mask: torch.Tensor, pairstat: torch.Tensor, ref_diff: torch.Tensor, margin: float, delta: float, g: torch.Tensor):
    """(d loss / d d_i, d loss / d d_j) float32 [B, M, M] for the outputs of spread_rank_fwd; g: float32 [1] on the device."""
    b, m = _chk_spread_rank("spread_rank_bwd", mask, ref_diff, ())
    _chk_f32_on("spread_rank_bwd", "mask", mask.device, (pairstat, (b, 3), "pairstat"), (g, (1,), "g"))
    gi = torch.empty(b, m, m, dtype=torch.float32, device=mask.device)
    gj = torch.empty_like(gi)
    check(_lib.load().frl_spread_rank_bwd(_p(mask), _p(pairstat), _p(ref_diff), _p(g), b, m, float(margin), float(delta), _p(gi), _p(gj),
                                          _stream()), "frl_spread_rank_bwd")
    return gi, gj


def _chk_spread_rank_gathered(name: str, emb, rows, lengths, ref_diff, checked: bool):
    """Shape limits first, then the device, then the layouts -> (B, M, rows [2, B, M] inside [0, R))."""
    if emb.dim() != 2:
        raise ValueError(f"{name}: expected emb [R, D], got {tuple(emb.shape)}")
    if rows.dim() != 3 or rows.shape[0] != 2:
        raise ValueError(f"{name}: the row indices come stacked as [2, B, M] (role i, role j), got {tuple(rows.shape)}")
    _, b, m = rows.shape
    if m > PHASE_MARGIN_MAX_T:
        raise ValueError(f"{name}: the gathered form supports M <= {PHASE_MARGIN_MAX_T} positions per pair, got M = {m}")
    if emb.shape[1] > PHASE_MARGIN_MAX_WIDTH:
        raise ValueError(f"{name}: the gathered form supports D <= {PHASE_MARGIN_MAX_WIDTH}, got D = {emb.shape[1]}")
    if tuple(lengths.shape) != (b,) or tuple(ref_diff.shape) != (b,):
        raise ValueError(f"{name}: lengths and ref_diff must have shape [{b}], got {tuple(lengths.shape)} and {tuple(ref_diff.shape)}")
    if not (emb.is_cuda and rows.is_cuda and lengths.is_cuda and ref_diff.is_cuda):
        raise _lib.FrlHipError(f"{name}: tensors must live on the GPU (no CPU fallback)")
    if b < 1 or m < 1 or emb.shape[0] < 1 or emb.shape[1] < 1:
        raise ValueError(f"{name}: needs at least one pair, position, row and column")
    if emb.dtype not in (torch.float32, torch.bfloat16) or not emb.is_contiguous():
        raise ValueError(f"{name}: emb must be contiguous float32 or bfloat16 rows")
    if rows.dtype != torch.int64 or not rows.is_contiguous() or lengths.dtype != torch.int64 or not lengths.is_contiguous():
        raise ValueError(f"{name}: row indices [2, {b}, {m}] and lengths [{b}] must be contiguous int64")
    _chk_spread_ref_diff(name, ref_diff, b, emb.device)
    if not checked:
        rows = sanitize_indices(rows, emb.shape[0], name + ": row indices")
    return b, m, rows


@_timed("spread_rank_gathered_fwd")
def spread_rank_gathered_fwd(emb: torch.Tensor, rows: torch.Tensor, lengths: torch.Tensor, ref_diff: torch.Tensor, margin: float = 0.1,
                             delta: float = 0.5, checked: bool = False):
    """emb [R, D] float32 | bfloat16, rows [2, B, M] int64 (role i, role j), lengths [B] int64, ref_diff [B] float32 -> (out2, stats,
    pairstat as spread_rank_fwd, rows sanitised into [0, R)).  M <= 32, D <= 256."""
    b, m, rows = _chk_spread_rank_gathered("spread_rank_gathered_fwd", emb, rows, lengths, ref_diff, checked)
    pairstat, out2, stats = _pair_outputs(b, 3, emb.device)
    check(_lib.load().frl_spread_rank_gathered_fwd(_p(emb), emb.shape[1], _dt(emb), _p(rows[0]), _p(rows[1]), _p(lengths), _p(ref_diff), b, m,
                                                   float(margin), float(delta), _p(pairstat), _p(out2), _p(stats), _stream()),
          "frl_spread_rank_gathered_fwd")
    return out2, stats, pairstat, rows


@_timed("spread_rank_gathered_bwd")
def spread_rank_gathered_bwd(emb: torch.Tensor, rows: torch.Tensor, lengths: torch.Tensor, ref_diff: torch.Tensor, margin: float, delta: float,
                             pairstat: torch.Tensor, g: torch.Tensor, checked: bool = False) -> torch.Tensor:
    """Gradient rows float32 [2, B, M, D] (role i, then role j) for the outputs of spread_rank_gathered_fwd; fold them into d emb with
    segment_sum_rows.  g: float32 [1] on the device."""
    b, m, rows = _chk_spread_rank_gathered("spread_rank_gathered_bwd", emb, rows, lengths, ref_diff, checked)
    _chk_f32_on("spread_rank_gathered_bwd", "emb", emb.device, (pairstat, (b, 3), "pairstat"), (g, (1,), "g"))
    grows = torch.empty(2, b, m, emb.shape[1], dtype=torch.float32, device=emb.device)
    check(_lib.load().frl_spread_rank_gathered_bwd(_p(emb), emb.shape[1], _dt(emb), _p(rows[0]), _p(rows[1]), _p(lengths), _p(ref_diff), b, m,
                                                   float(margin), float(delta), _p(pairstat), _p(g), _p(grows), _stream()),
          "frl_spread_rank_gathered_bwd")
    return grows


# ----------------------------------------------------------------------------------------------
# diagonal-covariance Gaussian mixtures and the phase summary (csrc/gmm.hip)
# ----------------------------------------------------------------------------------------------
GMM_MAX_K, GMM_MAX_D, GMM_MAX_KD, GMM_MAX_WORKGROUPS = 128, 128, 8192, MAX_WORKGROUPS
GMM_M_EM, GMM_M_LLOYD, GMM_M_INIT = 0, 1, 2
PHASE_SUMMARY_MAX_T, PHASE_SUMMARY_MAX_D = 64, 64


def chk_gmm_dims(n: int, d: int, k: int, name: str = "gmm", need_rows: bool = True):
    """Every size limit of the frl_gmm_* calls (ValueError)."""
    if not 1 <= k <= GMM_MAX_K:
        raise ValueError(f"{name}: supports 1 <= K <= {GMM_MAX_K} components, got {k}")
    if not 1 <= d <= GMM_MAX_D:
        raise ValueError(f"{name}: supports 1 <= D <= {GMM_MAX_D} columns, got {d}")
    if k * d > GMM_MAX_KD:
        raise ValueError(f"{name}: supports K * D <= {GMM_MAX_KD}, got {k} * {d}")
    if n >= 2 ** 31:
        raise ValueError(f"{name}: supports N < 2^31 rows, got {n}")
    if n < (k if need_rows else 1):
        raise ValueError(f"{name}: needs N >= {'K' if need_rows else '1'} rows, got N = {n}, K = {k}")


def chk_gmm(x: torch.Tensor, k: int, sample_weight: Optional[torch.Tensor] = None, workgroups: int = 0, name: str = "gmm",
            need_rows: bool = True):
    """Every limit of frl_gmm_em_step / frl_gmm_score that needs no device (ValueError)."""
    if x.dim() != 2:
        raise ValueError(f"{name}: expected X [N, D], got {tuple(x.shape)}")
    chk_gmm_dims(x.shape[0], x.shape[1], int(k), name, need_rows)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: X must be a contiguous float32 tensor, got {x.dtype} stride {x.stride()}")
    if sample_weight is not None and (sample_weight.dtype != torch.float32 or sample_weight.shape != (x.shape[0],)
                                      or not sample_weight.is_contiguous()):
        raise ValueError(f"{name}: sample_weight must be a contiguous float32 [N] tensor, got {sample_weight.dtype} {tuple(sample_weight.shape)}")
    chk_workgroups(name, workgroups)


def _chk_gmm_params(name: str, device, k: int, d: int, **tensors):
    for what, (t, shape) in tensors.items():
        if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous float32 {shape} tensor, got {t.dtype} {tuple(t.shape)}")
        _chk_one_device(name, t)
        if t.device != device:
            raise ValueError(f"{name}: {what} must be on the device of X")


def gmm_workspace(n: int, d: int, k: int, device, workgroups: int = 0) -> torch.Tensor:
    """A workspace of one fit: it carries the partial sums from gmm_em_step to gmm_m_step, so it is not the shared scratch buffer."""
    chk_gmm_dims(n, d, k, "gmm_workspace", need_rows=False)
    return _owned_workspace("gmm_workspace", lambda lib: lib.frl_gmm_workspace_bytes(n, d, k, int(workgroups)), device)


@_timed("gmm_pivot")
def gmm_pivot(x: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """X [N, D] f32 -> its column means [D] f32 (summed in double in a fixed order)."""
    chk_gmm(x, 1, name="gmm_pivot", need_rows=False)
    _chk_one_device("gmm_pivot", x)
    pivot = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    check(_lib.load().frl_gmm_pivot(_p(x), x.shape[0], x.shape[1], _p(pivot), _p(ws), ws.numel(), _stream()), "frl_gmm_pivot")
    return pivot


@_timed("gmm_em_step")
def gmm_em_step(x: torch.Tensor, sample_weight: Optional[torch.Tensor], pivot: torch.Tensor, weights: torch.Tensor, means_c: torch.Tensor,
                variances: torch.Tensor, state: torch.Tensor, ws: torch.Tensor, hard: bool = False, workgroups: int = 0) -> None:
    """The E pass of one iteration (include/frl_hip.h: frl_gmm_em_step): the partial sums land in ws for gmm_m_step.  No host read."""
    k = weights.shape[0] if weights.dim() == 1 else -1
    chk_gmm(x, k, sample_weight, workgroups, "gmm_em_step")
    _chk_one_device("gmm_em_step", x)
    d = x.shape[1]
    _chk_gmm_params("gmm_em_step", x.device, k, d, pivot=(pivot, (d,)), weights=(weights, (k,)), means_c=(means_c, (k, d)),
                    variances=(variances, (k, d)))
    if state.dtype != torch.int32 or state.numel() != 2 or state.device != x.device:
        raise ValueError("gmm_em_step: state must be an int32 [2] tensor on the device of X")
    check(_lib.load().frl_gmm_em_step(_p(x), _p(sample_weight), x.shape[0], d, k, _p(pivot), _p(weights), _p(means_c), _p(variances),
                                      1 if hard else 0, int(workgroups), _p(state), _p(ws), ws.numel(), _stream()), "frl_gmm_em_step")


@_timed("gmm_m_step")
def gmm_m_step(n: int, pivot: torch.Tensor, weights: torch.Tensor, means: torch.Tensor, means_c: torch.Tensor, variances: torch.Tensor,
               state: torch.Tensor, ws: torch.Tensor, history: Optional[torch.Tensor] = None, reg_covar: float = 1e-6, tol: float = 1e-3,
               mode: int = GMM_M_EM, workgroups: int = 0) -> None:
    """The M pass (include/frl_hip.h: frl_gmm_m_step): parameters in place; mode GMM_M_EM also appends the lower bound to `history`
    (float64 [max_iter]) and keeps the iteration count and the convergence flag in `state`.  No host read."""
    k, d = means.shape
    chk_gmm_dims(int(n), d, k, "gmm_m_step")
    chk_workgroups("gmm_m_step", workgroups, hint="")
    _chk_gmm_params("gmm_m_step", means.device, k, d, pivot=(pivot, (d,)), weights=(weights, (k,)), means=(means, (k, d)),
                    means_c=(means_c, (k, d)), variances=(variances, (k, d)))
    max_iter = 0
    if mode == GMM_M_EM:
        if history is None or history.dtype != torch.float64 or history.dim() != 1 or history.device != means.device or history.numel() < 1:
            raise ValueError("gmm_m_step: the EM mode needs a float64 [max_iter] history on the device of the parameters")
        max_iter = history.numel()
    check(_lib.load().frl_gmm_m_step(int(n), d, k, _p(pivot), _p(weights), _p(means), _p(means_c), _p(variances), float(reg_covar), float(tol),
                                     int(mode), _p(history), max_iter, _p(state), int(workgroups), _p(ws), ws.numel(), _stream()),
          "frl_gmm_m_step")


@_timed("gmm_score")
def gmm_score(x: torch.Tensor, pivot: torch.Tensor, weights: torch.Tensor, means_c: torch.Tensor, variances: torch.Tensor,
              want_resp: bool = False):
    """-> (lse f32 [N], labels int32 [N], resp f32 [N, K] | None) of X under the mixture (include/frl_hip.h: frl_gmm_score)."""
    k = weights.shape[0] if weights.dim() == 1 else -1
    chk_gmm(x, k, name="gmm_score", need_rows=False)
    _chk_one_device("gmm_score", x)
    n, d = x.shape
    _chk_gmm_params("gmm_score", x.device, k, d, pivot=(pivot, (d,)), weights=(weights, (k,)), means_c=(means_c, (k, d)),
                    variances=(variances, (k, d)))
    lse = torch.empty(n, dtype=torch.float32, device=x.device)
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    resp = torch.empty(n, k, dtype=torch.float32, device=x.device) if want_resp else None
    check(_lib.load().frl_gmm_score(_p(x), n, d, k, _p(pivot), _p(weights), _p(means_c), _p(variances), _p(lse), _p(labels), _p(resp), _stream()),
          "frl_gmm_score")
    return lse, labels, resp


def chk_phase_summary(z_phase: torch.Tensor, ysfc: torch.Tensor):
    """Every limit of frl_phase_summary that needs no device (ValueError)."""
    if z_phase.dim() != 3 or ysfc.dim() != 2 or tuple(ysfc.shape) != tuple(z_phase.shape[:2]) or z_phase.shape[0] < 1:
        raise ValueError(f"phase_summary: expected z_phase [N, T, D] and ysfc [N, T] with N >= 1, got {tuple(z_phase.shape)} and {tuple(ysfc.shape)}")
    if not 1 <= z_phase.shape[1] <= PHASE_SUMMARY_MAX_T:
        raise ValueError(f"phase_summary: supports 1 <= T <= {PHASE_SUMMARY_MAX_T} timesteps, got {z_phase.shape[1]}")
    if not 1 <= z_phase.shape[2] <= PHASE_SUMMARY_MAX_D:
        raise ValueError(f"phase_summary: supports 1 <= D <= {PHASE_SUMMARY_MAX_D} channels, got {z_phase.shape[2]}")
    if z_phase.shape[0] >= 2 ** 31:
        raise ValueError("phase_summary: supports N < 2^31 rows")
    for t, what in ((z_phase, "z_phase"), (ysfc, "ysfc")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"phase_summary: {what} must be a contiguous float32 tensor, got {t.dtype} stride {t.stride()}")


@_timed("phase_summary")
def phase_summary(z_phase: torch.Tensor, ysfc: torch.Tensor, low_max: float = 1.0, high_min: float = 5.0):
    """z_phase [N, T, D], ysfc [N, T] (NaN: unobserved) -> (summary [N, 3 D], temporal_var [N]); include/frl_hip.h: frl_phase_summary."""
    chk_phase_summary(z_phase, ysfc)
    if not z_phase.is_cuda or not ysfc.is_cuda:
        raise _lib.FrlHipError("phase_summary: tensors must live on the GPU (no CPU fallback)")
    if z_phase.device != ysfc.device:
        raise ValueError("phase_summary: z_phase and ysfc must be on one device")
    n, t, d = z_phase.shape
    summary = torch.empty(n, 3 * d, dtype=torch.float32, device=z_phase.device)
    tvar = torch.empty(n, dtype=torch.float32, device=z_phase.device)
    check(_lib.load().frl_phase_summary(_p(z_phase), _p(ysfc), n, t, d, float(low_max), float(high_min), _p(summary), _p(tvar), _stream()),
          "frl_phase_summary")
    return summary, tvar


# ----------------------------------------------------------------------------------------------
# closed-form linear probes (csrc/probe.hip)
# ----------------------------------------------------------------------------------------------
PROBE_MAX_D, PROBE_MAX_CY, PROBE_MAX_WORKGROUPS = 128, 16, MAX_WORKGROUPS


def chk_probe_dims(d: int, cy: int, workgroups: int = 0, name: str = "probe"):
    """The size limits of the frl_probe_* calls that need no data (ValueError)."""
    if not 1 <= int(d) <= PROBE_MAX_D:
        raise ValueError(f"{name}: supports 1 <= D <= {PROBE_MAX_D} feature columns, got {d}")
    if not 1 <= int(cy) <= PROBE_MAX_CY:
        raise ValueError(f"{name}: supports 1 <= Cy <= {PROBE_MAX_CY} targets, got {cy}")
    chk_workgroups(name, workgroups)


def chk_probe(a: torch.Tensor, bs: Optional[torch.Tensor], y: torch.Tensor, mask: torch.Tensor, workgroups: int = 0, name: str = "probe"):
    """Every limit of the frl_probe_* calls that needs no device (ValueError) -> (B, T, P, Da, Db, Cy)."""
    for what, t in (("A", a), ("B", bs), ("Y", y)):
        if t is None:
            continue
        if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: {what} must be a contiguous float32 [B, T_s, P, C] tensor, got {t.dtype} {tuple(t.shape)} stride {t.stride()}")
    if mask.dim() != 2 or mask.dtype != torch.uint8 or not mask.is_contiguous():
        raise ValueError(f"{name}: mask must be a contiguous uint8 [B, P] tensor, got {mask.dtype} {tuple(mask.shape)}")
    b, p = mask.shape
    t = max(s.shape[1] for s in (a, bs, y) if s is not None)
    for what, s in (("A", a), ("B", bs), ("Y", y)):
        if s is not None and (s.shape[0] != b or s.shape[2] != p or s.shape[1] not in (1, t)):
            raise ValueError(f"{name}: {what} {tuple(s.shape)} does not match B = {b}, T in (1, {t}), P = {p}")
    da, db, cy = a.shape[3], 0 if bs is None else bs.shape[3], y.shape[3]
    chk_probe_dims(da + db, cy, workgroups, name)
    if b < 1 or p < 1 or t < 1 or da < 1 or (bs is not None and db < 1):
        raise ValueError(f"{name}: empty input, B = {b}, T = {t}, P = {p}, Da = {da}")
    if b * t * p >= 2 ** 31:
        raise ValueError(f"{name}: supports B * T * P < 2^31 observations, got {b * t * p}")
    _chk_one_device(name, a, bs, y, mask)
    return b, t, p, da, db, cy


def probe_workspace(d: int, cy: int, device, workgroups: int = 0) -> torch.Tensor:
    """A workspace for the frl_probe_* calls of one probe (slabs of partial sums between a pass and its reduction)."""
    chk_probe_dims(d, cy, workgroups, "probe_workspace")
    return _owned_workspace("probe_workspace", lambda lib: lib.frl_probe_workspace_bytes(int(d), int(cy), int(workgroups)), device)


def _probe_args(a, bs, y, mask, dims):
    b, t, p, da, db, cy = dims
    return (_p(a), a.shape[1], da, _p(bs), 1 if bs is None else bs.shape[1], db, _p(y), y.shape[1], cy, _p(mask), b, t, p)


@_timed("probe_pivot")
def probe_pivot(a: torch.Tensor, bs: Optional[torch.Tensor], y: torch.Tensor, mask: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """-> pivot f32 [D + Cy]: the masked column means of [x | y] (include/frl_hip.h: frl_probe_pivot)."""
    dims = chk_probe(a, bs, y, mask, 0, "probe_pivot")
    pivot = torch.empty(dims[3] + dims[4] + dims[5], dtype=torch.float32, device=a.device)
    check(_lib.load().frl_probe_pivot(*_probe_args(a, bs, y, mask, dims), _p(pivot), _p(ws), ws.numel(), _stream()), "frl_probe_pivot")
    return pivot


@_timed("probe_accumulate")
def probe_accumulate(a: torch.Tensor, bs: Optional[torch.Tensor], y: torch.Tensor, mask: torch.Tensor, pivot: torch.Tensor, s: torch.Tensor,
                     n: torch.Tensor, ws: torch.Tensor, workgroups: int = 0) -> None:
    """S f64 [C+1, C+1] += v^T v, n int64 [1] += the unmasked count (include/frl_hip.h: frl_probe_accumulate).  No host read."""
    dims = chk_probe(a, bs, y, mask, workgroups, "probe_accumulate")
    c = dims[3] + dims[4] + dims[5]
    _chk_tensor_on("probe_accumulate", "pivot", pivot, (c,), torch.float32, a.device)
    _chk_tensor_on("probe_accumulate", "S", s, (c + 1, c + 1), torch.float64, a.device)
    _chk_tensor_on("probe_accumulate", "n", n, (1,), torch.int64, a.device)
    check(_lib.load().frl_probe_accumulate(*_probe_args(a, bs, y, mask, dims), _p(pivot), int(workgroups), _p(s), _p(n), _p(ws), ws.numel(),
                                           _stream()), "frl_probe_accumulate")


@_timed("probe_evaluate")
def probe_evaluate(a: torch.Tensor, bs: Optional[torch.Tensor], y: torch.Tensor, mask: torch.Tensor, pivot: torch.Tensor, wc: torch.Tensor,
                   bc: torch.Tensor, e: torch.Tensor, n: torch.Tensor, ws: torch.Tensor, want_pred: bool = False, workgroups: int = 0):
    """E f64 [Cy, 3] += (SSE, sum (y - q), sum (y - q)^2), n int64 [1] += the unmasked count; -> pred f32 [B, T, P, Cy] | None
    (include/frl_hip.h: frl_probe_evaluate).  No host read."""
    dims = chk_probe(a, bs, y, mask, workgroups, "probe_evaluate")
    b, t, p, da, db, cy = dims
    _chk_tensor_on("probe_evaluate", "pivot", pivot, (da + db + cy,), torch.float32, a.device)
    _chk_tensor_on("probe_evaluate", "Wc", wc, (da + db, cy), torch.float32, a.device)
    _chk_tensor_on("probe_evaluate", "bc", bc, (cy,), torch.float32, a.device)
    _chk_tensor_on("probe_evaluate", "E", e, (cy, 3), torch.float64, a.device)
    _chk_tensor_on("probe_evaluate", "n", n, (1,), torch.int64, a.device)
    pred = torch.empty(b, t, p, cy, dtype=torch.float32, device=a.device) if want_pred else None
    check(_lib.load().frl_probe_evaluate(*_probe_args(a, bs, y, mask, dims), _p(pivot), _p(wc), _p(bc), int(workgroups), _p(e), _p(n), _p(pred),
                                         _p(ws), ws.numel(), _stream()), "frl_probe_evaluate")
    return pred


# the "full" design [z_type | z_phase | z_type (x) z_phase] (csrc/probe_full.hip)
PROBE_FULL_MAX_DT, PROBE_FULL_MAX_DP, PROBE_FULL_MAX_DQ = 64, 16, 768


def chk_probe_full_dims(dt: int, dp: int, cy: int, workgroups: int = 0, name: str = "probe_full"):
    """The size limits of the frl_probe_full_* calls that need no data (ValueError)."""
    if not 1 <= int(dt) <= PROBE_FULL_MAX_DT:
        raise ValueError(f"{name}: supports 1 <= Dt <= {PROBE_FULL_MAX_DT} z_type columns, got {dt}")
    if not 1 <= int(dp) <= PROBE_FULL_MAX_DP:
        raise ValueError(f"{name}: supports 1 <= Dp <= {PROBE_FULL_MAX_DP} z_phase columns, got {dp}")
    if int(dt) * int(dp) > PROBE_FULL_MAX_DQ:
        raise ValueError(f"{name}: supports Dt * Dp <= {PROBE_FULL_MAX_DQ} interaction columns, got {int(dt) * int(dp)}")
    chk_probe_dims(int(dt) + int(dp), cy, workgroups, name)


def chk_probe_full(a: torch.Tensor, bs: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, workgroups: int = 0, name: str = "probe_full"):
    """Every limit of the frl_probe_full_* calls that needs no device (ValueError) -> (B, T, P, Dt, Dp, Cy)."""
    if bs is None:
        raise ValueError(f"{name}: needs both sources, z_type and z_phase")
    if all(isinstance(s, torch.Tensor) and s.dim() == 4 for s in (a, bs, y)):    # the widths first: chk_probe ends on the device check
        chk_probe_full_dims(a.shape[3], bs.shape[3], y.shape[3], workgroups, name)
    return chk_probe(a, bs, y, mask, workgroups, name)


def probe_full_workspace(dt: int, dp: int, cy: int, device, workgroups: int = 0) -> torch.Tensor:
    """A workspace for the frl_probe_full_* calls of one probe; it serves the frl_probe_* calls of the same widths too."""
    chk_probe_full_dims(dt, dp, cy, workgroups, "probe_full_workspace")
    return _owned_workspace("probe_full_workspace", lambda lib: max(lib.frl_probe_full_workspace_bytes(int(dt), int(dp), int(cy), int(workgroups)),
                                                                    lib.frl_probe_workspace_bytes(int(dt) + int(dp), int(cy), int(workgroups))), device)


@_timed("probe_full_accumulate")
def probe_full_accumulate(a: torch.Tensor, bs: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, pivot: torch.Tensor, scq: torch.Tensor,
                          sqq: torch.Tensor, ws: torch.Tensor, workgroups: int = 0) -> None:
    """Scq f64 [C+1, Dq] += c^T q', Sqq f64 [Dq, Dq] += q'^T q' (include/frl_hip.h: frl_probe_full_accumulate).  No host read."""
    dims = chk_probe_full(a, bs, y, mask, workgroups, "probe_full_accumulate")
    c, dq = dims[3] + dims[4] + dims[5], dims[3] * dims[4]
    _chk_tensor_on("probe_full_accumulate", "pivot", pivot, (c,), torch.float32, a.device)
    _chk_tensor_on("probe_full_accumulate", "Scq", scq, (c + 1, dq), torch.float64, a.device)
    _chk_tensor_on("probe_full_accumulate", "Sqq", sqq, (dq, dq), torch.float64, a.device)
    check(_lib.load().frl_probe_full_accumulate(*_probe_args(a, bs, y, mask, dims), _p(pivot), int(workgroups), _p(scq), _p(sqq), _p(ws), ws.numel(),
                                                _stream()), "frl_probe_full_accumulate")


@_timed("probe_full_evaluate")
def probe_full_evaluate(a: torch.Tensor, bs: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, pivot: torch.Tensor, beta: torch.Tensor,
                        u: torch.Tensor, v: torch.Tensor, omega: torch.Tensor, e: torch.Tensor, n: torch.Tensor, ws: torch.Tensor,
                        want_pred: bool = False, workgroups: int = 0):
    """E f64 [Cy, 3] += (SSE, sum (y - q), sum (y - q)^2), n int64 [1] += the unmasked count for pred = beta + x' u + p' v + x'^T Omega p';
    -> pred f32 [B, T, P, Cy] | None (include/frl_hip.h: frl_probe_full_evaluate).  No host read."""
    dims = chk_probe_full(a, bs, y, mask, workgroups, "probe_full_evaluate")
    b, t, p, dt, dp, cy = dims
    _chk_tensor_on("probe_full_evaluate", "pivot", pivot, (dt + dp + cy,), torch.float32, a.device)
    _chk_tensor_on("probe_full_evaluate", "beta", beta, (cy,), torch.float32, a.device)
    _chk_tensor_on("probe_full_evaluate", "u", u, (cy, dt), torch.float32, a.device)
    _chk_tensor_on("probe_full_evaluate", "v", v, (cy, dp), torch.float32, a.device)
    _chk_tensor_on("probe_full_evaluate", "omega", omega, (cy, dt, dp), torch.float32, a.device)
    _chk_tensor_on("probe_full_evaluate", "E", e, (cy, 3), torch.float64, a.device)
    _chk_tensor_on("probe_full_evaluate", "n", n, (1,), torch.int64, a.device)
    pred = torch.empty(b, t, p, cy, dtype=torch.float32, device=a.device) if want_pred else None
    check(_lib.load().frl_probe_full_evaluate(*_probe_args(a, bs, y, mask, dims), _p(pivot), _p(beta), _p(u), _p(v), _p(omega), int(workgroups),
                                              _p(e), _p(n), _p(pred), _p(ws), ws.numel(), _stream()), "frl_probe_full_evaluate")
    return pred


# ----------------------------------------------------------------------------------------------
# EVT-stratified diagnostics (csrc/strata.hip)
# ----------------------------------------------------------------------------------------------
STRATA_MAX_G, STRATA_MAX_R, STRATA_MAX_CELLS = 4095, 4096, 1 << 24
STRATA_MAX_GC, STRATA_MAX_D, STRATA_MAX_GD, STRATA_MAX_WORKGROUPS = 128, 128, 8192, MAX_WORKGROUPS


def chk_strata_table_dims(r: int, g: int, workgroups: int = 0, name: str = "strata_contingency"):
    """The size limits of frl_strata_contingency that need no data (ValueError)."""
    if not 1 <= int(g) <= STRATA_MAX_G:
        raise ValueError(f"{name}: supports 1 <= G <= {STRATA_MAX_G} codes in the vocabulary, got {g}")
    if not 1 <= int(r) <= STRATA_MAX_R:
        raise ValueError(f"{name}: supports 1 <= R <= {STRATA_MAX_R} row labels, got {r}")
    if int(r) * int(g) > STRATA_MAX_CELLS:
        raise ValueError(f"{name}: supports R * G <= 2^24 cells, got {r} * {g}")
    chk_workgroups(name, workgroups)


def chk_strata_moment_dims(gc: int, d: int, workgroups: int = 0, name: str = "strata_moments"):
    """The size limits of frl_strata_moments that need no data (ValueError)."""
    if not 1 <= int(d) <= STRATA_MAX_D:
        raise ValueError(f"{name}: supports 1 <= D <= {STRATA_MAX_D} columns, got {d}")
    if not 1 <= int(gc) <= STRATA_MAX_GC:
        raise ValueError(f"{name}: supports a window of 1 <= Gc <= {STRATA_MAX_GC} groups, got {gc}")
    if int(gc) * int(d) > STRATA_MAX_GD:
        raise ValueError(f"{name}: supports Gc * D <= {STRATA_MAX_GD}, got {gc} * {d}")
    chk_workgroups(name, workgroups)


def _chk_strata_keys(name: str, codes: torch.Tensor, mask: Optional[torch.Tensor], vocab: torch.Tensor, b: int, t: int, p: int):
    if codes.dtype not in (torch.int32, torch.float32) or tuple(codes.shape) != (b, p) or not codes.is_contiguous():
        raise ValueError(f"{name}: codes must be a contiguous int32 or float32 [B, P] = [{b}, {p}] tensor, got {codes.dtype} {tuple(codes.shape)}")
    if vocab.dtype != torch.int32 or vocab.dim() != 1 or not vocab.is_contiguous():
        raise ValueError(f"{name}: vocab must be a contiguous int32 [G] tensor, got {vocab.dtype} {tuple(vocab.shape)}")
    if not 1 <= vocab.numel() <= STRATA_MAX_G:
        raise ValueError(f"{name}: supports 1 <= G <= {STRATA_MAX_G} codes in the vocabulary, got {vocab.numel()}")
    if mask is not None and (mask.dtype != torch.uint8 or mask.dim() != 3 or mask.shape[0] != b or mask.shape[2] != p or mask.shape[1] not in (1, t)
                             or not mask.is_contiguous()):
        raise ValueError(f"{name}: mask must be a contiguous uint8 [B, Tm, P] = [{b}, 1 or {t}, {p}] tensor, got {mask.dtype} {tuple(mask.shape)}")
    if b < 1 or t < 1 or p < 1:
        raise ValueError(f"{name}: empty input, B = {b}, T = {t}, P = {p}")
    if b * t * p >= 2 ** 31:
        raise ValueError(f"{name}: supports B * T * P < 2^31 observations, got {b * t * p}")


def strata_workspace(gc: int, d: int, temporal: bool, device, workgroups: int = 0) -> torch.Tensor:
    """A workspace for frl_strata_moments (the slabs of partial sums between the pass and its reduction)."""
    chk_strata_moment_dims(gc, d, workgroups, "strata_workspace")
    return _owned_workspace("strata_workspace", lambda lib: lib.frl_strata_workspace_bytes(int(gc), int(d), int(bool(temporal)), int(workgroups)), device)


@_timed("strata_contingency")
def strata_contingency(rows: torch.Tensor, codes: torch.Tensor, mask: Optional[torch.Tensor], vocab: torch.Tensor, table: torch.Tensor,
                       unmatched: torch.Tensor, rejected: torch.Tensor, workgroups: int = 0) -> None:
    """table int64 [R, G] += the counts of (rows [B, Tr, P] int32, column of codes [B, P]) over the unmasked observations; unmatched and
    rejected int64 [1] += the skipped ones (include/frl_hip.h: frl_strata_contingency).  No host read."""
    name = "strata_contingency"
    if rows.dim() != 3 or rows.dtype != torch.int32 or not rows.is_contiguous():
        raise ValueError(f"{name}: rows must be a contiguous int32 [B, Tr, P] tensor, got {rows.dtype} {tuple(rows.shape)}")
    b, tr, p = rows.shape
    t = max(tr, 1 if mask is None or mask.dim() != 3 else mask.shape[1])
    if tr not in (1, t):
        raise ValueError(f"{name}: rows {tuple(rows.shape)} and mask {tuple(mask.shape)} differ in T")
    _chk_strata_keys(name, codes, mask, vocab, b, t, p)
    if table.dim() != 2 or table.shape[1] != vocab.numel():
        raise ValueError(f"{name}: table must be [R, G] = [R, {vocab.numel()}], got {tuple(table.shape)}")
    r, g = table.shape
    chk_strata_table_dims(r, g, workgroups, name)
    _chk_one_device(name, rows, codes, mask, vocab, table, unmatched, rejected)
    _chk_tensor_on(name, "table", table, (r, g), torch.int64, rows.device)
    _chk_tensor_on(name, "unmatched", unmatched, (1,), torch.int64, rows.device)
    _chk_tensor_on(name, "rejected", rejected, (1,), torch.int64, rows.device)
    check(_lib.load().frl_strata_contingency(_p(rows), tr, _p(codes), int(codes.dtype == torch.float32), _p(mask), 1 if mask is None else mask.shape[1],
                                             _p(vocab), g, b, t, p, r, int(workgroups), _p(table), _p(unmatched), _p(rejected), _stream()),
          "frl_strata_contingency")


@_timed("strata_moments")
def strata_moments(x: torch.Tensor, codes: torch.Tensor, mask: Optional[torch.Tensor], vocab: torch.Tensor, g0: int, gc: int, pivot: torch.Tensor,
                   count: torch.Tensor, s1: torch.Tensor, s2: torch.Tensor, sw: Optional[torch.Tensor], unmatched: Optional[torch.Tensor],
                   ws: torch.Tensor, temporal: bool = False, workgroups: int = 0) -> None:
    """count int64 [G], S1, S2 (and SW, temporal) float64 [G, D] += the moments of x [B, T, P, D] - pivot over the groups [g0, g0 + gc) of
    the vocabulary (include/frl_hip.h: frl_strata_moments).  No host read."""
    name = "strata_moments"
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be a contiguous float32 [B, T, P, D] tensor, got {x.dtype} {tuple(x.shape)}")
    b, t, p, d = x.shape
    chk_strata_moment_dims(gc, d, workgroups, name)
    _chk_strata_keys(name, codes, mask, vocab, b, t, p)
    g = vocab.numel()
    if not 0 <= int(g0) <= g - int(gc):
        raise ValueError(f"{name}: the window [{g0}, {g0} + {gc}) must lie in the vocabulary of {g} codes")
    if temporal and mask is not None and mask.shape[1] != 1:
        raise ValueError(f"{name}: the temporal mode takes a per-pixel mask [B, 1, P], got {tuple(mask.shape)}")
    if temporal and sw is None:
        raise ValueError(f"{name}: the temporal mode needs SW")
    _chk_one_device(name, x, codes, mask, vocab, pivot, count, s1, s2, sw, unmatched, ws)
    _chk_tensor_on(name, "pivot", pivot, (d,), torch.float32, x.device)
    _chk_tensor_on(name, "count", count, (g,), torch.int64, x.device)
    for what, s in (("S1", s1), ("S2", s2), ("SW", sw)):
        if s is not None:
            _chk_tensor_on(name, what, s, (g, d), torch.float64, x.device)
    if unmatched is not None:
        _chk_tensor_on(name, "unmatched", unmatched, (1,), torch.int64, x.device)
    check(_lib.load().frl_strata_moments(_p(x), _p(codes), int(codes.dtype == torch.float32), _p(mask), 1 if mask is None else mask.shape[1], _p(vocab),
                                         g, int(g0), int(gc), b, t, p, d, _p(pivot), int(bool(temporal)), int(workgroups), _p(count), _p(s1), _p(s2),
                                         _p(sw), _p(unmatched), _p(ws), ws.numel(), _stream()), "frl_strata_moments")


# ----------------------------------------------------------------------------------------------
# exact grouped quantiles (csrc/quantile.hip)
# ----------------------------------------------------------------------------------------------
QUANT_MAX_D, QUANT_MAX_Q, QUANT_MAX_C, QUANT_MAX_SLOTS = 16, 8, 65535, 1 << 23


def chk_quantile_dims(c: int, d: int, q: int = 1, workgroups: int = 0, name: str = "quantile_select"):
    """The size limits of frl_quantile_append and frl_quantile_select that need no data (ValueError)."""
    if not 1 <= int(d) <= QUANT_MAX_D:
        raise ValueError(f"{name}: supports 1 <= D <= {QUANT_MAX_D} columns, got {d}")
    if not 1 <= int(q) <= QUANT_MAX_Q:
        raise ValueError(f"{name}: supports 1 <= Q <= {QUANT_MAX_Q} probabilities, got {q}")
    if not 1 <= int(c) <= QUANT_MAX_C:
        raise ValueError(f"{name}: supports 1 <= C <= {QUANT_MAX_C} cells, got {c}")
    if int(c) * int(d) * 2 * int(q) > QUANT_MAX_SLOTS:
        raise ValueError(f"{name}: supports C * D * 2Q <= 2^23, got {c} * {d} * {2 * int(q)}")
    chk_workgroups(name, workgroups)


def chk_quantile_probs(q, name: str = "quantile_select"):
    """-> the probabilities as a list of floats: 1 <= Q <= 8 of them, each in [0, 1] (ValueError)."""
    probs = [float(v) for v in (q if hasattr(q, "__iter__") else [q])]
    if not 1 <= len(probs) <= QUANT_MAX_Q:
        raise ValueError(f"{name}: supports 1 <= Q <= {QUANT_MAX_Q} probabilities, got {len(probs)}")
    if any(not 0.0 <= v <= 1.0 for v in probs):
        raise ValueError(f"{name}: probabilities must lie in [0, 1], got {probs}")
    return probs


@_timed("quantile_append")
def quantile_append(x: torch.Tensor, codes: torch.Tensor, rows: Optional[torch.Tensor], mask: Optional[torch.Tensor], vocab: torch.Tensor, r: int,
                    cells: torch.Tensor, keys: torch.Tensor, state: torch.Tensor, workgroups: int = 0) -> None:
    """Appends one record (cell, D keys) per surviving observation of x [B, T, P, D] to cells int32 [capacity], keys int32 [D, capacity];
    state int64 [5] = (cursor, unmatched, rejected, nonfinite, dropped) (include/frl_hip.h: frl_quantile_append).  No host read."""
    name = "quantile_append"
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{name}: x must be a contiguous float32 [B, T, P, D] tensor, got {x.dtype} {tuple(x.shape)}")
    b, t, p, d = x.shape
    _chk_strata_keys(name, codes, mask, vocab, b, t, p)
    g = vocab.numel()
    chk_quantile_dims(int(r) * g, d, 1, workgroups, name)
    if rows is None:
        if int(r) != 1:
            raise ValueError(f"{name}: R must be 1 without rows, got {r}")
    elif rows.dtype != torch.int32 or rows.dim() != 3 or rows.shape[0] != b or rows.shape[2] != p or rows.shape[1] not in (1, t) or not rows.is_contiguous():
        raise ValueError(f"{name}: rows must be a contiguous int32 [B, Tr, P] = [{b}, 1 or {t}, {p}] tensor, got {rows.dtype} {tuple(rows.shape)}")
    if cells.dim() != 1 or not 1 <= cells.numel() < 2 ** 31:
        raise ValueError(f"{name}: cells must be [capacity] with 1 <= capacity < 2^31, got {tuple(cells.shape)}")
    cap = cells.numel()
    _chk_one_device(name, x, codes, rows, mask, vocab, cells, keys, state)
    _chk_tensor_on(name, "cells", cells, (cap,), torch.int32, x.device)
    _chk_tensor_on(name, "keys", keys, (d, cap), torch.int32, x.device)
    _chk_tensor_on(name, "state", state, (5,), torch.int64, x.device)
    sp = state.data_ptr()
    check(_lib.load().frl_quantile_append(_p(x), _p(codes), int(codes.dtype == torch.float32), _p(rows), 1 if rows is None else rows.shape[1], _p(mask),
                                          1 if mask is None else mask.shape[1], _p(vocab), g, b, t, p, d, int(r), int(workgroups), _p(cells), _p(keys),
                                          cap, *[ctypes.c_void_p(sp + 8 * i) for i in range(5)], _stream()), "frl_quantile_append")


@_timed("quantile_select")
def quantile_select(probs, c: int, d: int, cells: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None,
                    cursor: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, workgroups: int = 0):
    """The bracketing order statistics of every (cell, column) at every probability, either of the records (cells, keys, cursor) or of the
    rows of x [N, D] (mask uint8 [N] optional; one cell) -> (count int64 [C], lo f32 [C, D, Q], hi f32 [C, D, Q], frac f64 [C, Q]) on the
    device (include/frl_hip.h: frl_quantile_select).  No host read."""
    name = "quantile_select"
    probs = chk_quantile_probs(probs, name)
    nq = len(probs)
    chk_quantile_dims(c, d, nq, workgroups, name)
    if x is not None:
        if x.dim() != 2 or x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] != d or not 1 <= x.shape[0] < 2 ** 31:
            raise ValueError(f"{name}: x must be a contiguous float32 [N, {d}] tensor with 1 <= N < 2^31, got {x.dtype} {tuple(x.shape)}")
        if int(c) != 1 or cells is not None or keys is not None or cursor is not None:
            raise ValueError(f"{name}: x goes into a single cell and excludes records")
        if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (x.shape[0],) or not mask.is_contiguous()):
            raise ValueError(f"{name}: mask must be a contiguous uint8 [{x.shape[0]}] tensor, got {mask.dtype} {tuple(mask.shape)}")
        first, cap, n = x, 0, x.shape[0]
        _chk_one_device(name, x, mask)
    else:
        if cells is None or keys is None or cursor is None or mask is not None:
            raise ValueError(f"{name}: needs x, or cells, keys and cursor without a mask")
        first, cap, n = cells, cells.numel(), 0
        _chk_one_device(name, cells, keys, cursor)
        _chk_tensor_on(name, "cells", cells, (cap,), torch.int32, cells.device)
        _chk_tensor_on(name, "keys", keys, (d, cap), torch.int32, cells.device)
        if cursor.dtype != torch.int64 or cursor.numel() < 1 or not cursor.is_contiguous():
            raise ValueError(f"{name}: cursor must be a contiguous int64 tensor")
        if not 1 <= cap < 2 ** 31:
            raise ValueError(f"{name}: supports 1 <= capacity < 2^31, got {cap}")
    dev = first.device
    lib = _lib.load()
    ws = torch.empty(max(lib.frl_quantile_workspace_bytes(int(c), int(d), nq), 256), dtype=torch.uint8, device=dev)
    count = torch.empty(int(c), dtype=torch.int64, device=dev)
    lo = torch.empty(int(c), int(d), nq, dtype=torch.float32, device=dev)
    hi = torch.empty_like(lo)
    frac = torch.empty(int(c), nq, dtype=torch.float64, device=dev)
    pr = (ctypes.c_double * nq)(*probs)
    check(lib.frl_quantile_select(_p(cells), _p(keys), cap, _p(cursor), _p(x), _p(mask), n, int(c), int(d), ctypes.cast(pr, ctypes.c_void_p), nq,
                                  int(workgroups), _p(count), _p(lo), _p(hi), _p(frac), _p(ws), ws.numel(), _stream()), "frl_quantile_select")
    return count, lo, hi, frac
