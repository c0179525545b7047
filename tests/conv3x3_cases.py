"""Shared cases for the 3x3 convolution kernels (csrc/conv3x3.hip, csrc/conv3x3_wgrad.hip): a pure-Python mirror of the host dispatch
(which tile, grid, staging route, channel chunks, output block groups and store route a shape takes), a covering table of shapes, and
the CPU references both tests/test_cpu_conv3x3_cases.py and tests/test_gpu_conv3x3_routes.py use.  Touches no GPU.

Exact tier.  Inputs are small integers: x, dy in {-2..2} (a case may shrink this with `xmax`), w in {-1, 0, 1} drawn densely,
bias in {-8..8}, add / sub_from in {-16..16}, ReLU outputs used as masks are relu(integers in {-2..2}), sigmoid outputs used as masks are
drawn from {0, 0.5, 1} (y * (1 - y) is then 0 or 0.25, exact in float32).  Every product and every float32 partial sum of the f32 and of
the bf16 MFMA is an integer (or a quarter of one) far below 2**24, so the result does not depend on the summation order, and every value
a kernel stores as bf16 is an integer (or a quarter of one) of magnitude <= 256, which bf16 holds exactly.  The references are float64
conv2d / conv_transpose2d / conv2d_weight on the CPU; a GPU result that is not torch.equal to them is a kernel bug, not rounding.
test_cpu_conv3x3_cases.py checks the ranges that make this sound for every case and every expected tensor.

Forward and backward-data are ONE kernel (backward-data runs it on the flipped, transposed weight view), so the table lists shapes in
the kernel's terms: Cr = the channels it reduces over, Cp = the channels it produces.  The forward tests use a layer Cin = Cr, Cout = Cp;
the backward-data tests a layer Cout = Cr, Cin = Cp.  Every operation runs on every case, so every operation reaches every route.
"""
import functools
import os
import re
import zlib
from dataclasses import dataclass
from typing import Dict, Tuple

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vq-vae_amd", "csrc")

# ----------------------------------------------------------------------------------------------------------------------------------
# Constants of the host dispatch, with the place they were read from (line numbers as of the commit that added this file; the CPU test
# looks for the text, so a kernel change that moves a threshold fails there instead of leaving this table stale).
# ----------------------------------------------------------------------------------------------------------------------------------
TW = 16                # tile width of forward / bwd-data and of the generic weight gradient
TH_SHORT = 16          # forward / bwd-data tile height
TH_TALL = 32           # ... for bf16 images of at least TALL_MIN_H rows (hook frl_conv3x3_tile32 on)
TALL_MIN_H = 32
MAX_WG = 256           # persistent grids: min(tiles, 256)
LDS_BUDGET = 160 * 1024
F32_SMALL_CR = 16      # f32: Cr <= 16 -> CK 16, else CK 32
BF16_SMALL_CR = 32     # bf16: Cr <= 32 -> CK 32, else CK 64
VEC = {"f32": 4, "bf16": 8}
ESIZE = {"f32": 4, "bf16": 2}
WG_TH = 16             # generic weight gradient: 16 x 16 tiles
WG_SLICE = 64          # ... 64-channel output slices
WG_CHUNK = {"f32": 32, "bf16": 64}   # ... input chunks (IBC * 16)
BAND_TH, BAND_TW, BAND_C = 8, 32, 64  # bf16 band weight gradient: 8 x 32-pixel bands, Cin and Cout multiples of 64

SOURCE_CONSTANTS = [
    # (file, line, text that must be present, regex flag)
    ("conv3x3.hip", 19, "#define C3_TW 16"),
    ("conv3x3.hip", 104, "#define C3F_TH 16"),
    ("conv3x3.hip", 634, "const bool tall = g_c3_tile32 && sizeof(T) == 2 && H >= 32 && lds32 <= 160 * 1024;"),
    ("conv3x3.hip", 635, "const int TH = tall ? 32 : C3F_TH;"),
    ("conv3x3.hip", 645, "const int grid = tiles < 256 ? tiles : 256;"),
    ("conv3x3.hip", 657, "if (Cin <= 16) return launch_c3<float, 4>("),
    ("conv3x3.hip", 658, "return launch_c3<float, 8>("),
    ("conv3x3.hip", 660, "if (Cin <= 32) return launch_c3<bf16, 1>("),
    ("conv3x3.hip", 661, "return launch_c3<bf16, 2>("),
    ("conv3x3.hip", 182, "constexpr int q = NF * FE, CK = 4 * q;"),
    ("conv3x3.hip", 196, "const bool fast = (Cin % DT<T>::VEC) == 0;"),
    ("conv3x3.hip", 340, "if (nmb == 4 && (MB & 3) == 0 && (Cout & 63) == 0) {"),
    ("conv3x3.hip", 432, "if ((Cout & 3) == 0 && cb + 3 < Cout) {"),
    ("conv3x3.hip", 666, "#define C3W_TH 16"),
    ("conv3x3.hip", 669, "return tiles < 256 ? tiles : 256;"),
    ("conv3x3.hip", 734, "const bool band = c3v_supported(B, H, W, Cin, Cout, dtype) && (flags & 1) == 0;"),
    ("conv3x3.hip", 740, "for (int oc_base = 0; oc_base < Cout; oc_base += 64) {"),
    ("conv3x3.hip", 746, "auto kern = conv3x3_wgrad_kernel<float, 2, 1, 8>;"),
    ("conv3x3.hip", 752, "auto kern = conv3x3_wgrad_kernel<bf16, 4, 2, 8>;"),
    ("conv3x3.hip", 476, "const bool fastA = (Cout % V) == 0;"),
    ("conv3x3.hip", 36, "const bool fast = (C % V) == 0;"),
    ("conv3x3_wgrad.hip", 22, "#define C3V_TH 8"),
    ("conv3x3_wgrad.hip", 23, "#define C3V_TW 32"),
    ("conv3x3_wgrad.hip", 231,
     "return !g_c3v_off && dtype == FRL_BF16 && B > 0 && (W % C3V_TW) == 0 && (H % C3V_TH) == 0 && (Cin % 64) == 0 && (Cout % 64) == 0;"),
    ("conv3x3_wgrad.hip", 235, "return tiles < 256 ? tiles : 256;"),
    ("frl_common.hpp", 38, "static constexpr int VEC = 4;"),
    ("frl_common.hpp", 45, "static constexpr int VEC = 8;"),
]

DTYPES = ("f32", "bf16")


def _ceil(a: int, b: int) -> int:
    return (a + b - 1) // b


def _owners(tiles: int, grid: int) -> Tuple[int, ...]:
    """The distinct tile counts the workgroups of a persistent grid own."""
    return tuple(sorted({(tiles - w + grid - 1) // grid for w in range(grid)}))


# ----------------------------------------------------------------------------------------------------------------------------------
# Route classifiers
# ----------------------------------------------------------------------------------------------------------------------------------
def conv_route(dtype: str, B: int, H: int, W: int, Cr: int, Cp: int, tile32: bool = True) -> Dict:
    """The route of conv3x3_kernel (c3_dispatch / launch_c3) for Cr reduction channels and Cp produced channels."""
    if dtype == "f32":
        ck = 16 if Cr <= F32_SMALL_CR else 32
    else:
        ck = 32 if Cr <= BF16_SMALL_CR else 64
    pade = 16 // ESIZE[dtype]
    frag_bytes = 16 if dtype == "bf16" else 4
    nf = ck // (4 * (8 if dtype == "bf16" else 1))
    lds_w = 9 * 4 * nf * 64 * frag_bytes + _ceil(Cp, 16) * 16 * 4
    lds32 = (TH_TALL + 2) * (TW + 2) * (ck + pade) * ESIZE[dtype] + lds_w
    tall = bool(tile32) and dtype == "bf16" and H >= TALL_MIN_H and lds32 <= LDS_BUDGET
    th = TH_TALL if tall else TH_SHORT
    tiles = B * _ceil(H, th) * _ceil(W, TW)
    grid = min(tiles, MAX_WG)
    mb = _ceil(Cp, 16)
    noc = _ceil(mb, 4)
    return dict(th=th, tiles=tiles, grid=grid, owners=_owners(tiles, grid), rows_partial=H % th != 0, h_below_tile=H < th,
                w_ragged=W % TW != 0, fast=Cr % VEC[dtype] == 0, ck=ck, nck=_ceil(Cr, ck), chunk_partial=Cr % ck != 0,
                mb=mb, noc=noc, last_nmb=mb - 4 * (noc - 1),
                store="16" if Cp % 64 == 0 else "4" if Cp % 4 == 0 else "scalar", store4_partial_group=Cp % 4 == 0 and Cp % 16 != 0)


def wgrad_route(dtype: str, B: int, H: int, W: int, Cin: int, Cout: int, scalar_frags: bool = False, force_generic: bool = False) -> Dict:
    """The route of frl_conv3x3_bwd_weight."""
    band = (not force_generic and not scalar_frags and dtype == "bf16" and H % BAND_TH == 0 and W % BAND_TW == 0
            and Cin % BAND_C == 0 and Cout % BAND_C == 0)
    tiles = B * (H // BAND_TH) * (W // BAND_TW) if band else B * _ceil(H, WG_TH) * _ceil(W, TW)
    nwg = min(tiles, MAX_WG)
    tpw = _ceil(tiles, nwg)
    chunk = BAND_C if band else WG_CHUNK[dtype]
    return dict(kernel="band" if band else "generic", tiles=tiles, nwg=nwg, tpw=tpw, busy=_ceil(tiles, tpw), idle=nwg - _ceil(tiles, tpw),
                slices=_ceil(Cout, WG_SLICE), slice_partial=Cout % WG_SLICE != 0, chunks=_ceil(Cin, chunk), chunk_partial=Cin % chunk != 0,
                fast_dy=Cout % VEC[dtype] == 0, fast_halo=Cin % VEC[dtype] == 0,
                frag_reads="scalar" if (scalar_frags or dtype == "f32") and not band else "vector",
                ragged=H % WG_TH != 0 or W % TW != 0, hw=(H, W))


def conv_features(r: Dict, H: int, W: int) -> set:
    """The route values (the names of CONV_REQUIRED) that one classified case reaches."""
    th = f"th{r['th']}"
    f = {th, "stage.fast" if r["fast"] else "stage.scalar", f"store.{r['store']}"}
    if r["rows_partial"] and not r["h_below_tile"]:
        f.add(f"{th}.partial_row")
    if r["h_below_tile"]:
        f.add(f"{th}.H<TH")
    if H in (1, 2):
        f.add(f"H={H}")
    if r["w_ragged"]:
        f |= {"W.ragged", f"{th}.W.ragged"}
    if W in (1, 17):
        f.add(f"W={W}")
    if r["tiles"] > MAX_WG and r["owners"] == (1, 2):
        f.add(f"{th}.persistent.1and2")
    if r["nck"] == 1:
        f.add("nck=1")
    elif r["chunk_partial"]:
        f |= {"nck>1.partial", "nck>1.partial." + ("fast" if r["fast"] else "scalar")}
    if r["noc"] == 1:
        f.add("noc=1")
    elif r["last_nmb"] < 4:
        f.add("noc>1.nmb<4")
    if r["store4_partial_group"]:
        f.add("store.4.partial_group")
    if not r["fast"]:
        f.add(f"{th}.stage.scalar")
    return f


_CONV_COMMON = {"th16", "th16.partial_row", "th16.H<TH", "H=1", "H=2", "W.ragged", "th16.W.ragged", "W=1", "W=17", "th16.persistent.1and2",
                "stage.fast", "stage.scalar", "th16.stage.scalar", "nck=1", "nck>1.partial", "nck>1.partial.fast", "nck>1.partial.scalar",
                "noc=1", "noc>1.nmb<4", "store.16", "store.4", "store.4.partial_group", "store.scalar"}
# (float32 never takes the 32-row tile, and a 32-row tile is only chosen for H >= 32: "H < TH" does not exist under it)
CONV_REQUIRED = {"f32": set(_CONV_COMMON),
                 "bf16": _CONV_COMMON | {"th32", "th32.partial_row", "th32.W.ragged", "th32.persistent.1and2", "th32.stage.scalar"}}

# Operations of the forward / bwd-data kernel; every case runs all of them.  epi1 (the sigmoid gate blend) cannot be exact and is held to
# the tolerance tier on every case; epi3 is exact with out_y drawn from {0, 0.5, 1} and is held to the tolerance tier as well.
CONV_OPS = ("fwd", "bwd_mask", "epi0", "epi1", "epi2", "epi3")


def wgrad_features(dtype: str, c: "WgradCase") -> set:
    f = set()
    for scalar in (False, True):
        r = wgrad_route(dtype, c.B, c.H, c.W, c.Cin, c.Cout, scalar_frags=scalar)
        f |= {r["kernel"], f"generic.{r['frag_reads']}" if r["kernel"] == "generic" else "band.vector"}
        if r["kernel"] == "generic":
            if r["ragged"]:
                f.add("generic.ragged")
            if (c.H, c.W) == (1, 1):
                f.add("generic.1x1")
            if r["tpw"] > 1 and r["idle"] > 0:
                f.add("generic.tpw>1.idle")
            if r["slice_partial"] and r["slices"] > 1:
                f.add("generic.slices>1.partial")
            if r["chunk_partial"] and r["chunks"] > 1:
                f.add("generic.chunks>1.partial")
            f |= {f"generic.Cin={c.Cin}", f"generic.Cout={c.Cout}", "generic.dy." + ("fast" if r["fast_dy"] else "scalar"),
                  "generic.halo." + ("fast" if r["fast_halo"] else "scalar")}
        else:
            f.add(f"band.{c.H}x{c.W}")
            if (c.H, c.W) != (32, 32):
                f.add("band.not32x32")
            if r["tiles"] > MAX_WG:
                f.add("band.tiles>256")
            if r["tpw"] > 1 and r["idle"] > 0:
                f.add("band.tpw>1.idle")
            if r["slices"] > 1:
                f.add("band.slices>1")
            if r["chunks"] > 1:
                f.add("band.chunks>1")
    return f


_WG_COMMON = ({"generic", "generic.scalar", "generic.ragged", "generic.1x1", "generic.tpw>1.idle", "generic.slices>1.partial",
               "generic.chunks>1.partial", "generic.dy.fast", "generic.dy.scalar", "generic.halo.fast", "generic.halo.scalar"}
              | {f"generic.Cin={c}" for c in (4, 12, 40, 96)} | {f"generic.Cout={c}" for c in (3, 20, 72, 130)})
# (the float32 generic kernel has one fragment-read route, plain LDS reads; only bf16 has the transposing vector reads and the band kernel)
WGRAD_REQUIRED = {"f32": set(_WG_COMMON),
                  "bf16": _WG_COMMON | {"generic.vector", "band", "band.vector", "band.8x32", "band.24x96", "band.not32x32", "band.tiles>256",
                                        "band.tpw>1.idle", "band.slices>1", "band.chunks>1"}}
WGRAD_MASKS = ("none", "relu")


# ----------------------------------------------------------------------------------------------------------------------------------
# Case tables
# ----------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ConvCase:
    B: int
    H: int
    W: int
    Cr: int
    Cp: int
    xmax: int = 2
    ops: Tuple[str, ...] = CONV_OPS

    @property
    def name(self) -> str:
        return f"{self.B}x{self.H}x{self.W}x{self.Cr}to{self.Cp}"

    @property
    def seed(self) -> int:
        return zlib.crc32(("conv" + self.name).encode())


@dataclass(frozen=True)
class WgradCase:
    B: int
    H: int
    W: int
    Cin: int
    Cout: int
    xmax: int = 2

    @property
    def name(self) -> str:
        return f"{self.B}x{self.H}x{self.W}x{self.Cin}to{self.Cout}"

    @property
    def seed(self) -> int:
        return zlib.crc32(("wgrad" + self.name).encode())


CONV_CASES = [
    # --- the 32-row tile (bf16; float32 walks the same images in 16-row tiles) ---
    ConvCase(2, 33, 17, 130, 72),    # partial tall tile, W = 17, scalar staging, 3 chunks (last: 2 channels), 2 block groups (last: 1 block)
    ConvCase(75, 33, 17, 8, 8),      # 300 tall / 450 short tiles on 256 workgroups: the persistent loop and its halo prefetch across tiles
    ConvCase(65, 33, 17, 72, 72),    # 260 tall / 390 short tiles, several (out-chunk, in-chunk) stages per tile inside the persistent loop
    ConvCase(1, 65, 33, 96, 192),    # three tile rows (last: 1 image row), three full block groups, 16-wide stores
    ConvCase(1, 33, 17, 192, 96),    # the widest reduction of the table; 2 block groups (last: 2 blocks)
    ConvCase(1, 32, 32, 128, 64),    # exactly one tall tile row, whole chunks
    ConvCase(2, 48, 20, 64, 128),    # 32 + 16 rows, W = 20
    ConvCase(1, 40, 1, 16, 64),      # W = 1 under the tall tile; Cr = 16 is the last width of the float32 CK = 16 kernel
    ConvCase(1, 63, 5, 32, 96),      # H = 63; Cr = 32 is the last width of the bf16 CK = 32 kernel
    ConvCase(1, 64, 16, 8, 12),      # two whole tall tile rows; a 4-wide store with an empty last 4-group
    ConvCase(1, 33, 16, 24, 130),    # scalar stores, 3 block groups (last: 1 block); one partial chunk
    # --- the 16-row tile for both dtypes ---
    ConvCase(75, 17, 17, 8, 8),      # 300 short tiles on 256 workgroups
    ConvCase(3, 17, 15, 68, 20),     # partial short tile; 68 = scalar staging in bf16, vector staging in float32; 4-wide stores, Cp = 20
    ConvCase(1, 31, 16, 64, 64),     # one row short of the tall tile
    ConvCase(1, 17, 17, 40, 80),     # float32: 32 + 8 channels; Cp = 80: 2 block groups (last: 1 block)
    ConvCase(1, 9, 11, 12, 8),       # H < 16; the ragged shape of test_backward_epilogue_sums_match_separate_launches
    ConvCase(1, 16, 16, 6, 6),       # one whole tile, scalar staging and scalar stores
    ConvCase(2, 1, 1, 12, 3),        # a single pixel
    ConvCase(1, 2, 17, 3, 12),       # H = 2, W = 17
    ConvCase(2, 5, 7, 4, 20),        # Cr = 4: one float32 vector, scalar in bf16
    ConvCase(1, 8, 8, 17, 16),       # Cr = 17: first width of the float32 CK = 32 kernel, scalar staging
    ConvCase(1, 8, 40, 33, 4),       # Cr = 33: first width of the bf16 CK = 64 kernel, scalar staging
    ConvCase(1, 20, 18, 130, 3),     # scalar staging with several chunks under the short tile
]

WGRAD_CASES = [
    WgradCase(1, 1, 1, 4, 3),
    WgradCase(1, 2, 1, 12, 12),
    WgradCase(1, 9, 11, 12, 8),
    WgradCase(2, 33, 17, 130, 72),   # ragged tiles; Cin 130 = 2 (4) whole chunks + 2 channels; a second output slice of 8 channels
    WgradCase(75, 33, 17, 8, 8),     # 450 tiles on 256 workgroups: two tiles each, 31 idle workgroups write zero slabs
    WgradCase(3, 17, 15, 68, 20),
    WgradCase(1, 20, 40, 40, 130),   # three output slices, the last of 2 channels
    WgradCase(2, 7, 5, 96, 20),
    WgradCase(1, 17, 33, 20, 6),
    WgradCase(1, 16, 16, 64, 64),    # whole tiles and chunks, generic for both dtypes (W is no multiple of 32)
    WgradCase(1, 65, 33, 96, 192),   # three whole output slices
    # --- band-eligible (bf16; float32 takes the generic kernel) ---
    WgradCase(1, 8, 32, 64, 64),     # one band
    WgradCase(1, 32, 32, 64, 64),
    WgradCase(2, 24, 96, 128, 64),   # 3 x 3 bands per image, two input chunks
    WgradCase(1, 8, 64, 64, 128),    # two output slices
    WgradCase(100, 24, 32, 64, 64),  # 300 bands on 256 workgroups: two each, 106 idle workgroups
]

# Tolerance tier (sigmoid paths, random data), as LAYER shapes (B, H, W, Cin, Cout): one on the vector routes under the tall tile, one on
# the scalar routes with ragged tiles.
TOL_SHAPES = [(2, 33, 17, 64, 64), (3, 17, 15, 70, 6)]


# ----------------------------------------------------------------------------------------------------------------------------------
# Exact-tier data and references (float64 on the CPU, returned as float32: every value is an integer or a quarter of one, |v| < 2**24)
# ----------------------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=2)
def conv_exact(case: ConvCase):
    """-> (inputs, expected): NHWC float32 tensors of the exact tier for one kernel shape.

    inputs:   x [B,H,W,Cr] (the forward input, and dy of the backward calls), w_fwd [Cp,Cr,3,3], bias [Cp], w_bwd [Cr,Cp,3,3] (the weight
              of a layer Cin = Cp, Cout = Cr), y_relu_mask [B,H,W,Cr] (a ReLU output: the layer's y), add / sub_from [B,H,W,Cp],
              out_y_relu / out_y_sig [B,H,W,Cp]
    expected: y_none, y_relu; dx_plain, dx_mask (ReLU mask); dx_add = dx_mask + add; out2_sub = sub_from - dx_plain;
              out2_both = sub_from - dx_add; dx_out_relu = dx_plain .* (out_y_relu > 0); dx_out_sig = dx_mask .* out_y_sig (1 - out_y_sig)
    """
    g = torch.Generator().manual_seed(case.seed)
    B, H, W, Cr, Cp, m = case.B, case.H, case.W, case.Cr, case.Cp, case.xmax
    x = _ints(g, (B, H, W, Cr), -m, m)
    w_fwd = _ints(g, (Cp, Cr, 3, 3), -1, 1)
    bias = _ints(g, (Cp,), -8, 8)
    w_bwd = _ints(g, (Cr, Cp, 3, 3), -1, 1)
    y_relu_mask = _ints(g, (B, H, W, Cr), -2, 2).clamp(min=0)
    add = _ints(g, (B, H, W, Cp), -16, 16)
    sub = _ints(g, (B, H, W, Cp), -16, 16)
    out_y_relu = _ints(g, (B, H, W, Cp), -2, 2).clamp(min=0)
    out_y_sig = _ints(g, (B, H, W, Cp), 0, 2) * 0.5
    y_none = _nhwc(F.conv2d(_nchw(x), w_fwd, bias, padding=1))
    dx_plain = _nhwc(F.conv_transpose2d(_nchw(x), w_bwd, padding=1))
    dx_mask = _nhwc(F.conv_transpose2d(_nchw(x * (y_relu_mask > 0)), w_bwd, padding=1))
    dx_add = dx_mask + add
    inputs = dict(x=x, w_fwd=w_fwd, bias=bias, w_bwd=w_bwd, y_relu_mask=y_relu_mask, add=add, sub_from=sub, out_y_relu=out_y_relu,
                  out_y_sig=out_y_sig)
    expected = dict(y_none=y_none, y_relu=y_none.clamp(min=0), dx_plain=dx_plain, dx_mask=dx_mask, dx_add=dx_add, out2_sub=sub - dx_plain,
                    out2_both=sub - dx_add, dx_out_relu=dx_plain * (out_y_relu > 0), dx_out_sig=dx_mask * (out_y_sig * (1 - out_y_sig)))
    return {k: v.float() for k, v in inputs.items()}, {k: v.float() for k, v in expected.items()}


# which operation each expected tensor of conv_exact belongs to (the kernel stores every one of them in the activation dtype)
CONV_EXPECTED_OPS = {"y_none": "fwd", "y_relu": "fwd", "dx_plain": "epi0", "dx_mask": "bwd_mask", "dx_add": "epi0", "out2_sub": "epi0",
                     "out2_both": "epi0", "dx_out_relu": "epi2", "dx_out_sig": "epi3"}


@functools.lru_cache(maxsize=2)
def wgrad_exact(case: WgradCase):
    """-> (inputs, expected): x [B,H,W,Cin], dy / y_relu_mask [B,H,W,Cout]; dw_none, db_none, dw_relu, db_relu (float32 results)."""
    g = torch.Generator().manual_seed(case.seed)
    B, H, W, Cin, Cout, m = case.B, case.H, case.W, case.Cin, case.Cout, case.xmax
    x = _ints(g, (B, H, W, Cin), -m, m)
    dy = _ints(g, (B, H, W, Cout), -m, m)
    y_relu_mask = _ints(g, (B, H, W, Cout), -2, 2).clamp(min=0)
    expected = {}
    for mask, d in (("none", dy), ("relu", dy * (y_relu_mask > 0))):
        expected[f"dw_{mask}"] = torch.nn.grad.conv2d_weight(_nchw(x), (Cout, Cin, 3, 3), _nchw(d), padding=1)
        expected[f"db_{mask}"] = d.sum(dim=(0, 1, 2))
    inputs = dict(x=x, dy=dy, y_relu_mask=y_relu_mask)
    return {k: v.float() for k, v in inputs.items()}, {k: v.float() for k, v in expected.items()}


def source_text(name: str) -> str:
    with open(os.path.join(CSRC, name), encoding="utf-8") as f:
        return f.read()


def squeeze_ws(s: str) -> str:
    return re.sub(r"\s+", " ", s)
