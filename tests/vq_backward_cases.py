"""Shared cases for the quantizer's backward and EMA kernels (csrc/vq.hip: vq_bwd_kernel<float>, the three vq_bwd_mfma_kernel instances,
the CodeEpi slab reduction, vq_ema_kernel): seeded inputs with SYNTHETIC indices, the float64 reference, a-priori error bounds, a float32
emulation of the kernels' arithmetic with mutants, and the case table.  Touches no GPU.

    reference (float64, on the inputs as the kernel sees them: z and g_out rounded to the row dtype, E_eff = the codebook rounded to bf16
    in bf16 mode and the codebook itself in float32 mode, gscale as float32 values):
        g_z = g_out + cz (z - E_eff[idx])        cz = gscale[0] beta 2 / (N d)
        S_k = sum_{n: idx_n = k} z_n
        g_E = ce (n_k E_eff_k - S_k)             ce = gscale[1] 2 / (N d)

    bounds (elementwise; u32 = 2^-24; u_T = 2^-8 for bf16 rows -- one round-to-nearest-even of the float32 value -- and u32 for float32):
        g_z   u_T |g_z| + 8 u32 (|g_out| + |cz| (|z| + |e|))
              cz is four float32 operations (beta * 2, N * d, the division, times gscale[0]), then the subtraction, the multiply and
              the add: seven roundings on the commitment term, two on g_out
        S     (n_k + 16) u32 sum_n |z_nj|
              any order of at most n_k additions inside a workgroup, plus the reduction of the 256 slabs (4 sequential + 3 tree + 8
              sequential additions per element)
        g_E   |ce| (bound_S + 4 u32 (n_k |e| + sum |z|))
              ce is three float32 operations, n_k e and the subtraction one each
    A bound of zero (an unused code: n_k = 0) means the output must be exact.

    EMA (float64 on float32 sums, int32 counts and the float32 VALUES of decay and eps, 1 - decay32 taken in float64: the float32
    subtraction 1.f - decay is exact for decay in [0.5, 1]):
        N_k = decay N_k + (1 - decay) n_k,  m_k = decay m_k + (1 - decay) S_k,  n = sum N_k
        e_k = m_k / ((N_k + eps) / (n + K eps) n)
        bounds:  moments 4 u32 (decay |old| + (1 - decay) |new|);  codebook 16 u32 (decay |old_sum| + (1 - decay) |sums|) / smoothed

The case table restates what the kernels branch on (KC of the matrix-core instances, vq_bwd_chunk of the float32 kernel, the row partition
over the 256 workgroups); every case names the branch it is there for and runs in both row dtypes.
"""
import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
WGS = 256                                                # VQ_BWD_WGS
BETA = 0.25
GS_A, GS_B = 0.37, -1.9                                  # gscale = [a N d, b N d]: both terms O(1) against g_out, different sign and size
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


# ---------------------------------------------------------------------------------------------------------------------------------
# what the host code of frl_vq_bwd decides
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_instance(d: int) -> Tuple[int, int, int]:
    """(RB, CB, NWV) of the vq_bwd_mfma_kernel instance that serves d channels."""
    if not 0 < d <= 128:
        raise ValueError("bf16 backward: 0 < d <= 128")
    return (4, 2, 8) if d <= 32 else (4, 4, 8) if d <= 64 else (2, 8, 8)


def bf16_chunk(d: int) -> int:
    rb, _, nwv = bf16_instance(d)
    return rb * nwv * 16                                 # KC: 512 codes for d <= 64, 256 above


def f32_chunk(k: int, d: int) -> int:
    """vq_bwd_chunk: halve (rounding up) until the chunk's float32 accumulators fit 96 KiB of LDS."""
    kc = k
    while kc * d * 4 > 96 * 1024 and kc > 1:
        kc = (kc + 1) // 2
    return kc


def chunk(k: int, d: int, dtype: str) -> int:
    return f32_chunk(k, d) if dtype == "f32" else bf16_chunk(d)


def chunk_sizes(k: int, d: int, dtype: str) -> List[int]:
    kc = chunk(k, d, dtype)
    return [min(kc, k - b) for b in range(0, k, kc)]


def f32_lds_bytes(k: int, d: int) -> int:
    return f32_chunk(k, d) * d * 4


def rows_per_workgroup(n: int, dtype: str) -> int:
    rows = (n + WGS - 1) // WGS
    return rows if dtype == "f32" else (rows + 63) // 64 * 64


def row_partition(n: int, dtype: str) -> List[Tuple[int, int]]:
    """[r0, r1) of each of the 256 workgroups (r0 == r1: an empty workgroup, which still writes its slab of zeros)."""
    rows = rows_per_workgroup(n, dtype)
    return [(min(w * rows, n), min((w + 1) * rows, n)) for w in range(WGS)]


def vector_path(d: int, dtype: str) -> bool:
    return d % (4 if dtype == "f32" else 8) == 0


def padded_width(d: int) -> int:
    return bf16_instance(d)[1] * 16


def branches(n: int, k: int, d: int, dtype: str) -> set:
    """Names of the branches a shape reaches in the kernel that serves it."""
    out = {"instance:" + ("f32" if dtype == "f32" else "%d,%d,%d" % bf16_instance(d))}
    cs = chunk_sizes(k, d, dtype)
    out.add("chunks:%s" % (len(cs) if len(cs) < 3 else ">=3"))
    if len(cs) > 1 and cs[-1] != cs[0]:
        out.add("ragged_last_chunk")
    out.add("vector" if vector_path(d, dtype) else "scalar")
    if dtype == "bf16" and d < padded_width(d):
        out.add("below_padded_width")
    if dtype == "f32" and f32_lds_bytes(k, d) > 64 * 1024:
        out.add("lds_opt_in")
    part = row_partition(n, dtype)
    sizes = [b - a for a, b in part]
    live = [s for s in sizes if s]
    if len(live) < WGS:
        out.add("empty_workgroups")
    if live[-1] == 1:
        out.add("one_row_last_workgroup")
    if dtype == "bf16":
        if any(s % 64 for s in live):
            out.add("partial_last_tile")
        if n < 64:
            out.add("n_below_tile")
        if max(live) > 64:
            out.add("several_tiles")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("uniform", "one_code", "edges", "half_unused", "sorted")


@dataclass(frozen=True)
class Case:
    n: int
    k: int
    d: int
    pattern: str
    why: str

    @property
    def id(self) -> str:
        return f"N{self.n}-K{self.k}-d{self.d}-{self.pattern}"

    @property
    def seed(self) -> int:
        return (self.n * 7919 + self.k * 104729 + self.d * 31 + PATTERNS.index(self.pattern)) % (2 ** 31 - 1)


def make_idx(case: Case, dtype: str, g: torch.Generator) -> torch.Tensor:
    n, k = case.n, case.k
    if case.pattern == "uniform":
        idx = torch.randint(0, k, (n,), generator=g)
    elif case.pattern == "one_code":
        idx = torch.full((n,), k - 1)
    elif case.pattern == "edges":
        kc = chunk(k, case.d, dtype)                     # first and last code of a chunk, of the codebook and of a 16-code block
        codes = sorted({c for c in (0, kc - 1, kc, k - 1, 15, 16) if 0 <= c < k})
        idx = torch.tensor(codes)[torch.randint(0, len(codes), (n,), generator=g)]
    elif case.pattern == "half_unused":
        idx = torch.randint(0, max(k // 2, 1), (n,), generator=g)
    elif case.pattern == "sorted":
        idx = torch.sort(torch.randint(0, k, (n,), generator=g)).values
    else:
        raise ValueError(case.pattern)
    return idx.to(torch.int32)


@functools.lru_cache(maxsize=4)
def inputs(case: Case, dtype: str) -> Dict[str, torch.Tensor]:
    """CPU tensors: z, g_out (row dtype), codebook (float32), e_eff (float32: what the kernel takes as the codebook), idx / counts (int32),
    zq (row dtype: e_eff[idx], exact), gscale (float32 [2]), and the float64 per-code sums of z and |z| every reference shares."""
    g = torch.Generator().manual_seed(case.seed)
    t = DTYPES[dtype]
    z = torch.randn(case.n, case.d, generator=g).to(t)
    g_out = torch.randn(case.n, case.d, generator=g).to(t)
    codebook = torch.randn(case.k, case.d, generator=g)
    idx = make_idx(case, dtype, g)
    counts = torch.bincount(idx.long(), minlength=case.k).to(torch.int32)
    e_eff = codebook.to(t).float()
    gscale = torch.tensor([GS_A * case.n * case.d, GS_B * case.n * case.d], dtype=torch.float32)
    sums64 = torch.zeros(case.k, case.d, dtype=torch.float64).index_add_(0, idx.long(), z.double())
    abs_sums64 = torch.zeros(case.k, case.d, dtype=torch.float64).index_add_(0, idx.long(), z.double().abs())
    return dict(z=z, g_out=g_out, codebook=codebook, e_eff=e_eff, idx=idx, counts=counts, zq=e_eff[idx.long()].to(t), gscale=gscale,
                sums64=sums64, abs_sums64=abs_sums64)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def scales64(n: int, d: int, gscale: Optional[torch.Tensor], beta: float) -> Tuple[float, float]:
    gs0, gs1 = (1.0, 1.0) if gscale is None else (float(gscale[0]), float(gscale[1]))     # the float32 values, exactly
    return gs0 * beta * 2.0 / (n * d), gs1 * 2.0 / (n * d)


def reference(inp, gscale: Optional[torch.Tensor], beta: float, with_gout: bool = True) -> Dict[str, torch.Tensor]:
    """float64 outputs and their bounds: gz, sums, ge and gz_bound, sums_bound, ge_bound."""
    z, e, idx = inp["z"].double(), inp["e_eff"].double(), inp["idx"].long()
    n, d = z.shape
    k = e.shape[0]
    g_out = inp["g_out"].double() if with_gout else torch.zeros_like(z)
    cz, ce = scales64(n, d, gscale, beta)
    eg = e[idx]
    gz = g_out + cz * (z - eg)
    sums, abs_sums = inp["sums64"], inp["abs_sums64"]
    nk = torch.bincount(idx, minlength=k).double()[:, None]
    ge = ce * (nk * e - sums)
    u_t = U32 if inp["z"].dtype == torch.float32 else U_BF16
    gz_bound = u_t * gz.abs() + 8 * U32 * (g_out.abs() + abs(cz) * (z.abs() + eg.abs()))
    sums_bound = torch.where(nk > 0, (nk + 16) * U32 * abs_sums, torch.zeros_like(abs_sums))
    ge_bound = abs(ce) * (sums_bound + 4 * U32 * (nk * e.abs() + abs_sums))
    return dict(gz=gz, sums=sums, ge=ge, gz_bound=gz_bound, sums_bound=sums_bound, ge_bound=ge_bound)


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - ref| / bound; where the bound is zero the output must be exact (inf otherwise); NaN counts as inf."""
    err = (got.detach().to("cpu", torch.float64) - ref).abs()
    if err.numel() == 0:
        return 0.0
    if bool((torch.isnan(err) | ((bound == 0) & (err != 0))).any()):
        return float("inf")
    return float(torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 emulation of the kernels' arithmetic (and mutants of it)
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("swapped_gscale", "moved_row", "unrounded_codebook", "no_commit")


def mutant_applies(mutant: str, case: Case, dtype: str, gscale, beta: float, with_gout: bool = True) -> bool:
    """Whether the mutant changes an output by more than its bound BY CONSTRUCTION of the inputs: the commitment term is O(1) against g_out
    only under the large upstream scales (or alone, without g_out); with gscale = None it is ~1e-5 of g_out, below one bf16 rounding."""
    if mutant == "swapped_gscale":
        return gscale is not None
    if mutant == "moved_row":
        return case.k > 1
    if mutant == "unrounded_codebook":
        return dtype == "bf16"
    if mutant == "no_commit":
        return beta != 0 and (gscale is not None or not with_gout)
    raise ValueError(mutant)


def slab_reduce32(slab: torch.Tensor) -> torch.Tensor:
    """slab_reduce_t over 256 float32 slabs [256, ...]: slab w = 64 t + 8 j + grp goes to accumulator j of slab group grp in step t; then
    s_j += s_{j+4}, (s0 + s1) + (s2 + s3), and the eight groups in order."""
    v = slab.reshape(4, 8, 8, -1)                                                   # [t, j, grp, element]
    s = torch.zeros_like(v[0])
    for t in range(4):
        s = s + v[t]
    s = s[:4] + s[4:]
    r = (s[0] + s[1]) + (s[2] + s[3])                                               # [grp, element]
    out = r[0]
    for grp in range(1, 8):
        out = out + r[grp]
    return out.reshape(slab.shape[1:])


def emulate_idx(inp, mutant: Optional[str] = None) -> torch.Tensor:
    idx = inp["idx"].long().clone()
    if mutant == "moved_row":                                                       # one row goes to a neighbouring code
        r, k = idx.numel() // 2, inp["codebook"].shape[0]
        idx[r] = idx[r] + 1 if idx[r] + 1 < k else idx[r] - 1
    return idx


def emulate_sums(inp, dtype: str, mutant: Optional[str] = None) -> torch.Tensor:
    """Per-code sums as the kernels form them in float32: per workgroup in row order, then the fixed-order reduction of the 256 slabs."""
    z, idx = inp["z"].float(), emulate_idx(inp, mutant)
    n, d = z.shape
    k = inp["codebook"].shape[0]
    wg = torch.arange(n) // rows_per_workgroup(n, dtype)
    slab = torch.zeros(WGS * k, d, dtype=torch.float32).index_add_(0, wg * k + idx, z)
    return slab_reduce32(slab.reshape(WGS, k, d))


def emulate(inp, dtype: str, gscale: Optional[torch.Tensor], beta: float, with_gout: bool = True, mutant: Optional[str] = None,
            sums: Optional[torch.Tensor] = None):
    """float32 arithmetic in the kernels' order: float32 scale factors, g_z rounded once to the row dtype, g_E from the emulated per-code
    sums (`sums`: those of emulate_sums for this mutant, when the caller already has them).  -> dict(gz [row dtype], sums, ge [float32])."""
    t = DTYPES[dtype]
    z, idx = inp["z"].float(), emulate_idx(inp, mutant)
    n, d = z.shape
    e = inp["codebook"] if mutant == "unrounded_codebook" else inp["e_eff"]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    nd = f(float(n)) * f(float(d))
    gs = torch.ones(2) if gscale is None else gscale.clone()
    if mutant == "swapped_gscale":
        gs = gs.flip(0)
    cz = (f(beta) * f(2.0)) / nd * gs[0]
    ce = f(2.0) / nd * gs[1]
    if mutant == "no_commit":
        cz = f(0.0)
    g_out = inp["g_out"].float() if with_gout else torch.zeros_like(z)
    gz = (g_out + cz * (z - e[idx])).to(t)
    if sums is None:
        sums = emulate_sums(inp, dtype, mutant)
    counts = inp["counts"].float()[:, None]
    ge = ce * (counts * e - sums)
    return dict(gz=gz, sums=sums, ge=ge)


def ratios(out, ref) -> Dict[str, float]:
    return {name: ratio(out[name], ref[name], ref[name + "_bound"]) for name in ("gz", "sums", "ge") if out.get(name) is not None}


# ---------------------------------------------------------------------------------------------------------------------------------
# EMA
# ---------------------------------------------------------------------------------------------------------------------------------
EMA_SHAPES = ((96, 64), (1000, 12), (1, 8), (513, 128))           # K <= 256, the strided loop, one code, a wide row
EMA_DECAY, EMA_EPS = 0.99, 1e-5


def ema_inputs(k: int, d: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """float32 sums / int32 counts with the upper half of the codes unused (K = 1: used), old moments with every third count at zero."""
    g = torch.Generator().manual_seed(1000 * k + d + seed)
    counts = torch.randint(1, 200, (k,), generator=g).to(torch.int32)
    sums = torch.randn(k, d, generator=g) * counts[:, None].float().sqrt()
    if k > 1:
        counts[k // 2:] = 0
        sums[k // 2:] = 0
    ema_count = torch.rand(k, generator=g) * 10
    if k > 1:
        ema_count[::3] = 0
    ema_sum = torch.randn(k, d, generator=g)
    codebook = torch.randn(k, d, generator=g)
    return dict(sums=sums, counts=counts, ema_count=ema_count, ema_sum=ema_sum, codebook=codebook)


def ema_scalars(decay: float, eps: float, rounded: bool = True) -> Tuple[float, float]:
    """The values the kernel receives (float32 arguments), as Python floats."""
    if not rounded:
        return decay, eps
    return float(torch.tensor(decay, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))


def ema_reference(inp, decay: float = EMA_DECAY, eps: float = EMA_EPS, rounded: bool = True) -> Dict[str, torch.Tensor]:
    """float64 -> codebook, ema_count, ema_sum and their bounds."""
    dc, ep = ema_scalars(decay, eps, rounded)
    sums, counts = inp["sums"].double(), inp["counts"].double()
    oc, osum = inp["ema_count"].double(), inp["ema_sum"].double()
    k = counts.shape[0]
    nc = dc * oc + (1.0 - dc) * counts
    ms = dc * osum + (1.0 - dc) * sums
    n = nc.sum()
    smoothed = (nc + ep) / (n + k * ep) * n
    return dict(codebook=ms / smoothed[:, None], ema_count=nc, ema_sum=ms,
                ema_count_bound=4 * U32 * (dc * oc.abs() + (1.0 - dc) * counts.abs()),
                ema_sum_bound=4 * U32 * (dc * osum.abs() + (1.0 - dc) * sums.abs()),
                codebook_bound=16 * U32 * (dc * osum.abs() + (1.0 - dc) * sums.abs()) / smoothed[:, None])


def ema_emulate(inp, decay: float = EMA_DECAY, eps: float = EMA_EPS) -> Dict[str, torch.Tensor]:
    """vq_ema_kernel in float32 (the total count in float64, cast back, as the kernel does)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    dc, ep = f(decay), f(eps)
    k = inp["counts"].shape[0]
    nc = dc * inp["ema_count"] + (f(1.0) - dc) * inp["counts"].float()
    n = nc.double().sum().float()
    ms = dc * inp["ema_sum"] + (f(1.0) - dc) * inp["sums"]
    smoothed = (nc + ep) / (n + f(float(k)) * ep) * n
    return dict(codebook=ms / smoothed[:, None], ema_count=nc, ema_sum=ms)


def ema_ratios(out, ref) -> Dict[str, float]:
    return {name: ratio(out[name], ref[name], ref[name + "_bound"]) for name in ("codebook", "ema_count", "ema_sum")}


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
N_SWEEP = ((1, "uniform", "one row: 255 empty workgroups, N below a tile"),
           (63, "uniform", "N below a 64-row tile"),
           (65, "sorted", "bf16: one tile and one row in one workgroup; float32: one row per workgroup, 191 empty"),
           (300, "one_code", "bf16: four full tiles and a 44-row tile, 251 empty workgroups; float32: two rows per workgroup"),
           (16384, "uniform", "every workgroup exactly one full tile"),
           (16385, "half_unused", "bf16: a last workgroup of one row behind 128 full ones; float32: a last workgroup of five rows"),
           (16421, "sorted", "bf16: a partial last tile of 37 rows"),
           (40000, "uniform", "three tiles per workgroup, a 64-row last workgroup, empty ones behind it"))
N_SWEEP_SHAPES = ((16, 8, "instance 4,2,8"), (37, 40, "instance 4,4,8 below its padded width"), (37, 72, "instance 2,8,8 below its padded width"),
                  (37, 12, "float32 kernel, vector path; bf16: d % 8 != 0, scalar path"))
KD_SWEEP = ((16, 12, "uniform", "bf16 scalar channel path at the phase latent's width"),
            (512, 32, "edges", "4,2,8: one full 512-code chunk at the full padded width"),
            (513, 8, "edges", "4,2,8: a second chunk of one code"),
            (1030, 32, "half_unused", "4,2,8: three chunks, the last of six codes"),
            (37, 50, "uniform", "4,4,8: scalar channel path (d % 8 = 2)"),
            (512, 64, "edges", "4,4,8: one full chunk; float32: two chunks of 256 codes at exactly 64 KiB"),
            (513, 40, "sorted", "4,4,8: a second chunk of one code"),
            (1030, 64, "edges", "4,4,8: three chunks; float32: four chunks (258, 258, 258, 256) above 64 KiB of LDS"),
            (256, 128, "half_unused", "2,8,8: one full 256-code chunk at the full width"),
            (257, 72, "edges", "2,8,8: a second chunk of one code"),
            (600, 100, "uniform", "2,8,8: three chunks, scalar channel path (d % 8 = 4)"),
            (600, 128, "sorted", "2,8,8: three chunks; float32: four chunks of 150 codes, 75 KiB of LDS"),
            (385, 64, "edges", "float32: two uneven chunks (193, 192)"),
            (37, 10, "uniform", "float32: d % 4 != 0, scalar path"),
            (1, 8, "one_code", "a codebook of one code"))
KD_SWEEP_N = 3000


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    out = [Case(n, k, d, pat, f"{shape_why}; {why}") for k, d, shape_why in N_SWEEP_SHAPES for n, pat, why in N_SWEEP]
    out += [Case(KD_SWEEP_N, k, d, pat, why) for k, d, pat, why in KD_SWEEP]
    assert len({c.id for c in out}) == len(out)
    assert max(WGS * c.k * c.d * 4 for c in out) < 100e6
    return tuple(out)


CASE_IDS = tuple(c.id for c in cases())


def case_by_id(cid: str) -> Case:
    return cases()[CASE_IDS.index(cid)]


# the multi-chunk cases of the deferred-reduction check: (case id, dtype).  The float32 kernel sums with LDS float atomics, whose order is
# free; with N = 300 a float32 workgroup holds two rows, a code gets at most two addends per workgroup, and a sum of two floats does not
# depend on the order -- so the float32 result is reproducible there and its bits may be compared.
def deferred_cases() -> Tuple[Tuple[Case, str], ...]:
    return ((Case(3000, 1030, 32, "uniform", "bf16: three chunks"), "bf16"),
            (Case(300, 385, 64, "uniform", "float32: two chunks, at most two rows per workgroup"), "f32"))
