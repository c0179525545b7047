"""Cases, inputs, the float64 restatement and the error bounds for the EVT-stratified diagnostics (test_cpu_strata.py,
test_gpu_strata.py).

Inputs are regenerated from numpy's default_rng, never stored; tests/golden/strata_*.npz (tests/golden/make_strata_golden.py) holds
what the reference's own functions gave for them, and a checksum of the inputs.  No product code is imported here; numpy only.

Keys.  codes [B, P] int32 or float32; valid where finite and > 0 (the reference's np.isfinite(evt_grid) & (evt_grid > 0)), a valid float
truncated as astype(np.int32).  In this order an observation (b, t, p) is dropped by its mask, dropped for an invalid code, counted as
`unmatched` for a valid code outside the vocabulary, counted as `rejected` for a row label outside [0, R).

Bounds (u = 2^-24), none of them taken from the code under test.  For a group with n contributing rows and float32 terms t_i, float32
accumulation in any order, with the pivot subtraction and the square before it, is off by at most (n + T + 8) u sum |t_i|; the slab sums in
double add nothing visible.  What the terms are:
  observations mode: y = x - pivot carries one rounding, y^2 three, the sum n: terms |y| for S1, y^2 for S2 (T counts for nothing).
  temporal mode: the pixel mean mu of y_t is a chain of T terms y_t / T, each with the rounding of its subtraction, then one division:
  |mu~ - mu| <= (T + 1) u a with a = mean_t |y_t| >= |mu|.  Terms a for S1.  mu~^2 - mu^2 is within 2 |mu| (T + 1) u a + u mu^2
  <= (2 T + 3) u a^2, so the terms of S2 are 2 a^2: (n + T + 8) 2 a^2 >= (n + 2 T + 3) a^2.  For SW, d_t = y_t - mu~ is off by
  u |y_t| + u |d_t| plus the shift of mu~, whose first order cancels in sum_t d_t^2 because sum_t d_t = 0; squares, the fmaf chain over t and
  the division add (T + 4) u w.  Terms mean_t (d_t^2 + 2 |d_t| |y_t|).
This is a derived worst case, not a measurement.  `propagate_*` carry the bounds to first order to the mean, the standard deviation,
the temporal fraction and R^2, doubled for the higher orders; for a standard deviation near zero |sqrt(a) - sqrt(b)| <= sqrt(|a - b|).

Where a standard deviation is compared (the end-to-end case) the data keeps every class's standard deviation at 1e-2 or more of its
spread about the pivot (the root mean square of x - pivot), so that its bound stays meaningful; `e2e_inputs` asserts this on what it
makes (`assert_spread`; a class of one row has none and is held to the square-root form of the bound).
"""
from __future__ import annotations

import zlib

import numpy as np

U32 = 2.0 ** -24
LDS_CELLS = 8192                                                                 # R * G up to which the table kernel counts in LDS


def checksum(*arrays) -> int:
    h = 0
    for a in arrays:
        if a is not None:
            h = zlib.crc32(np.ascontiguousarray(a).tobytes(), h)
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------------------------------------
def make_vocab(rng, g: int) -> np.ndarray:
    """g distinct positive codes, increasing."""
    return np.sort(rng.choice(np.arange(1, 4 * g + 10), size=g, replace=False)).astype(np.int32)


def make_codes(rng, vocab: np.ndarray, shape, as_float: bool, coherent: bool = False, junk: float = 0.1, full=None) -> np.ndarray:
    """Codes mostly from `vocab`; `junk` of them are valid codes outside the vocabulary (`full`, where `vocab` is a part of it), or
    invalid: 0, negative, and for floats NaN, +-inf; float codes of the vocabulary carry a fraction that the truncation drops."""
    n = int(np.prod(shape))
    full = vocab if full is None else full
    if coherent:                                                                 # runs of equal codes
        run = rng.integers(0, len(vocab), size=n // 16 + 1)
        c = vocab[np.repeat(run, 16)[:n]].astype(np.int64)
    else:
        c = vocab[rng.integers(0, len(vocab), size=n)].astype(np.int64)
    absent = np.setdiff1d(np.arange(1, int(full.max()) + 6), full)
    kind = rng.random(n)
    out = c.astype(np.float64)
    if as_float:
        out += rng.random(n) * 0.9                                               # a non-integer float truncates to its code
    sel = kind < junk / 2
    out[sel] = absent[rng.integers(0, len(absent), size=int(sel.sum()))]
    bad = (kind >= junk / 2) & (kind < junk)
    pool = np.array([0.0, -1.0, -7.0, np.nan, np.inf, -np.inf, 0.0]) if as_float else np.array([0.0, -1.0, -7.0])
    out[bad] = pool[rng.integers(0, len(pool), size=int(bad.sum()))]
    return (out.astype(np.float32) if as_float else out.astype(np.int32)).reshape(shape)


def lookup(codes: np.ndarray, vocab: np.ndarray):
    """-> (valid bool, column int64 (-1: not in the vocabulary)) of codes of any shape."""
    c = np.asarray(codes)
    if np.issubdtype(c.dtype, np.floating):
        valid = np.isfinite(c) & (c > 0)
        ci = np.where(valid, c, 0).astype(np.int32)
    else:
        valid = c > 0
        ci = c.astype(np.int32)
    pos = np.searchsorted(vocab, ci)
    hit = valid & (pos < len(vocab)) & (vocab[np.minimum(pos, len(vocab) - 1)] == ci)
    return valid, np.where(hit, pos, -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the contingency table
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, T, P) x (R, G): 15 000 cells is the global-atomic path, 4 x 2048 the LDS path at its edge, 3 x 2731 one cell past it
TABLE_SHAPES = [(1, 1, 1), (1, 1, 63), (2, 1, 257), (3, 5, 1000)]
TABLE_SIZES = [(1, 1), (20, 15), (50, 300), (4, 2048), (3, 2731)]
assert 4 * 2048 == LDS_CELLS and 3 * 2731 == LDS_CELLS + 1


def table_case(shape, size, as_float: bool, tr_full: bool, tm, seed: int = 0):
    """rows [B, Tr, P] int32, codes [B, P], mask [B, Tm, P] bool | None (tm: None, False = per pixel, True = per timestep), vocab, R."""
    (b, t, p), (r, g) = shape, size
    rng = np.random.default_rng([seed, b, t, p, r, g, int(as_float), int(tr_full), 2 if tm is None else int(tm)])
    vocab = make_vocab(rng, g)
    codes = make_codes(rng, vocab, (b, p), as_float)
    tr = t if tr_full else 1
    rows = rng.integers(0, r, size=(b, tr, p)).astype(np.int32)
    off = rng.random((b, tr, p)) < 0.03
    rows[off] = rng.choice(np.array([-1, r, r + 5], np.int32), size=int(off.sum()))
    mask = None if tm is None else rng.random((b, t if tm else 1, p)) < 0.7
    return dict(rows=rows, codes=codes, mask=mask, vocab=vocab, R=r, T=t)


def contingency(rows, codes, mask, vocab, R, T=None):
    """-> (table int64 [R, G], unmatched, rejected) of rows [B, Tr, P], codes [B, P], mask [B, Tm, P] | None."""
    b, tr, p = rows.shape
    t = T if T is not None else max(tr, 1 if mask is None else mask.shape[1])
    on = np.ones((b, t, p), bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (b, t, p))
    valid, col = lookup(codes, vocab)
    valid, col = np.broadcast_to(valid[:, None], (b, t, p)), np.broadcast_to(col[:, None], (b, t, p))
    lab = np.broadcast_to(rows, (b, t, p)).astype(np.int64)
    live = on & valid
    unmatched = int((live & (col < 0)).sum())
    live = live & (col >= 0)
    bad = (lab < 0) | (lab >= R)
    rejected = int((live & bad).sum())
    live = live & ~bad
    table = np.zeros((R, len(vocab)), np.int64)
    np.add.at(table, (lab[live], col[live]), 1)
    return table, unmatched, rejected


# tables for the clustering metrics [clusters, EVT classes]; the golden holds what the reference's compute_metrics (sklearn) gives for
# the label pairs they expand to
def metric_table(name: str):
    """-> (table int64 [R, G], EVT codes int32 [G])."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "a":                                                              # 20 clusters x 15 classes with structure
        t = rng.poisson(2.0, size=(20, 15)) + 40 * (rng.random((20, 15)) < 0.08)
    elif name == "b":                                                            # 50 x 300, sparse
        t = rng.poisson(0.3, size=(50, 300)) * rng.integers(1, 9, size=(50, 300))
    elif name == "one_cluster":
        t = rng.integers(1, 30, size=(1, 7))
    elif name == "one_class":
        t = rng.integers(1, 30, size=(6, 1))
    elif name == "single_pixel":
        t = np.ones((1, 1))
    elif name == "diagonal":
        t = np.diag([5, 11, 2])
    elif name == "empty_rows":                                                   # clusters and classes without a pixel
        t = rng.poisson(1.5, size=(6, 5))
        t[2] = 0
        t[:, 3] = 0
    else:
        raise KeyError(name)
    t = np.asarray(t, np.int64)
    return t, make_vocab(rng, t.shape[1])


METRIC_TABLES = ["a", "b", "one_cluster", "one_class", "single_pixel", "diagonal", "empty_rows"]
METRIC_KEYS = ["nmi", "homogeneity", "completeness", "v_measure", "purity", "n_pixels_metrics"]


def expand_table(table, codes, seed: int = 0):
    """-> (cluster labels int32 [n], EVT codes int32 [n]): one pair per count, shuffled."""
    r, c = np.nonzero(table)
    reps = table[r, c]
    cl, ev = np.repeat(r, reps).astype(np.int32), np.repeat(np.asarray(codes)[c], reps).astype(np.int32)
    perm = np.random.default_rng(seed).permutation(len(cl))
    return cl[perm], ev[perm]


# ---------------------------------------------------------------------------------------------------------------------------------
# grouped moments
# ---------------------------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1, 1, 1), (1, 1, 65, 12), (2, 5, 300, 12), (1, 15, 130, 64), (1, 3, 70, 128)]      # (B, T, P, D)
MOMENT_GROUPS = [1, 20, 127, 300]


def moment_case(shape, g: int, shift: float = 0.0, as_float: bool = False, per_step_mask: bool = False, seed: int = 0):
    """X [B, T, P, D] float32 = class centre + pixel offset + temporal noise (+ shift), codes [B, P], mask [B, Tm, P] bool, vocab [g].
    The last code of the vocabulary has no pixel (an empty class), and with g >= 3 and P >= 8 the one before it exactly one."""
    b, t, p, d = shape
    rng = np.random.default_rng([seed, b, t, p, d, g, int(as_float), int(per_step_mask)])
    vocab = make_vocab(rng, g)
    usable = vocab[:-1] if g >= 2 else vocab
    lone = g >= 3 and b * p >= 8
    if lone:
        usable = usable[:-1]
    codes = make_codes(rng, usable, (b, p), as_float, junk=0.1 if b * p >= 8 else 0.0, full=vocab)
    mask = rng.random((b, t if per_step_mask else 1, p)) < 0.8 if b * p >= 8 else np.ones((b, 1, p), bool)
    centre = rng.normal(0.0, 1.0, size=(g, d))
    if lone:
        bi, pi = divmod(3, p)
        codes[bi, pi] = vocab[-2]
        mask[bi, :, pi] = True
        centre[-2] = 3.0                                                         # the lone row sits clear of the pivot in every column
    _, col = lookup(codes, vocab)
    x = centre[np.maximum(col, 0)][:, None] + rng.normal(0.0, 0.5, size=(b, 1, p, d)) + rng.normal(0.0, 0.3, size=(b, t, p, d))
    return dict(X=(x + shift).astype(np.float32), codes=codes, mask=mask, vocab=vocab)


def _live(codes, mask, vocab, b, t, p):
    """-> (live bool [B, T, P], column [B, T, P], unmatched count) over observations."""
    on = np.ones((b, t, p), bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (b, t, p))
    valid, col = lookup(codes, vocab)
    valid, col = np.broadcast_to(valid[:, None], (b, t, p)), np.broadcast_to(col[:, None], (b, t, p))
    return on & valid & (col >= 0), col, int((on & valid & (col < 0)).sum())


def _terms(x, codes, mask, vocab, pivot, temporal: bool):
    """The float64 rows a group adds and the terms of their bounds -> (col [n], v1, v2, vw | None, a1, a2, aw | None, T, unmatched)."""
    x = np.asarray(x)
    b, t, p, d = x.shape
    y = x.astype(np.float64) - np.asarray(pivot, np.float32).astype(np.float64)
    if not temporal:
        live, col, unm = _live(codes, mask, vocab, b, t, p)
        v = y[live]
        return col[live], v, v * v, None, np.abs(v), v * v, None, 0, unm
    live, col, unm = _live(codes, mask, vocab, b, 1, p)
    live, col = live[:, 0], col[:, 0]
    yl = np.transpose(y, (0, 2, 1, 3))[live]                                     # [n, T, D]
    mu = yl.mean(axis=1)
    dt = yl - mu[:, None]
    w = (dt * dt).mean(axis=1)
    a = np.abs(yl).mean(axis=1)
    return col[live], mu, mu * mu, w, a, 2.0 * a * a, (dt * dt + 2.0 * np.abs(dt) * np.abs(yl)).mean(axis=1), t, unm


def _by_group(col, v, g):
    out = np.zeros((g, v.shape[1]))
    np.add.at(out, col, v)
    return out


def moments(x, codes, mask, vocab, pivot, temporal: bool = False):
    """Float64 restatement about the float32 pivot -> dict(count int64 [G], S1, S2 [G, D], SW [G, D] | None, unmatched)."""
    col, v1, v2, vw, _, _, _, _, unm = _terms(x, codes, mask, vocab, pivot, temporal)
    g = len(vocab)
    return dict(count=np.bincount(col, minlength=g).astype(np.int64), S1=_by_group(col, v1, g), S2=_by_group(col, v2, g),
                SW=None if vw is None else _by_group(col, vw, g), unmatched=unm)


def sum_bounds(x, codes, mask, vocab, pivot, temporal: bool = False):
    """(n + T + 8) u sum |t_i| per (group, column) -> dict(S1, S2, SW | None); see the module docstring for the terms."""
    col, _, _, _, a1, a2, aw, t, _ = _terms(x, codes, mask, vocab, pivot, temporal)
    g = len(vocab)
    f = (np.bincount(col, minlength=g) + t + 8)[:, None] * U32
    return dict(S1=f * _by_group(col, a1, g), S2=f * _by_group(col, a2, g), SW=None if aw is None else f * _by_group(col, aw, g))


def assert_spread(x, codes, mask, vocab, pivot, temporal: bool = False):
    """Every class with two rows or more has a standard deviation of at least 1e-2 of its root mean square about the pivot."""
    m = moments(x, codes, mask, vocab, pivot, temporal)
    n = np.maximum(m["count"], 1)[:, None]
    var = m["S2"] / n - (m["S1"] / n) ** 2
    ok = (np.sqrt(np.maximum(var, 0.0)) >= 1e-2 * np.sqrt(m["S2"] / n)) | (m["count"] < 2)[:, None]
    assert ok.all(), "a class's standard deviation is below 1e-2 of its spread about the pivot"


# ---- first-order propagation, doubled ------------------------------------------------------------------------------------------------
def propagate_mean(n, d1):
    return 2.0 * d1 / n


def _dvar(n, s1, d1, d2):
    return d2 / n + 2.0 * np.abs(s1 / n) * d1 / n


def propagate_std(n, s1, s2, d1, d2):
    dv = 2.0 * _dvar(n, s1, d1, d2)
    std = np.sqrt(np.maximum(s2 / n - (s1 / n) ** 2, 0.0))
    return np.where(std * std > dv, dv / np.maximum(std, 1e-300), np.sqrt(dv))


def propagate_temporal_frac(n, s1, s2, sw, d1, d2, dw):
    within, between = sw / n, np.maximum(s2 / n - (s1 / n) ** 2, 0.0)
    total = np.maximum(within + between, 1e-12)
    return 2.0 * (between * dw / n + within * _dvar(n, s1, d1, d2)) / total ** 2


def propagate_r2(n, pivot_e, s1e, s2e, d1e, d2e, s1t, s2t, d1t, d2t):
    """R^2 = 1 - ssres / sstot from the moments of [pred - target | target]; the float32 subtraction pred - target moves ssres by
    2 u ssres more."""
    ssres = s2e + 2.0 * pivot_e * s1e + n * pivot_e ** 2
    sstot = np.maximum(s2t - s1t ** 2 / n, 1e-12)
    dres = d2e + 2.0 * np.abs(pivot_e) * d1e + 2.0 * U32 * ssres
    dtot = d2t + 2.0 * np.abs(s1t / n) * d1t
    return 2.0 * (dres / sstot + ssres * dtot / sstot ** 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the end-to-end case: model-shaped tensors, channels-last
# ---------------------------------------------------------------------------------------------------------------------------------
E2E = dict(b=2, t=5, h=16, w=16, d_phase=12, c=5, g=8, seed=41)


def e2e_inputs():
    """gamma [2, 16, 16, 12], z_phase [2, 5, 16, 16, 12], pred and target [2, 5, 16, 16, 5] float32, codes [2, 16, 16] float32 (as the
    reference's evt_grid), mask [2, 16, 16] bool, vocab [8]: its last class is empty, the one before it has one pixel."""
    c = E2E
    rng = np.random.default_rng(c["seed"])
    b, t, h, w, d, k, g = c["b"], c["t"], c["h"], c["w"], c["d_phase"], c["c"], c["g"]
    vocab = make_vocab(rng, g)
    codes = make_codes(rng, vocab[:-2], (b, h * w), True, coherent=True, junk=0.06, full=vocab)
    codes = np.where(np.isfinite(codes) & (codes > 0), np.floor(codes), codes).astype(np.float32)   # the reference's grid holds whole codes
    mask = rng.random((b, h * w)) < 0.8
    codes[0, 5], mask[0, 5] = vocab[-2], True
    _, col = lookup(codes, vocab)
    cg, cz = rng.normal(1.0, 0.4, size=(g, d)), rng.normal(0.0, 1.0, size=(g, d))
    cg[-2] = cz[-2] = 3.0
    cc = np.maximum(col, 0)
    gamma = cg[cc] + rng.normal(0.0, 0.3, size=(b, h * w, d))
    z = cz[cc][:, None] + rng.normal(0.0, 0.5, size=(b, 1, h * w, d)) + rng.normal(0.0, 0.3, size=(b, t, h * w, d))
    target = rng.normal(0.0, 1.0, size=(g, k))[cc][:, None] + rng.normal(0.0, 0.6, size=(b, t, h * w, k))
    pred = target + rng.normal(0.0, 0.35, size=(b, t, h * w, k))
    f = np.float32
    out = dict(gamma=gamma.astype(f).reshape(b, h, w, d), z_phase=z.astype(f).reshape(b, t, h, w, d), pred=pred.astype(f).reshape(b, t, h, w, k),
               target=target.astype(f).reshape(b, t, h, w, k), codes=codes.reshape(b, h, w), mask=mask.reshape(b, h, w), vocab=vocab)
    m3 = mask.reshape(b, 1, h * w)
    for x, temporal in ((out["gamma"].reshape(b, 1, h * w, d), False), (out["z_phase"].reshape(b, t, h * w, d), True),
                        (out["target"].reshape(b, t, h * w, k), False)):          # what a standard deviation or a variance is taken of
        zero = moments(x, codes, m3, vocab, np.zeros(x.shape[-1], f), temporal)
        assert_spread(x, codes, m3, vocab, (zero["S1"].sum(0) / zero["count"].sum()).astype(f), temporal)
    return out


def e2e_flat(inp):
    """The valid pixels as the reference's process_batch hands them to its accumulators -> (codes int32 [N], gamma f64 [N, d],
    z_phase f64 [N, d, T], pred f64 [N T, C], target f64 [N T, C], codes per observation int32 [N T]) with observations t-major."""
    c = inp["codes"].reshape(-1)
    sel = inp["mask"].reshape(-1) & np.isfinite(c) & (c > 0)
    b, t, h, w, d = inp["z_phase"].shape
    sel2 = sel.reshape(b, h * w)
    ev = c[sel].astype(np.int32)
    gm = inp["gamma"].reshape(-1, d)[sel].astype(np.float64)
    zp = np.transpose(inp["z_phase"].reshape(b, t, h * w, d), (0, 2, 3, 1))[sel2].astype(np.float64)      # [N, d, T]
    k = inp["pred"].shape[-1]
    pr = np.transpose(inp["pred"].reshape(b, t, h * w, k), (1, 0, 2, 3))[:, sel2].astype(np.float64)       # [T, N, C]
    tg = np.transpose(inp["target"].reshape(b, t, h * w, k), (1, 0, 2, 3))[:, sel2].astype(np.float64)
    return ev, gm, zp, pr.reshape(-1, k), tg.reshape(-1, k), np.tile(ev, t)


def evt_stats(inp):
    """The reference's EvtAccumulators quantities restated with its own formulas in float64 -> {code: dict(n, mean, std, frac, r2)}."""
    ev, gm, zp, pr, tg, evo = e2e_flat(inp)
    out = {}
    for e in np.unique(ev):
        i, j = ev == e, evo == e
        n, m = int(i.sum()), int(j.sum())
        mean = gm[i].sum(0) / n
        var = np.maximum((gm[i] ** 2).sum(0) / n - mean ** 2, 0.0)
        pm = zp[i].mean(axis=2)
        within = zp[i].var(axis=2).sum(0) / n
        mm = pm.sum(0) / n
        between = np.maximum((pm ** 2).sum(0) / n - mm ** 2, 0.0)
        mt = tg[j].sum(0) / m
        sstot = np.maximum((tg[j] ** 2).sum(0) - m * mt ** 2, 1e-12)
        out[int(e)] = dict(n=n, mean=mean, std=np.sqrt(var), frac=within / np.maximum(within + between, 1e-12),
                           r2=1.0 - ((pr[j] - tg[j]) ** 2).sum(0) / sstot)
    return out
