"""Cases, inputs, the numpy restatement and the one derived bound for the exact quantiles (test_cpu_quantile.py, test_gpu_quantile.py).

Inputs are regenerated from numpy's default_rng, never stored; tests/golden/quantile_recovery.npz (tests/golden/make_quantile_golden.py)
holds what the reference's own EvtReservoir and save_csv gave for `recovery_inputs`, and a checksum of the inputs.  No product code is
imported here; numpy only.

Restatement.  Per cell: np.sort of the float32 values (-0.0 folded into +0.0 first, as the kernel's key does), then for a probability q
and n values v = (n - 1) q in float64, k = floor(v), t = v - k, lo = x[k], hi = x[min(k + 1, n - 1)], and the quantile
lo + (hi - lo) t for t < 0.5 else hi - (hi - lo) (1 - t) in float64.  test_cpu_quantile.py holds this to exact equality with
np.percentile of the float64 cast, so the GPU is held to exact equality with it: there is no tolerance anywhere but below.

The reference against the restatement.  save_csv calls np.percentile and np.median on float32 arrays, and numpy then works in float32
throughout.  With u = 2^-24 and ulp(v) the float32 spacing at v:
  the virtual index n q + (1 - q) - 1 takes five roundings (q = 25 / 100, n q, 1 - q, the sum, the - 1) of quantities of at most
  v + 1 <= 2 max(v, 1), each at most ulp(max(v, 1)): |v32 - v| <= dv = 5 ulp(max(v, 1)); its floor and fraction are then exact;
  the quantile is continuous and piecewise linear in v, with slope x[i + 1] - x[i] on segment i, so moving v by dv moves it by at most
  dv times the widest gap among the segments within ceil(dv) + 1 of k: with t within dv of 0 or 1 the shifted index lies in the
  neighbouring segment, whose slope is that segment's gap and not |hi - lo| (|hi - lo| alone would be wrong exactly there);
  the float32 lerp rounds hi - lo, the product and the sum: 2 u |hi - lo| + u max(|lo|, |hi|); np.median's mean of two float32 values
  rounds once, u max(|lo|, |hi|), which the same term covers.
`reference_bound` adds these up.  It is derived, not measured; the golden's report records how much of it the fixture uses.
"""
from __future__ import annotations

import numpy as np

import strata_cases as SC

U32 = 2.0 ** -24
PROBS7 = [0.0, 0.02, 0.25, 0.5, 0.75, 0.98, 1.0]
QUARTILES = [0.25, 0.5, 0.75]
LDS_WINDOW = 48                                                                  # slots (cell, column[, rank]) of one LDS window of the kernel
LDS_WINDOWS = 4                                                                  # later passes count in LDS up to this many windows


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def fold(x) -> np.ndarray:
    """float32 with -0.0 replaced by +0.0."""
    x = np.asarray(x, np.float32)
    return np.where(x == 0, np.float32(0.0), x)


def ranks(n: int, q: float):
    """-> (k, min(k + 1, n - 1), t) of v = (n - 1) q in float64."""
    v = np.float64(n - 1) * np.float64(q)
    k = int(np.floor(v))
    return k, min(k + 1, n - 1), float(v - np.floor(v))


def lerp(lo, hi, t):
    lo, hi, t = np.asarray(lo, np.float64), np.asarray(hi, np.float64), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(t < 0.5, lo + (hi - lo) * t, hi - (hi - lo) * (1.0 - t))


def order_statistics(x, probs):
    """x float32 [n] -> (lo float32 [Q], hi float32 [Q], t float64 [Q]); NaN, NaN, 0 for n = 0."""
    xs = np.sort(fold(x))
    nq = len(probs)
    if xs.size == 0:
        return np.full(nq, np.nan, np.float32), np.full(nq, np.nan, np.float32), np.zeros(nq)
    r = [ranks(xs.size, q) for q in probs]
    return xs[[a for a, _, _ in r]], xs[[b for _, b, _ in r]], np.asarray([t for _, _, t in r])


def quantiles(x, probs) -> np.ndarray:
    """float64 [Q]."""
    return lerp(*order_statistics(x, probs))


# ---------------------------------------------------------------------------------------------------------------------------------
# key order: one cell
# ---------------------------------------------------------------------------------------------------------------------------------
KEY_ORDER_N = [1, 2, 3, 64, 65, 4097]


def _from_key(keys) -> np.ndarray:
    """The float32 of a monotone uint32 key (the inverse of: flip every bit of a negative, set the sign bit of any other)."""
    k = np.asarray(keys, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def key_order_pool() -> np.ndarray:
    """Negatives, positives, +-0, denormals, +-FLT_MAX, and runs of three ties on either side of a boundary of every 8-bit digit."""
    fmax, fmin, den = np.finfo(np.float32).max, np.finfo(np.float32).tiny, np.float32(1e-45)
    special = np.array([0.0, -0.0, 0.0, -0.0, den, -den, fmin - den, -(fmin - den), fmin, -fmin, fmax, -fmax, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38,
                        1e-30, -1e-30, 255.0, 256.0, 65535.0, 65536.0], np.float32)
    edges = []
    for top in (0xC0000000, 0x40000000, 0xA5000000, 0x12000000):                   # two positive and two negative top digits
        for shift in (24, 16, 8):                                                # key b - 1 and key b differ in the digit at `shift` and all below
            b = top + ((1 << shift) if shift < 24 else 0)
            edges += [b - 1, b]
    edges = np.asarray(edges, np.uint64).astype(np.uint32)
    vals = _from_key(edges)
    vals = vals[np.isfinite(vals)]
    return np.concatenate([special, np.repeat(vals, 3)]).astype(np.float32)


def key_order_values(n: int) -> np.ndarray:
    rng = np.random.default_rng([17, n])
    pool = key_order_pool()
    if n <= 3:
        return np.array([-0.0, np.finfo(np.float32).max, -np.float32(1e-45)], np.float32)[:n]
    if n <= pool.size:                                                           # the first 12: +-0, denormals, +-FLT_MIN, +-FLT_MAX always
        return rng.permutation(np.concatenate([pool[:12], rng.permutation(pool[12:])[:n - 12]]))
    extra = n - pool.size
    more = np.concatenate([rng.choice(pool, extra // 2), (rng.normal(size=extra - extra // 2) * 10.0 ** rng.integers(-30, 30, size=extra - extra // 2))])
    return rng.permutation(np.concatenate([pool, more.astype(np.float32)])).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# grouped
# ---------------------------------------------------------------------------------------------------------------------------------
def grouped_case(b: int, t: int, p: int, g: int, r: int, d: int, as_float: bool = False, per_step_mask: bool = False, per_step_rows: bool = True,
                 nonfinite: bool = True, seed: int = 0):
    """values [B, T, P, D] float32, codes [B, P] with junk, rows [B, Tr, P] int32 (None for r = 1) with labels outside [0, r), mask
    [B, Tm, P] bool, vocab [g].  With g >= 3 the last code has no pixel (empty cells), the one before it a single pixel (a cell of T elements, one
    at T = 1), and with g >= 4 the first code holds all-equal values; a few rows carry a NaN or an inf in one column."""
    rng = np.random.default_rng([seed, b, t, p, g, r, d, int(as_float), int(per_step_mask)])
    vocab = SC.make_vocab(rng, g)
    usable = vocab[:-2] if g >= 3 else vocab
    codes = SC.make_codes(rng, usable, (b, p), as_float, junk=0.1, full=vocab)
    mask = rng.random((b, t if per_step_mask else 1, p)) < 0.8
    if g >= 3:
        codes[0, 3] = vocab[-2]
        mask[0, :, 3] = True
    rows = None
    if r > 1:
        rows = rng.integers(0, r, size=(b, t if per_step_rows else 1, p)).astype(np.int32)
        off = rng.random(rows.shape) < 0.03
        rows[off] = rng.choice(np.array([-1, r, r + 5], np.int32), size=int(off.sum()))
        if g >= 3:
            rows[0, :, 3] = r - 1
    x = (rng.normal(0.0, 1.0, size=(b, t, p, d)) * 10.0 ** rng.integers(-2, 3, size=(1, 1, 1, d))).astype(np.float32)
    x[rng.random(x.shape) < 0.05] = 0.25                                         # ties
    _, col = SC.lookup(codes, vocab)
    if g >= 4:
        x[np.broadcast_to((col == 0)[:, None], (b, t, p))] = -7.5                 # an all-equal class
    if nonfinite:
        bad = rng.random((b, t, p)) < 0.02
        x[bad, rng.integers(0, d, size=int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), size=int(bad.sum()))
    if g >= 3:
        x[0, :, 3] = 1.25                                                        # the single pixel stays finite
    return dict(X=x, codes=codes, rows=rows, mask=mask, vocab=vocab, R=r)


def grouped(x, codes, rows, mask, vocab, R, probs):
    """-> dict(count int64 [R, G], lo, hi float32 [R, G, D, Q], frac float64 [R, G, Q], unmatched, rejected, nonfinite, records), the
    tests in the kernel's order: mask, invalid code, code outside the vocabulary, row label outside [0, R), a value that is not finite."""
    x = np.asarray(x, np.float32)
    b, t, p, d = x.shape
    g, nq = len(vocab), len(probs)
    on = np.ones((b, t, p), bool) if mask is None else np.broadcast_to(np.asarray(mask) != 0, (b, t, p))
    valid, col = SC.lookup(codes, vocab)
    valid, col = np.broadcast_to(valid[:, None], (b, t, p)), np.broadcast_to(col[:, None], (b, t, p))
    live = on & valid
    unmatched = int((live & (col < 0)).sum())
    live = live & (col >= 0)
    lab = np.zeros((b, t, p), np.int64) if rows is None else np.broadcast_to(rows, (b, t, p)).astype(np.int64)
    bad = (lab < 0) | (lab >= R)
    rejected = int((live & bad).sum())
    live = live & ~bad
    fin = np.isfinite(x).all(axis=-1)
    nonfinite = int((live & ~fin).sum())
    live = live & fin
    cell = lab * g + col
    count = np.zeros((R, g), np.int64)
    lo, hi = np.full((R, g, d, nq), np.nan, np.float32), np.full((R, g, d, nq), np.nan, np.float32)
    frac = np.zeros((R, g, nq))
    xs, cs = x[live], cell[live]
    order = np.argsort(cs, kind="stable")
    xs, cs = xs[order], cs[order]
    starts = np.searchsorted(cs, np.arange(R * g + 1))
    for c in range(R * g):
        rows_c = xs[starts[c]:starts[c + 1]]
        count[c // g, c % g] = len(rows_c)
        for k in range(d):
            lo[c // g, c % g, k], hi[c // g, c % g, k], fr = order_statistics(rows_c[:, k], probs)
            frac[c // g, c % g] = fr
    return dict(count=count, lo=lo, hi=hi, frac=frac, unmatched=unmatched, rejected=rejected, nonfinite=nonfinite, records=int(live.sum()))


def same_bits(a, b) -> bool:
    """Equal as bit patterns but for the payload of a NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------------------------
# recovery curves against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
RECOVERY_BINS = [(0, 1), (1, 2), (2, 3), (3, 5), (5, 8), (8, 13), (13, 20), (20, 31)]     # phase_recovery_curves.py, right-exclusive
RECOVERY = dict(b=2, t=5, h=12, w=12, g=6, max_ysfc=32.0, seed=23)          # 31 and 32 years count but fall into no bin
RECOVERY_COLUMNS = ["pred_nbr_q25", "pred_nbr_median", "pred_nbr_q75", "obs_nbr_median"]


def recovery_inputs():
    """evt_grid [2, 12, 12] float32 with junk, ysfc [2, 5, 12, 12] in years (whole numbers from -2 to 34, some NaN), pred_nbr and obs_nbr
    [2, 5, 12, 12] float32, mask [2, 5, 12, 12] bool, vocab [6] whose last code has no pixel."""
    c = RECOVERY
    rng = np.random.default_rng(c["seed"])
    b, t, h, w, g = c["b"], c["t"], c["h"], c["w"], c["g"]
    vocab = SC.make_vocab(rng, g)
    codes = SC.make_codes(rng, vocab[:-1], (b, h * w), True, coherent=True, junk=0.08, full=vocab)
    codes = np.where(np.isfinite(codes) & (codes > 0), np.floor(codes), codes).astype(np.float32)
    ysfc = rng.integers(-2, 35, size=(b, t, h, w)).astype(np.float32)
    ysfc[rng.random(ysfc.shape) < 0.04] = np.nan
    obs = rng.normal(0.0, 1.0, size=(b, t, h, w)) + 0.03 * np.nan_to_num(ysfc)
    pred = obs + rng.normal(0.0, 0.4, size=(b, t, h, w))
    pred[rng.random(pred.shape) < 0.1] = 0.5                                     # ties
    mask = rng.random((b, t, h, w)) < 0.85
    return dict(evt_grid=codes.reshape(b, h, w), ysfc=ysfc, pred_nbr=pred.astype(np.float32), obs_nbr=obs.astype(np.float32), mask=mask, vocab=vocab)


def recovery_flat(inp):
    """What the reference's process_batch hands to EvtReservoir.add_batch, one call per (sample, timestep) ->
    [(evt int32 [n], ysfc, pred, obs float32 [n])]."""
    b, t, h, w = inp["ysfc"].shape
    out = []
    for i in range(b):
        grid = inp["evt_grid"][i].reshape(-1)
        ok = np.isfinite(grid) & (grid > 0)
        evt = np.where(ok, grid, 0).astype(np.int32)
        for s in range(t):
            y = inp["ysfc"][i, s].reshape(-1)
            with np.errstate(invalid="ignore"):
                m = ok & inp["mask"][i, s].reshape(-1) & (y >= 0) & (y <= RECOVERY["max_ysfc"])
            out.append((evt[m], y[m], inp["pred_nbr"][i, s].reshape(-1)[m], inp["obs_nbr"][i, s].reshape(-1)[m]))
    return out


def reference_bound(xs: np.ndarray, q: float) -> float:
    """How far float32 np.percentile(xs, 100 q) may lie from the float64 restatement (module docstring); xs sorted float32."""
    n = xs.size
    k, k1, _ = ranks(n, q)
    v = (n - 1) * q
    dv = 5.0 * float(np.spacing(np.float32(max(v, 1.0))))
    reach = int(np.ceil(dv)) + 1
    seg = xs[max(k - reach, 0):min(k1 + reach, n - 1) + 1].astype(np.float64)
    gap = float(np.max(np.diff(seg))) if seg.size > 1 else 0.0
    lo, hi = float(xs[k]), float(xs[k1])
    return dv * gap + U32 * (2.0 * abs(hi - lo) + max(abs(lo), abs(hi))) + 4.0 * np.finfo(np.float64).eps * max(abs(lo), abs(hi))


def recovery_table(inp, top_codes):
    """The restatement of save_csv -> (rows [dict(evt_code, bin, n_samples, the four RECOVERY_COLUMNS)], bounds [dict of the four]), in
    the order of top_codes and bins, empty bins left out; n_seen {code: observations}."""
    flat = recovery_flat(inp)
    evt = np.concatenate([f[0] for f in flat])
    y, pred, obs = (np.concatenate([f[i] for f in flat]) for i in (1, 2, 3))
    rows, bounds = [], []
    for code in top_codes:
        for r, (a, z) in enumerate(RECOVERY_BINS):
            sel = (evt == code) & (y >= a) & (y < z)
            if not sel.any():
                continue
            ps, os_ = np.sort(fold(pred[sel])), np.sort(fold(obs[sel]))
            qp = quantiles(ps, QUARTILES)
            rows.append(dict(evt_code=int(code), bin=r, n_samples=int(sel.sum()), pred_nbr_q25=float(qp[0]), pred_nbr_median=float(qp[1]),
                             pred_nbr_q75=float(qp[2]), obs_nbr_median=float(quantiles(os_, [0.5])[0])))
            bounds.append(dict(pred_nbr_q25=reference_bound(ps, 0.25), pred_nbr_median=reference_bound(ps, 0.5), pred_nbr_q75=reference_bound(ps, 0.75),
                               obs_nbr_median=reference_bound(os_, 0.5)))
    n_seen = {int(c): int((evt == c).sum()) for c in np.unique(evt)}
    return rows, bounds, n_seen
