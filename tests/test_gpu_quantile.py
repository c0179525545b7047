"""GPU tests of the exact quantiles (csrc/quantile.hip, frl_hip/quantiles.py, strata.RecoveryCurves) against the numpy restatement of
tests/quantile_cases.py.

Everything the kernels return is an integer or one of the input's own float32 values, so counts, counters and both bracketing order
statistics are held to exact (bit) equality, and the interpolated quantiles, formed in float64 from them, to exact equality as well.  The
one tolerance is against the reference's float32 np.percentile (tests/golden/quantile_recovery.npz): quantile_cases.reference_bound,
derived there and asserted for the restatement in test_cpu_quantile.py.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import quantile_cases as QC
import strata_cases as SC
from frl_hip import _lib, ops, quantiles as Q, strata as S
from frl_hip.quantiles import GroupedQuantiles, masked_quantiles, summary_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---- 1. key order: one cell ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", QC.KEY_ORDER_N)
def test_key_order_brackets_are_bit_exact(n):
    x = QC.key_order_values(n)
    if n >= 64:
        assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any() and (np.abs(x) == np.finfo(np.float32).max).any()
        assert ((x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)).any() and len(np.unique(x)) < n
    count, lo, hi, frac = ops.quantile_select(QC.PROBS7, 1, 1, x=_t(x).view(-1, 1))
    wlo, whi, wt = QC.order_statistics(x, QC.PROBS7)
    assert int(count.item()) == n
    assert QC.same_bits(lo.cpu().numpy()[0, 0], wlo) and QC.same_bits(hi.cpu().numpy()[0, 0], whi)
    assert np.array_equal(frac.cpu().numpy()[0], wt)
    got = masked_quantiles(_t(x), QC.PROBS7)
    assert got.dtype == torch.float64 and got.is_cuda and np.array_equal(got.cpu().numpy(), QC.quantiles(x, QC.PROBS7))
    assert np.array_equal(got.cpu().numpy(), np.percentile(x.astype(np.float64), [100.0 * q for q in QC.PROBS7]))


@pytest.mark.parametrize("d,nq", [(1, 1), (4, 8), (16, 8)])                      # 2 Q D slots: one LDS window, two, and the sweep without windows
def test_masked_quantiles_columns_and_mask(d, nq):
    n = 4097
    assert (2 * nq * d <= QC.LDS_WINDOW, 2 * nq * d > QC.LDS_WINDOW * QC.LDS_WINDOWS) == ((True, False), (False, False), (False, True))[[1, 4, 16].index(d)]
    rng = np.random.default_rng([3, d])
    x = np.stack([rng.permutation(QC.key_order_values(n)) for _ in range(d)], axis=1)
    mask = rng.random(n) < 0.6
    probs = (QC.PROBS7 + [0.6])[:nq] if nq > 1 else [0.5]
    for m in (None, mask, np.zeros(n, bool)):
        got = masked_quantiles(_t(x), probs, None if m is None else _t(m)).cpu().numpy()
        assert got.shape == (d, nq)
        for k in range(d):
            want = QC.quantiles(x[:, k] if m is None else x[m, k], probs)
            assert np.array_equal(got[k], want, equal_nan=True), (k, got[k], want)
    one = masked_quantiles(_t(x[:, 0].copy()), probs[0], _t(mask))
    assert one.shape == (1,) and one.item() == QC.quantiles(x[mask, 0], probs[:1])[0]
    if d == 1:                                                                   # an unaligned view takes the scalar path: the same bits
        buf = _t(np.concatenate([[0.0], x[:, 0]]).astype(np.float32))
        assert torch.equal(masked_quantiles(buf[1:], probs), masked_quantiles(_t(x[:, 0].copy()), probs))


# ---- 2. grouped ----------------------------------------------------------------------------------------------------------------------
def _fit(c, gq, b0=0, b1=None):
    """Feeds samples [b0, b1) of a quantile_cases.grouped_case through GroupedQuantiles: values [B, T, P, 1, D], codes [B, P, 1], rows and
    mask per pixel [B, P, 1] or per timestep [B, T, P, 1]."""
    x = c["X"][b0:b1]
    b, t, p, d = x.shape

    def lay(a):
        if a is None:
            return None
        a = a[b0:b1]
        return a.reshape(b, p, 1) if a.shape[1] == 1 and t > 1 else a.reshape(b, a.shape[1], p, 1)
    return gq.partial_fit(_t(x.reshape(b, t, p, 1, d)), _t(c["codes"][b0:b1].reshape(b, p, 1)), _t(lay(c["rows"])), _t(lay(c["mask"])))


def _check(gq, c, probs, what):
    want = QC.grouped(c["X"], c["codes"], c["rows"], c["mask"], c["vocab"], c["R"], probs)
    lo, hi, frac = gq.order_statistics(probs)
    print(f"{what}: {want['records']} records, {want['unmatched']} unmatched, {want['rejected']} rejected, {want['nonfinite']} not finite")
    assert np.array_equal(gq.count_, want["count"]), f"{what}: counts differ"
    assert (gq.unmatched_, gq.rejected_, gq.nonfinite_, gq.dropped_) == (want["unmatched"], want["rejected"], want["nonfinite"], 0)
    assert QC.same_bits(lo, want["lo"]) and QC.same_bits(hi, want["hi"]), f"{what}: order statistics differ"
    assert np.array_equal(frac, want["frac"])
    assert np.array_equal(gq.quantiles(probs), QC.lerp(want["lo"], want["hi"], want["frac"][:, :, None, :]), equal_nan=True)
    return want


def _grouped_combos():
    out, i = [], 0
    for t in (1, 3):
        for g in (1, 3, 40):
            for r in (1, 8):
                for d in (1, 2, 16):
                    as_float, per_step = bool(i % 2), bool((i // 2) % 2)
                    out.append(pytest.param(t, g, r, d, as_float, per_step, id=f"T{t}-G{g}-R{r}-D{d}-{'f32' if as_float else 'i32'}-{'step' if per_step else 'pixel'}"))
                    i += 1
    return out


@pytest.mark.parametrize("t,g,r,d,as_float,per_step", _grouped_combos())
def test_grouped_is_exact(t, g, r, d, as_float, per_step):
    c = QC.grouped_case(2, t, 1000, g, r, d, as_float=as_float, per_step_mask=per_step, per_step_rows=not per_step or t == 1)
    probs = QC.PROBS7 if g == 3 else QC.QUARTILES
    want = _check(_fit(c, GroupedQuantiles(c["vocab"], d, n_rows=r, capacity=2 * t * 1000)), c, probs, "grouped")
    assert want["nonfinite"] > 0 and want["unmatched"] > 0 and (r == 1 or want["rejected"] > 0)
    if as_float:
        assert np.isnan(c["codes"]).any()
    if g >= 3:
        assert not want["count"][:, -1].any() and want["count"][r - 1, -2] == t == want["count"][:, -2].sum()      # empty cells; a cell of one pixel
    if g >= 4:
        filled = want["count"][:, 0] > 0
        assert filled.any() and np.all(want["lo"][filled, 0] == -7.5) and np.all(want["hi"][filled, 0] == -7.5)   # the all-equal class
    if (g, r, d) == (40, 8, 16):
        assert r * g * d > QC.LDS_WINDOW                                         # pass 1 walks windows


# ---- 3. streaming, permutation, grids ------------------------------------------------------------------------------------------------
def _bits(gq, probs):
    lo, hi, frac = gq.order_statistics(probs)
    return gq.count_.tobytes() + lo.tobytes() + hi.tobytes() + frac.tobytes()


@pytest.mark.parametrize("g,r,d", [(3, 1, 2), (40, 8, 2)])
def test_streaming_permutation_and_grids_give_identical_bits(g, r, d):
    c = QC.grouped_case(3, 3, 1000, g, r, d, as_float=True, per_step_mask=True, nonfinite=False, seed=1)
    probs = QC.PROBS7
    one = _fit(c, GroupedQuantiles(c["vocab"], d, n_rows=r, capacity=9000))
    _check(one, c, probs, "one call")
    three = GroupedQuantiles(c["vocab"], d, n_rows=r, capacity=9000)
    for b in range(3):
        _fit(c, three, b, b + 1)
    assert _bits(three, probs) == _bits(one, probs)
    assert (three.unmatched_, three.rejected_) == (one.unmatched_, one.rejected_)
    perm = np.random.default_rng(5).permutation(1000)
    pc = dict(c, X=c["X"][:, :, perm], codes=c["codes"][:, perm], rows=None if c["rows"] is None else c["rows"][:, :, perm], mask=c["mask"][:, :, perm])
    assert _bits(_fit(pc, GroupedQuantiles(c["vocab"], d, n_rows=r, capacity=9000)), probs) == _bits(one, probs)
    for workgroups in (1, 7, 0):
        assert _bits(_fit(c, GroupedQuantiles(c["vocab"], d, n_rows=r, capacity=9000, workgroups=workgroups)), probs) == _bits(one, probs)
    x = QC.key_order_values(4097)
    ref = masked_quantiles(_t(x), probs)
    for workgroups in (1, 7):
        assert torch.equal(masked_quantiles(_t(x), probs, workgroups=workgroups), ref)
    assert torch.equal(masked_quantiles(_t(np.random.default_rng(6).permutation(x)), probs), ref)


# ---- 4. capacity ---------------------------------------------------------------------------------------------------------------------
def test_capacity_full_and_one_short():
    c = QC.grouped_case(2, 3, 1000, 3, 8, 2, seed=2)
    want = QC.grouped(c["X"], c["codes"], c["rows"], c["mask"], c["vocab"], c["R"], QC.QUARTILES)
    full = _fit(c, GroupedQuantiles(c["vocab"], 2, n_rows=8, capacity=want["records"]))
    assert full.dropped_ == 0
    _check(full, c, QC.QUARTILES, "capacity = records")
    short = _fit(c, GroupedQuantiles(c["vocab"], 2, n_rows=8, capacity=want["records"] - 1))
    assert short.dropped_ == 1 and int(short.count_.sum()) == want["records"] - 1
    with pytest.raises(RuntimeError, match="did not fit"):
        short.quantiles(QC.QUARTILES)
    with pytest.raises(RuntimeError, match="did not fit"):
        short.order_statistics(QC.QUARTILES)


# ---- 5. beyond 2^24 ------------------------------------------------------------------------------------------------------------------
def test_masked_quantiles_beyond_2_to_24():
    n = 2 ** 24 + 3
    x = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11))
    got = masked_quantiles(x, QC.PROBS7).cpu().numpy()
    xs = torch.sort(x).values
    r = [QC.ranks(n, q) for q in QC.PROBS7]
    lo = xs[torch.tensor([a for a, _, _ in r], device=DEV)].cpu().numpy()
    hi = xs[torch.tensor([b for _, b, _ in r], device=DEV)].cpu().numpy()
    assert np.array_equal(got, QC.lerp(lo, hi, np.asarray([t for _, _, t in r])))


# ---- 6. the reference's call sites -----------------------------------------------------------------------------------------------------
def test_recovery_curves_table_matches_the_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "quantile_recovery.npz"))
    inp = QC.recovery_inputs()
    assert SC.checksum(*[inp[k] for k in ("evt_grid", "ysfc", "pred_nbr", "obs_nbr", "mask", "vocab")]) == int(fx["checksum"])
    vocab = [int(v) for v in inp["vocab"]]
    rc = S.RecoveryCurves(vocab, max_ysfc=QC.RECOVERY["max_ysfc"], capacity=2048)
    for i in range(2):                                                           # sample by sample, as the reference streams
        rc.add(*[_t(inp[k][i:i + 1]) for k in ("evt_grid", "ysfc", "pred_nbr", "obs_nbr", "mask")])
    rows, bounds, n_seen = QC.recovery_table(inp, vocab)
    table = rc.table(vocab)
    assert len(table) == len(rows) == len(fx["evt_code"])
    in_vocab = {c: n for c, n in n_seen.items() if c in vocab}
    assert rc.pixel_counts() == in_vocab and all(rc.n_seen(c) == n for c, n in in_vocab.items()) and rc.n_seen(vocab[-1]) == 0
    assert rc.unmatched_ == sum(n for c, n in n_seen.items() if c not in vocab) and rc.dropped_ == 0 and rc.nonfinite_ == 0
    assert rc.top_codes(2) == [c for c, _ in sorted(in_vocab.items(), key=lambda cv: (-cv[1], cv[0]))[:2]]
    worst = 0.0
    for i, (got, want, bound) in enumerate(zip(table, rows, bounds)):
        assert (got["evt_code"], got["ysfc_bin"], got["n_samples"]) == (want["evt_code"], S.RECOVERY_YSFC_BIN_LABELS[want["bin"]], want["n_samples"])
        assert (got["evt_code"], got["n_samples"]) == (int(fx["evt_code"][i]), int(fx["n_samples"][i])) and want["bin"] == int(fx["bin"][i])
        for k in QC.RECOVERY_COLUMNS:
            assert got[k] == want[k], (i, k, got[k], want[k])                    # the restatement: exactly
            err = abs(got[k] - fx[k][i])                                         # the reference's float32 percentile: within the derived bound
            worst = max(worst, err / bound[k])
            assert err <= bound[k], (i, k, err, bound[k])
    print(f"largest distance from the reference at {worst:.4f} of the derived bound")
    assert rc.table([vocab[0]]) == [r for r in table if r["evt_code"] == vocab[0]]


def test_recovery_curves_bins_that_do_not_start_at_zero():
    """An observation below the first edge or at or beyond the last falls into no bin and still counts in n_seen; asking for the counts
    first leaves the select that table() needs."""
    rng = np.random.default_rng(13)
    ysfc = rng.integers(-1, 12, size=(1, 4, 50)).astype(np.float32)
    pred, obs = rng.normal(size=(2, 1, 4, 50)).astype(np.float32)
    evt = np.full((1, 50), 7, np.int32)
    rc = S.RecoveryCurves([7, 9], bins=[(2, 5), (5, 9)], max_ysfc=10.0, capacity=256)
    rc.add(_t(evt), _t(ysfc), _t(pred), _t(obs))
    keep = (ysfc >= 0) & (ysfc <= 10.0)
    assert rc.n_seen(7) == int(keep.sum()) and rc.top_codes(5) == [7] and rc._q.rejected_ == 0
    held = rc._q._host
    table = rc.table([7, 9])
    assert rc._q._host is held                                                   # one select for both
    assert [r["ysfc_bin"] for r in table] == ["2-5", "5-9"]
    for r, (a, z) in zip(table, [(2, 5), (5, 9)]):
        sel = keep & (ysfc >= a) & (ysfc < z)
        qp = QC.quantiles(pred[sel], QC.QUARTILES)
        assert r["n_samples"] == int(sel.sum()) and (r["pred_nbr_q25"], r["pred_nbr_median"], r["pred_nbr_q75"]) == tuple(qp)
        assert r["obs_nbr_median"] == QC.quantiles(obs[sel], [0.5])[0]
    assert sum(r["n_samples"] for r in table) < rc.n_seen(7)


def test_summary_stats_quantiles_are_exact():
    rng = np.random.default_rng(9)
    parts = [rng.random(s).astype(np.float32) for s in ((3, 700), (1234,), (5, 5, 41))]
    parts[1][::3] = 1.0                                                          # a saturated gate
    got = summary_stats([_t(p) for p in parts])
    flat = np.concatenate([p.reshape(-1) for p in parts])
    q = QC.quantiles(flat, QC.QUARTILES)
    assert list(got) == ["mean", "std", "min", "max", "q25", "q50", "q75"]
    assert (got["q25"], got["q50"], got["q75"]) == (q[0], q[1], q[2])
    assert (got["min"], got["max"]) == (float(flat.min()), float(flat.max()))
    f64 = flat.astype(np.float64)
    tol = flat.size * QC.U32 * np.abs(f64).mean()                                # float32 sums of n terms, in any order: n u mean |x|
    assert abs(got["mean"] - f64.mean()) <= tol and abs(got["std"] - f64.std(ddof=1)) <= 4.0 * tol / f64.std(ddof=1)
    one = summary_stats([_t(parts[0])])
    assert one["q50"] == QC.quantiles(parts[0].reshape(-1), [0.5])[0]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_before_a_launch():
    x = torch.zeros(100, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="D <= 16"):
        masked_quantiles(torch.zeros(4, 17, device=DEV), 0.5)
    with pytest.raises(ValueError, match="Q <= 8"):
        masked_quantiles(x, [0.1] * 9)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        masked_quantiles(x, [0.5, 1.5])
    with pytest.raises(ValueError, match="C <= 65535"):
        ops.quantile_select([0.5], 65536, 1, cells=torch.zeros(4, dtype=torch.int32, device=DEV), keys=torch.zeros(1, 4, dtype=torch.int32, device=DEV),
                            cursor=torch.zeros(1, dtype=torch.int64, device=DEV))
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        masked_quantiles(x.cpu(), 0.5)
    g = GroupedQuantiles([1, 2, 3], 1)
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        g.partial_fit(torch.zeros(10, 1), torch.ones(10, dtype=torch.int32, device=DEV))
    lib = _lib.load()
    n, f = ctypes.c_void_p(0), ctypes.c_void_p(x.data_ptr())
    pr = (ctypes.c_double * 9)(*([0.5] * 9))
    p = ctypes.cast(pr, ctypes.c_void_p)
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    o = ctypes.c_void_p(out.data_ptr())
    ws = torch.zeros(4 * 2 * 8 * 258, dtype=torch.uint8, device=DEV)
    w = ctypes.c_void_p(ws.data_ptr())
    for c, d, q in ((1, 17, 1), (1, 1, 9), (65536, 1, 1), (2, 1, 1)):             # the last: X goes into one cell
        assert lib.frl_quantile_select(n, n, 0, n, f, n, 100, c, d, p, q, 0, o, o, o, o, w, ws.numel(), n) == -2
    pr[0] = 1.5
    assert lib.frl_quantile_select(n, n, 0, n, f, n, 100, 1, 1, p, 1, 0, o, o, o, o, w, ws.numel(), n) == -2
    pr[0] = 0.5
    assert lib.frl_quantile_select(n, n, 0, n, f, n, 2 ** 31, 1, 1, p, 1, 0, o, o, o, o, w, ws.numel(), n) == -2
    assert lib.frl_quantile_select(n, n, 0, n, f, n, 100, 1, 1, p, 1, 4097, o, o, o, o, w, ws.numel(), n) == -2
    assert lib.frl_quantile_select(n, n, 0, n, f, n, 100, 1, 1, p, 1, 0, o, o, o, o, w, 4 * 2 * 258 - 1, n) == -4
    torch.cuda.synchronize()
    assert not out.any()                                                         # nothing was launched
