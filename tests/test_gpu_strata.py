"""GPU tests of the EVT-stratified diagnostics (csrc/strata.hip, frl_hip/strata.py) against the float64 restatement of
tests/strata_cases.py and what the reference's own functions gave (tests/golden/strata_*.npz).

The contingency table, `unmatched` and `rejected` are integers and are held to exact equality.

Moments: counts exact; S1, S2 and SW within strata_cases.sum_bounds of the float64 sums of the same float32 inputs about the pivot the
accumulator reports, (n + T + 8) u sum |t_i| per (group, column) with u = 2^-24 (the terms are derived in strata_cases.py; nothing of the
bound comes from the kernel's output).  The bound covers any order of accumulation, so it is asserted for every `workgroups`.

End to end: gamma_stats, temporal_frac and probe_r2 against the reference's EvtAccumulators within the first-order propagation of those
bounds, doubled (strata_cases.propagate_*), plus the 1e-12 relative that test_cpu_strata.py allows between the reference and the
restatement; the clustering metrics against sklearn's at 1e-12.
"""
import os

import numpy as np
import pytest
import torch

import strata_cases as SC
from frl_hip import ops, strata as S
from frl_hip.strata import ContingencyTable, EvtAccumulators, GroupedMoments

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


# ---- 1. the contingency table ------------------------------------------------------------------------------------------------------
def _fit_table(c, table=None, workgroups=0):
    """Feeds a strata_cases.table_case through ContingencyTable: labels and mask per pixel [B, P] or per timestep [B, T, P]."""
    if table is None:
        table = ContingencyTable(c["R"], c["vocab"], workgroups=workgroups)
    rows, mask = c["rows"], c["mask"]
    rows = rows[:, 0] if rows.shape[1] == 1 and c["T"] > 1 else rows
    if mask is not None and mask.shape[1] == 1 and c["T"] > 1:
        mask = mask[:, 0]
    assert c["T"] == 1 or rows.ndim == 3 or (mask is not None and mask.ndim == 3), "no input of this case carries T"
    return table.partial_fit(_t(rows), _t(c["codes"]), _t(mask))


def _check_table(t, c, what):
    want, unmatched, rejected = SC.contingency(c["rows"], c["codes"], c["mask"], c["vocab"], c["R"], c["T"])
    got, cols = t.table()
    print(f"{what}: {int(want.sum())} counted, {unmatched} unmatched, {rejected} rejected")
    assert cols == c["vocab"].tolist()
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} cells differ"
    assert (t.unmatched_, t.rejected_) == (unmatched, rejected)


def _combos():
    out, i = [], 0
    for shape in SC.TABLE_SHAPES:
        for size in SC.TABLE_SIZES:
            for as_float in (False, True):
                tr_full, tm = bool(i % 2), (None, False, True)[i % 3]
                if shape[1] > 1 and not tr_full and not tm:
                    tr_full = True                                               # something must carry T
                out.append(pytest.param(shape, size, as_float, tr_full, tm, id=f"{shape}-{size}-{'f32' if as_float else 'i32'}-Tr{int(tr_full)}-Tm{tm}"))
                i += 1
    return out


@pytest.mark.parametrize("shape,size,as_float,tr_full,tm", _combos())
def test_contingency_is_exact(shape, size, as_float, tr_full, tm):
    c = SC.table_case(shape, size, as_float, tr_full, tm)
    _check_table(_fit_table(c), c, "table")


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("tr_full,tm", [(True, None), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("size", [(20, 15), (50, 300)])
def test_contingency_broadcasts_rows_and_mask(size, tr_full, tm, as_float):
    c = SC.table_case((3, 5, 1000), size, as_float, tr_full, tm, seed=1)
    valid, col = SC.lookup(c["codes"], c["vocab"])
    if as_float:
        assert np.isnan(c["codes"]).any() and np.isinf(c["codes"]).any() and (c["codes"] != np.floor(c["codes"]))[valid].any()
    assert (c["codes"] <= 0).any() and (valid & (col < 0)).any() and ((c["rows"] < 0) | (c["rows"] >= c["R"])).any()
    _check_table(_fit_table(c), c, "broadcast")


@pytest.mark.parametrize("workgroups", [1, 3, 4096])
def test_contingency_for_any_grid(workgroups):
    c = SC.table_case((3, 5, 1000), (20, 15), False, True, True, seed=2)
    _check_table(_fit_table(c, workgroups=workgroups), c, f"workgroups {workgroups}")


@pytest.mark.parametrize("size", [(20, 15), (50, 300)])
def test_contingency_all_zero_mask(size):
    c = SC.table_case((2, 1, 257), size, False, True, False, seed=3)
    c["mask"] = np.zeros_like(c["mask"])
    t = _fit_table(c)
    assert not t.table()[0].any() and (t.unmatched_, t.rejected_) == (0, 0)


@pytest.mark.parametrize("size,cell", [((2, 3), (1, 2)), ((50, 300), (49, 299))])
def test_contingency_single_cell_contention(size, cell):
    r, g = size
    vocab = np.arange(10, 10 + g, dtype=np.int32)
    n = 70000                                                                    # more than 16 bits in one cell
    t = ContingencyTable(r, vocab).partial_fit(torch.full((n,), cell[0], dtype=torch.int32, device=DEV),
                                               torch.full((n,), int(vocab[cell[1]]), dtype=torch.int32, device=DEV))
    want = np.zeros(size, np.int64)
    want[cell] = n
    assert np.array_equal(t.table()[0], want)


def test_contingency_two_calls_equal_one():
    c = SC.table_case((3, 5, 1000), (20, 15), True, True, True, seed=4)
    one = _fit_table(c)
    two = ContingencyTable(c["R"], c["vocab"])
    for sl in (slice(0, 1), slice(1, 3)):
        two.partial_fit(_t(c["rows"][sl]), _t(c["codes"][sl]), _t(c["mask"][sl]))
    assert np.array_equal(one.table()[0], two.table()[0])
    assert (one.unmatched_, one.rejected_) == (two.unmatched_, two.rejected_)
    _check_table(two, c, "two calls")


@pytest.mark.parametrize("as_float", [False, True])
def test_contingency_discovers_the_vocabulary(as_float):
    c = SC.table_case((3, 5, 1000), (20, 15), as_float, True, True, seed=5)
    given = _fit_table(c)
    found = ContingencyTable(c["R"])
    for sl in (slice(0, 1), slice(1, 2), slice(2, 3)):                           # the vocabulary grows from call to call
        found.partial_fit(_t(c["rows"][sl]), _t(c["codes"][sl]), _t(c["mask"][sl]))
    tg, cg = given.table()
    tf, cf = found.table()
    assert set(cg) <= set(cf) and found.unmatched_ == 0                          # discovery also finds the codes outside the given vocabulary
    assert np.array_equal(tf[:, [cf.index(code) for code in cg]], tg)
    extra = [i for i, code in enumerate(cf) if code not in cg]
    assert int(tf[:, extra].sum()) + found.rejected_ - given.rejected_ == given.unmatched_
    assert found.top_codes(3) == [cf[i] for i in np.lexsort((np.asarray(cf), -tf.sum(0)))[:3]]


def test_ysfc_histogram():
    rng = np.random.default_rng(7)
    b, t, p = 2, 6, 333
    vocab = SC.make_vocab(rng, 9)
    codes = SC.make_codes(rng, vocab, (b, p), True)
    ysfc = rng.integers(-3, 50, size=(b, t, p)).astype(np.float32)
    ysfc[rng.random((b, t, p)) < 0.05] = np.nan
    mask = rng.random((b, t, p)) < 0.8
    table = S.ysfc_evt_histogram(_t(ysfc), _t(codes), _t(mask), evt_codes=vocab)
    keep = mask & (ysfc >= 0) & (ysfc <= 40.0)
    lo = np.array([a for a, _ in S.YSFC_BINS])
    rows = (np.searchsorted(lo, np.nan_to_num(ysfc, nan=0.0), side="right") - 1).astype(np.int32)
    want, unmatched, rejected = SC.contingency(rows, codes, keep, vocab, len(S.YSFC_BINS), t)
    assert np.array_equal(table.table()[0], want) and (table.unmatched_, table.rejected_) == (unmatched, 0) and rejected == 0
    for (a, z), row in zip(S.YSFC_BINS, want):                                   # the reference's own count per bin
        valid, col = SC.lookup(codes, vocab)
        sel = keep & (ysfc >= a) & (ysfc < z) & np.broadcast_to((col >= 0)[:, None], keep.shape)
        assert int(sel.sum()) == int(row.sum())


# ---- 2. grouped moments ------------------------------------------------------------------------------------------------------------
def _fit_moments(c, temporal, pivot=None, workgroups=0):
    g = GroupedMoments(c["vocab"], c["X"].shape[-1], temporal=temporal, pivot=pivot, workgroups=workgroups)
    b, t, p, dd = c["X"].shape
    return g.partial_fit(_t(c["X"].reshape(b, t, p, 1, dd)), _t(c["codes"].reshape(b, p, 1)), _t(c["mask"].reshape(b, -1, p, 1) if c["mask"].shape[1] > 1
                                                                                                 else c["mask"].reshape(b, p, 1)))


def _check_moments(g, c, temporal, what):
    pivot = g.pivot_.astype(np.float32)
    want = SC.moments(c["X"], c["codes"], c["mask"], c["vocab"], pivot, temporal)
    bound = SC.sum_bounds(c["X"], c["codes"], c["mask"], c["vocab"], pivot, temporal)
    n, s1, s2 = g.pivoted()
    assert np.array_equal(n, want["count"]), f"{what}: counts differ"
    assert g.unmatched_ == want["unmatched"]
    ratios = []
    for key, got in (("S1", s1), ("S2", s2), ("SW", g.within_)):
        if want[key] is None:
            assert got is None
            continue
        err = np.abs(got - want[key])
        ratios.append(float((err / np.maximum(bound[key], 1e-300)).max()))
        print(f"{what} {key}: largest error at {ratios[-1]:.4f} of its bound")
        assert np.all(err <= bound[key]), f"{what} {key}: {ratios[-1]:.3f} of the bound"
        assert np.all(got[n == 0] == 0)
    return want, bound


@pytest.mark.parametrize("temporal", [False, True], ids=["observations", "temporal"])
@pytest.mark.parametrize("g", SC.MOMENT_GROUPS)
@pytest.mark.parametrize("shape", SC.MOMENT_SHAPES, ids=str)
def test_moments_within_bounds(shape, g, temporal):
    c = SC.moment_case(shape, g)
    m = _fit_moments(c, temporal)
    want, _ = _check_moments(m, c, temporal, f"{shape} G={g}")
    if g >= 2:
        assert want["count"][-1] == 0 and np.all(m.mean()[-1] == 0)              # the empty class
    if g >= 3 and shape[0] * shape[2] >= 8 and (temporal or shape[1] == 1):
        assert want["count"][-2] == 1 and np.all(m.var()[-2] <= 1e-4)            # the class of one row
    if temporal and shape[1] == 1:
        assert np.all(m.within_ == 0.0)                                          # exactly
    if g > m.window:
        windows = [(want["count"][a:a + m.window] > 0).any() for a in range(0, g, m.window)]
        assert len(windows) >= 2
        if shape == (1, 1, 1, 1):
            assert not all(windows)                                              # a window without a row


@pytest.mark.parametrize("temporal", [False, True], ids=["observations", "temporal"])
def test_moments_float_codes_and_per_step_mask(temporal):
    c = SC.moment_case((2, 5, 300, 12), 20, as_float=True, per_step_mask=not temporal, seed=1)
    assert np.isnan(c["codes"]).any() and c["mask"].shape[1] == (1 if temporal else 5)
    _check_moments(_fit_moments(c, temporal), c, temporal, "float codes")


@pytest.mark.parametrize("temporal", [False, True], ids=["observations", "temporal"])
def test_moments_pivot_matters(temporal):
    c = SC.moment_case((2, 5, 300, 12), 20, shift=1000.0, seed=2)
    m = _fit_moments(c, temporal)                                                # pivot: the mean of the call
    assert np.abs(m.pivot_ - 1000.0).max() < 2.0
    _, tight = _check_moments(m, c, temporal, "shifted, pivot mean")
    z = _fit_moments(c, temporal, pivot="zero")
    assert not z.pivot_.any()
    _, loose = _check_moments(z, c, temporal, "shifted, pivot zero")
    live = m.count_ > 0
    assert np.all(loose["S2"][live] > 1e4 * tight["S2"][live])                   # what the pivot buys, from the bounds alone
    # both give the same statistics, each within its own propagated bound
    n = np.maximum(m.count_, 1)[:, None].astype(np.float64)
    for a in (m, z):
        _, s1, s2 = a.pivoted()
        b = tight if a is m else loose
        want = SC.moments(c["X"], c["codes"], c["mask"], c["vocab"], np.zeros(12, np.float32), temporal)
        mean = np.where(live[:, None], want["S1"] / n, 0.0)
        assert np.all(np.abs(a.mean() - mean)[live] <= SC.propagate_mean(n, b["S1"])[live] + 1e-12 * np.abs(mean[live]))


@pytest.mark.parametrize("temporal", [False, True], ids=["observations", "temporal"])
@pytest.mark.parametrize("shape,g", [((2, 5, 300, 12), 20), ((1, 3, 70, 128), 127), ((1, 2, 70, 6), 20)])   # D = 6: the scalar staging path
def test_moments_for_any_grid_and_bit_identical(shape, g, temporal):
    c = SC.moment_case(shape, g, seed=3)
    pivot = np.full(shape[3], 0.25, np.float32)
    for workgroups in (1, 3, 0):
        runs = [_fit_moments(c, temporal, pivot=pivot, workgroups=workgroups) for _ in range(2)]
        _check_moments(runs[0], c, temporal, f"workgroups {workgroups}")
        assert torch.equal(runs[0]._s1, runs[1]._s1) and torch.equal(runs[0]._s2, runs[1]._s2) and torch.equal(runs[0]._count, runs[1]._count)
        if temporal:
            assert torch.equal(runs[0]._sw, runs[1]._sw)


@pytest.mark.parametrize("temporal", [False, True], ids=["observations", "temporal"])
def test_moments_more_tiles_than_workgroups_chunked(temporal):
    """More tiles of 64 pixels than the library starts workgroups, and a vocabulary of a full window and a shorter one: the shorter
    window runs more workgroups with smaller slabs out of the same workspace, and every workgroup walks more than one tile."""
    c = SC.moment_case((1, 2, 66000, 4), 200, seed=5)
    m = _fit_moments(c, temporal)
    assert m.window == 128 and 66000 // 64 > 1024
    _check_moments(m, c, temporal, "many tiles")


def test_moments_stream_and_layouts():
    c = SC.moment_case((2, 5, 300, 12), 20, seed=4)
    pivot = np.zeros(12, np.float32)
    one = _fit_moments(c, False, pivot=pivot)
    two = GroupedMoments(c["vocab"], 12, pivot=pivot)
    for b in range(2):                                                           # [B, T, H, W, D] sample by sample; then the counts add up
        two.partial_fit(_t(c["X"][b:b + 1].reshape(1, 5, 300, 1, 12)), _t(c["codes"][b:b + 1].reshape(1, 300, 1)), _t(c["mask"][b:b + 1].reshape(1, 300, 1)))
    assert np.array_equal(one.count_, two.count_)
    _check_moments(two, c, False, "two calls")
    flat = GroupedMoments(c["vocab"], 12, pivot=pivot)                            # [N, D] rows with [N] codes: one timestep of one sample
    flat.partial_fit(_t(c["X"][0, 0]), _t(c["codes"][0]), _t(c["mask"][0, 0]))
    c0 = dict(X=c["X"][:1, :1], codes=c["codes"][:1], mask=c["mask"][:1], vocab=c["vocab"])
    _check_moments(flat, c0, False, "[N, D]")
    cf = GroupedMoments(c["vocab"], 12, pivot=pivot)                              # channels-first [B, D, T, H, W]: one permute copy
    cf.partial_fit(_t(np.transpose(c["X"].reshape(2, 5, 300, 1, 12), (0, 4, 1, 2, 3))), _t(c["codes"].reshape(2, 300, 1)), _t(c["mask"].reshape(2, 300, 1)),
                   channels_last=False)
    assert torch.equal(cf._s1, one._s1) and torch.equal(cf._s2, one._s2)


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------
def _e2e_bounds(inp, acc):
    """Restated moments and their bounds about the pivots the accumulators chose -> {name: (moments, bounds, pivot)}."""
    b, t, h, w, d = inp["z_phase"].shape
    k = inp["pred"].shape[-1]
    codes, mask, vocab = inp["codes"].reshape(b, h * w), inp["mask"].reshape(b, 1, h * w), inp["vocab"]
    src = dict(gamma=(inp["gamma"].reshape(b, 1, h * w, d), False), phase=(inp["z_phase"].reshape(b, t, h * w, d), True),
               probe=(np.concatenate([inp["pred"] - inp["target"], inp["target"]], -1).reshape(b, t, h * w, 2 * k), False))
    out = {}
    for name, (x, temporal) in src.items():
        pivot = getattr(acc, name).pivot_.astype(np.float32)
        out[name] = (SC.moments(x, codes, mask, vocab, pivot, temporal), SC.sum_bounds(x, codes, mask, vocab, pivot, temporal), pivot.astype(np.float64))
    return out


@pytest.mark.parametrize("layout", ["channels_last", "reference"])
def test_evt_accumulators_match_the_reference(golden_dir, layout):
    fx = np.load(os.path.join(golden_dir, "strata_evt.npz"))
    inp = SC.e2e_inputs()
    assert SC.checksum(*[inp[k] for k in ("gamma", "z_phase", "pred", "target", "codes", "mask", "vocab")]) == int(fx["checksum"])
    b, t, h, w, d = inp["z_phase"].shape
    k, vocab = inp["pred"].shape[-1], inp["vocab"]
    acc = EvtAccumulators(d, k, codes=vocab)
    if layout == "channels_last":                                                # as forward_phase_nhwc and RidgeProbe.predict return them
        acc.add_pixels(_t(inp["codes"]), _t(inp["gamma"]), _t(inp["z_phase"]), _t(inp["mask"]))
        acc.add_probe(_t(inp["codes"]), _t(inp["pred"]), _t(inp["target"]), _t(inp["mask"]))
    else:                                                                        # [N, d, T] rows of one sample at a time, as the reference's process_batch
        for i in range(b):
            z = np.transpose(inp["z_phase"][i].reshape(t, h * w, d), (1, 2, 0))
            acc.add_pixels(_t(inp["codes"][i].reshape(-1)), _t(inp["gamma"][i].reshape(-1, d)), _t(z), _t(inp["mask"][i].reshape(-1)))
            acc.add_probe(_t(inp["codes"][i:i + 1]), _t(inp["pred"][i:i + 1]), _t(inp["target"][i:i + 1]), _t(inp["mask"][i:i + 1]))
    r = _e2e_bounds(inp, acc)
    in_vocab = [int(e) for e in fx["codes"] if int(e) in set(vocab.tolist())]
    assert acc.all_evt_codes() == in_vocab
    assert acc.unmatched_ == int(sum(fx["n"][i] for i, e in enumerate(fx["codes"]) if int(e) not in in_vocab))
    worst = {}
    for i, e in enumerate(fx["codes"]):
        if int(e) not in in_vocab:
            continue
        j = int(np.searchsorted(vocab, e))
        (mg, bg, _), (mp, bp, _), (mq, bq, pq) = r["gamma"], r["phase"], r["probe"]
        n = float(mg["count"][j])
        assert n == fx["n"][i] and mp["count"][j] == n and mq["count"][j] == n * t
        mean, std = acc.gamma_stats(int(e))
        tol = dict(mean=SC.propagate_mean(n, bg["S1"][j]), std=SC.propagate_std(n, mg["S1"][j], mg["S2"][j], bg["S1"][j], bg["S2"][j]),
                   frac=SC.propagate_temporal_frac(n, mp["S1"][j], mp["S2"][j], mp["SW"][j], bp["S1"][j], bp["S2"][j], bp["SW"][j]),
                   r2=SC.propagate_r2(n * t, pq[:k], mq["S1"][j, :k], mq["S2"][j, :k], bq["S1"][j, :k], bq["S2"][j, :k], mq["S1"][j, k:], mq["S2"][j, k:],
                                      bq["S1"][j, k:], bq["S2"][j, k:]))
        for key, got in (("mean", mean), ("std", std), ("frac", acc.temporal_frac(int(e))), ("r2", acc.probe_r2(int(e)))):
            err = np.abs(got.numpy() - fx[key][i])
            lim = tol[key] + 1e-12 * np.abs(fx[key][i])
            worst[key] = max(worst.get(key, 0.0), float((err / np.maximum(lim, 1e-300)).max()))
            assert np.all(err <= lim), (int(e), key, float(err.max()), float(lim.min()))
    print("largest error over its bound:", worst)
    empty = int(vocab[-1])
    assert not acc.gamma_stats(empty)[0].any() and not acc.temporal_frac(empty).any() and acc.probe_r2(empty) is None


@pytest.mark.parametrize("name", ["a", "b"])
def test_contingency_metrics_match_sklearn(golden_dir, name):
    fx = np.load(os.path.join(golden_dir, "strata_metrics.npz"))
    table, codes = SC.metric_table(name)
    assert SC.checksum(table, codes) == int(fx[name + "_checksum"])
    cl, ev = SC.expand_table(table, codes, seed=1)
    half = len(cl) // 2
    t = ContingencyTable(table.shape[0], codes)
    t.partial_fit(_t(cl[:half]), _t(ev[:half])).partial_fit(_t(cl[half:]), _t(ev[half:].astype(np.float32)))
    assert np.array_equal(t.table()[0], table)
    m = t.metrics()
    for i, key in enumerate(SC.METRIC_KEYS):
        assert abs(m[key] - fx[name][i]) <= 1e-12, (key, m[key], fx[name][i])
