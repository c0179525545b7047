"""CPU tests of the exact quantiles: the numpy restatement of tests/quantile_cases.py against np.percentile (exactly) and against what
the reference's EvtReservoir and save_csv gave (tests/golden/quantile_recovery.npz, within the bound derived in quantile_cases.py), the
ABI, and the refusals that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import quantile_cases as QC
import strata_cases as SC
from frl_hip import _lib, ops, quantiles as Q, strata as S


# ---- 1. the restatement against numpy ------------------------------------------------------------------------------------------------
def test_restatement_equals_numpy_percentile_exactly():
    rng = np.random.default_rng(0)
    arrays = [QC.key_order_values(n) for n in QC.KEY_ORDER_N]
    for i in range(400):
        n = int(rng.integers(1, 400))
        x = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 4) + rng.integers(-2, 3) * 100.0).astype(np.float32)
        if i % 3 == 0:
            x[rng.random(n) < 0.3] = x[0]                                        # ties
        arrays.append(x)
    for x in arrays:
        got = QC.quantiles(x, QC.PROBS7)
        want = np.percentile(x.astype(np.float64), [100.0 * q for q in QC.PROBS7])
        assert np.array_equal(got, want), (x.size, got, want)


def test_restatement_brackets_and_empty_cell():
    lo, hi, t = QC.order_statistics(np.array([3.0, -0.0, 1.0, 2.0], np.float32), [0.0, 0.5, 1.0])
    assert lo.tolist() == [0.0, 1.0, 3.0] and hi.tolist() == [1.0, 2.0, 3.0] and t.tolist() == [0.0, 0.5, 0.0]
    assert not np.signbit(lo[0])                                                 # -0.0 folded
    lo, hi, t = QC.order_statistics(np.zeros(0, np.float32), [0.25])
    assert np.isnan(lo).all() and np.isnan(hi).all() and t.tolist() == [0.0]


def test_interpolate_is_the_restatement_lerp():
    rng = np.random.default_rng(1)
    lo = rng.normal(size=(3, 2, 4)).astype(np.float32)
    hi = lo + rng.random((3, 2, 4)).astype(np.float32)
    t = rng.random((3, 4))
    want = QC.lerp(lo, hi, t[:, None, :])
    assert np.array_equal(Q.interpolate(lo, hi, t), want)
    assert np.array_equal(Q.interpolate(torch.from_numpy(lo), torch.from_numpy(hi), torch.from_numpy(t)).numpy(), want)


# ---- 2. the restatement against the reference ---------------------------------------------------------------------------------------
def test_recovery_restatement_matches_the_reference(golden_dir):
    fx = np.load(os.path.join(golden_dir, "quantile_recovery.npz"))
    inp = QC.recovery_inputs()
    assert SC.checksum(*[inp[k] for k in ("evt_grid", "ysfc", "pred_nbr", "obs_nbr", "mask", "vocab")]) == int(fx["checksum"])
    rows, bounds, n_seen = QC.recovery_table(inp, [int(c) for c in inp["vocab"]])
    assert len(rows) == len(fx["evt_code"]) >= 30
    assert [r["evt_code"] for r in rows] == fx["evt_code"].tolist() and [r["bin"] for r in rows] == fx["bin"].tolist()
    assert [r["n_samples"] for r in rows] == fx["n_samples"].tolist()
    assert n_seen == dict(zip(fx["n_seen_codes"].tolist(), fx["n_seen"].tolist()))
    for code in set(r["evt_code"] for r in rows):                                # observations at or beyond the last bin edge count in n_seen
        assert n_seen[code] >= sum(r["n_samples"] for r in rows if r["evt_code"] == code)
    assert sum(n_seen[c] for c in set(r["evt_code"] for r in rows)) > sum(r["n_samples"] for r in rows)
    worst = 0.0
    for i, (row, bound) in enumerate(zip(rows, bounds)):
        for k in QC.RECOVERY_COLUMNS:
            err = abs(row[k] - fx[k][i])
            worst = max(worst, err / bound[k])
            assert err <= bound[k], (row["evt_code"], row["bin"], k, err, bound[k])
    print(f"largest distance from the reference at {worst:.4f} of the derived bound (the golden's report: {float(fx['worst_ratio']):.4f})")
    assert worst == float(fx["worst_ratio"])


def test_recovery_bins_are_the_references():
    assert S.RECOVERY_YSFC_BINS == QC.RECOVERY_BINS and len(S.RECOVERY_YSFC_BIN_LABELS) == 8
    assert S.RECOVERY_YSFC_BINS != S.YSFC_BINS and S.RECOVERY_YSFC_BINS == S.YSFC_BINS[:8]


# ---- 3. the ABI ----------------------------------------------------------------------------------------------------------------------
def test_quantile_symbols_are_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("frl_quantile_workspace_bytes", "frl_quantile_append", "frl_quantile_select"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    fn = lib.frl_quantile_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    assert fn(1, 1, 1) == 4 * 2 * (256 + 2) and fn(3, 2, 3) == 4 * 36 * 258
    assert fn(1, 17, 1) == 0 and fn(1, 1, 9) == 0 and fn(65536, 1, 1) == 0 and fn(0, 1, 1) == 0


# ---- 4. refusals that need no GPU ----------------------------------------------------------------------------------------------------
def test_refusals_before_a_device_is_touched():
    x = torch.zeros(10, dtype=torch.float32)
    with pytest.raises(ValueError, match="D <= 16"):
        Q.masked_quantiles(torch.zeros(4, 17), 0.5)
    with pytest.raises(ValueError, match="Q <= 8"):
        Q.masked_quantiles(x, [0.1] * 9)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            Q.masked_quantiles(x, [0.5, bad])
    with pytest.raises(ValueError, match="C <= 65535"):
        Q.GroupedQuantiles(np.arange(1, 4096), 1, n_rows=17)                      # 4095 x 17 = 69 615 cells
    assert Q.GroupedQuantiles(np.arange(1, 4096), 1, n_rows=16).count_.shape == (16, 4095)   # 65 520 cells
    with pytest.raises(ValueError, match="D <= 16"):
        Q.GroupedQuantiles([1, 2], 17)
    with pytest.raises(ValueError, match="float32"):
        Q.masked_quantiles(x.double(), 0.5)
    with pytest.raises(ValueError, match="mask must be"):
        Q.masked_quantiles(x, 0.5, mask=torch.ones(9, dtype=torch.bool))
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        Q.masked_quantiles(x, 0.5)
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        Q.summary_stats([x])
    g = Q.GroupedQuantiles([1, 2, 3], 2, n_rows=2)
    with pytest.raises(ValueError, match="columns"):
        g.partial_fit(torch.zeros(10, 3), torch.ones(10, dtype=torch.int32), torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows must be given"):
        g.partial_fit(torch.zeros(10, 2), torch.ones(10, dtype=torch.int32))
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        g.partial_fit(torch.zeros(10, 2), torch.ones(10, dtype=torch.int32), torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match="Q <= 8"):
        g.quantiles([0.5] * 9)
    rc = S.RecoveryCurves([1, 2, 3])
    with pytest.raises(_lib.FrlHipError, match="must live on the GPU"):
        rc.add(torch.ones(1, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4), torch.zeros(1, 2, 4, 4))
    with pytest.raises(ValueError, match="contiguous and increasing"):
        S.RecoveryCurves([1], bins=[(0, 1), (2, 3)])
    assert Q.summary_stats([]) == {k: 0.0 for k in ("mean", "std", "min", "max", "q25", "q50", "q75")}
    with pytest.raises(ValueError, match="C <= 65535"):
        ops.chk_quantile_dims(65536, 1, 1)


def test_nothing_accumulated_reads_as_empty():
    g = Q.GroupedQuantiles([5, 9], 2, n_rows=3)
    assert g.count_.shape == (3, 2) and not g.count_.any() and (g.unmatched_, g.rejected_, g.nonfinite_, g.dropped_) == (0, 0, 0, 0)
    assert np.isnan(g.quantiles([0.25, 0.5])).all() and g.quantiles([0.25, 0.5]).shape == (3, 2, 2, 2)
