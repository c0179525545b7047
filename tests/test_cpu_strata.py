"""CPU tests of the EVT-stratified diagnostics (frl_hip/strata.py): what needs no GPU.

clustering_metrics against what the reference's compute_metrics (sklearn 1.7.2) gave for the same tables with every label pair given
(tests/golden/strata_metrics.npz): 1e-12 absolute, float64 formulas over at most R G terms on both sides.  The restatement of
strata_cases.py against the reference's EvtAccumulators (tests/golden/strata_evt.npz): 1e-12 relative, float64 on the same float32 inputs
on both sides.  The un-pivoting algebra of GroupedMoments and EvtAccumulators from exact float64 sums about three pivots: 1e-9 relative to
the scale of the sums, what float64 leaves of sums of a few hundred terms about a pivot 2.5 off the mean.
"""
import os
import warnings

import numpy as np
import pytest
import torch

import strata_cases as SC
from frl_hip import _lib, ops, strata as S
from frl_hip.strata import ContingencyTable, EvtAccumulators, GroupedMoments, clustering_metrics


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"strata_{name}.npz"))


# ---- 1. metrics of a table ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.METRIC_TABLES)
def test_clustering_metrics_match_the_reference(golden_dir, name):
    fx = _fx(golden_dir, "metrics")
    table, codes = SC.metric_table(name)
    assert SC.checksum(table, codes) == int(fx[name + "_checksum"]), "the case generator changed under the golden"
    m = clustering_metrics(table)
    assert list(m) == SC.METRIC_KEYS
    for i, k in enumerate(SC.METRIC_KEYS):
        print(name, k, m[k], fx[name][i])
        assert abs(m[k] - fx[name][i]) <= 1e-12, (name, k, m[k], fx[name][i])
    assert isinstance(m["n_pixels_metrics"], int) and m["n_pixels_metrics"] == int(table.sum())


def test_clustering_metrics_degenerate_tables():
    one_cluster = clustering_metrics(np.array([[4, 9, 2]]))
    assert (one_cluster["nmi"], one_cluster["homogeneity"], one_cluster["completeness"], one_cluster["v_measure"]) == (0.0, 0.0, 1.0, 0.0)
    assert one_cluster["purity"] == 9 / 15
    one_class = clustering_metrics(np.array([[4], [9], [2]]))
    assert (one_class["nmi"], one_class["homogeneity"], one_class["completeness"], one_class["v_measure"]) == (0.0, 1.0, 0.0, 0.0)
    assert one_class["purity"] == 1.0
    single = clustering_metrics(np.array([[1]]))
    assert [single[k] for k in SC.METRIC_KEYS] == [1.0, 1.0, 1.0, 1.0, 1.0, 1]
    both = clustering_metrics(np.array([[0, 0], [0, 7]]))                        # one cluster and one class in use: both entropies 0
    assert both["nmi"] == 1.0 and both["v_measure"] == 1.0
    with pytest.raises(ValueError):
        clustering_metrics(np.zeros((2, 2), np.int64))
    with pytest.raises(ValueError):
        clustering_metrics(np.ones((2, 2)))                                      # counts are integers


def test_metrics_refuse_rejected_rows_and_warn_on_unmatched():
    table, codes = SC.metric_table("a")
    with pytest.raises(ValueError, match="row label"):
        ContingencyTable.from_table(table, codes, rejected=3).metrics()
    with pytest.warns(UserWarning, match="5 observations"):
        m = ContingencyTable.from_table(table, codes, unmatched=5).metrics()
    assert m["n_unmatched"] == 5 and m["n_pixels_metrics"] == int(table.sum())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert ContingencyTable.from_table(table, codes).metrics()["n_unmatched"] == 0


# ---- 2. the restatement against the reference's accumulators -----------------------------------------------------------------------
def test_restatement_matches_the_reference_accumulators(golden_dir):
    fx = _fx(golden_dir, "evt")
    inp = SC.e2e_inputs()
    assert SC.checksum(*[inp[k] for k in ("gamma", "z_phase", "pred", "target", "codes", "mask", "vocab")]) == int(fx["checksum"])
    st = SC.evt_stats(inp)
    assert sorted(st) == [int(e) for e in fx["codes"]]
    for i, e in enumerate(fx["codes"]):
        s = st[int(e)]
        assert s["n"] == int(fx["n"][i])
        for k in ("mean", "std", "frac", "r2"):
            assert np.all(np.abs(s[k] - fx[k][i]) <= 1e-12 * np.abs(fx[k][i])), (int(e), k)
    n = fx["n"]
    assert (n == 1).any() and (n > 50).any()                                     # a class of one pixel and full ones


# ---- 3. un-pivoting from exact sums ------------------------------------------------------------------------------------------------
def _pivot(kind, x, live_mean):
    if kind == "zero":
        return np.zeros(x.shape[-1], np.float32)
    return (live_mean + (2.5 if kind == "off" else 0.0)).astype(np.float32)


@pytest.mark.parametrize("kind", ["mean", "zero", "off"])
def test_grouped_moments_unpivot(kind):
    c = SC.moment_case((2, 5, 300, 12), 20)
    x, codes, mask, vocab = c["X"], c["codes"], c["mask"], c["vocab"]
    zero = SC.moments(x, codes, mask, vocab, np.zeros(12, np.float32))           # about zero: the plain sums
    pivot = _pivot(kind, x, zero["S1"].sum(0) / zero["count"].sum())
    m = SC.moments(x, codes, mask, vocab, pivot)
    g = GroupedMoments.from_sums(vocab, m["count"], m["S1"], m["S2"], pivot)
    n = np.maximum(m["count"], 1)[:, None]
    assert np.array_equal(g.count_, m["count"]) and g.count_[-1] == 0
    scale1, scale2 = np.abs(zero["S1"]).max(), np.abs(zero["S2"]).max()
    assert np.abs(g.sum() - zero["S1"]).max() <= 1e-9 * scale1
    assert np.abs(g.sumsq() - zero["S2"]).max() <= 1e-9 * scale2
    mean = zero["S1"] / n
    var = zero["S2"] / n - mean ** 2
    assert np.abs(g.mean() - mean).max() <= 1e-9 and np.abs(g.var() - np.maximum(var, 0)).max() <= 1e-9
    assert np.all(g.mean()[-1] == 0) and np.all(g.var()[-1] == 0)                # the empty class


@pytest.mark.parametrize("kind", ["mean", "zero", "off"])
def test_evt_accumulators_from_exact_sums(golden_dir, kind):
    fx = _fx(golden_dir, "evt")
    inp = SC.e2e_inputs()
    b, t, h, w, d = inp["z_phase"].shape
    k, vocab = inp["pred"].shape[-1], inp["vocab"]
    codes, mask = inp["codes"].reshape(b, h * w), inp["mask"].reshape(b, 1, h * w)
    acc = EvtAccumulators(d, k, codes=vocab)
    sources = dict(gamma=(inp["gamma"].reshape(b, 1, h * w, d), False), phase=(inp["z_phase"].reshape(b, t, h * w, d), True),
                   probe=(np.concatenate([inp["pred"] - inp["target"], inp["target"]], -1).reshape(b, t, h * w, 2 * k), False))
    for name, (x, temporal) in sources.items():
        zero = SC.moments(x, codes, mask, vocab, np.zeros(x.shape[-1], np.float32), temporal)
        pivot = _pivot(kind, x, zero["S1"].sum(0) / zero["count"].sum())
        m = SC.moments(x, codes, mask, vocab, pivot, temporal)
        setattr(acc, name, GroupedMoments.from_sums(vocab, m["count"], m["S1"], m["S2"], pivot, within=m["SW"]))
    in_vocab = [int(e) for e in fx["codes"] if int(e) in set(vocab.tolist())]
    assert acc.all_evt_codes() == in_vocab and int(vocab[-1]) not in in_vocab and int(vocab[-2]) in in_vocab
    for i, e in enumerate(fx["codes"]):
        if int(e) not in in_vocab:
            continue
        mean, std = acc.gamma_stats(int(e))
        assert mean.dtype == torch.float64 and tuple(mean.shape) == (d,)
        # pred - target is formed in float32 here and in float64 by the reference: 2 u of ssres / sstot on R^2
        for got, key, tol in ((mean, "mean", 1e-9), (std, "std", 1e-7), (acc.temporal_frac(int(e)), "frac", 1e-9), (acc.probe_r2(int(e)), "r2", 1e-5)):
            assert np.abs(got.numpy() - fx[key][i]).max() <= tol, (kind, int(e), key, np.abs(got.numpy() - fx[key][i]).max())
        assert acc.n_pixels(int(e)) == int(fx["n"][i])
    empty = int(vocab[-1])
    z, s = acc.gamma_stats(empty)
    assert torch.equal(z, torch.zeros(d, dtype=torch.float64)) and torch.equal(s, z)
    assert torch.equal(acc.temporal_frac(empty), z) and acc.probe_r2(empty) is None
    assert EvtAccumulators(d, None, codes=vocab).probe_r2(in_vocab[0]) is None


# ---- 4. constants and orders -------------------------------------------------------------------------------------------------------
def test_ysfc_bins_are_the_reference_bins():
    assert S.YSFC_BINS == [(0, 1), (1, 2), (2, 3), (3, 5), (5, 8), (8, 13), (13, 20), (20, 31), (31, 41)]
    assert S.YSFC_BIN_LABELS == ["0", "1", "2", "3–4", "5–7", "8–12", "13–19", "20–30", "31–40"]
    assert len(S.YSFC_BINS) == len(S.YSFC_BIN_LABELS) == 9


def test_top_codes_order_and_ties():
    table = np.array([[3, 0, 5, 1, 2], [2, 5, 0, 4, 3]])                         # column totals 5 5 5 5 5 -> by code; then perturbed
    codes = [7, 11, 20, 31, 44]
    assert ContingencyTable.from_table(table, codes).top_codes(3) == [7, 11, 20]
    table[0, 3] += 2                                                             # 31 leads, the others tie
    t = ContingencyTable.from_table(table, codes)
    assert t.top_codes(3) == [31, 7, 11] and t.top_codes(10) == [31, 7, 11, 20, 44] and t.top_codes(0) == []
    got, cols = t.table()
    assert got.dtype == np.int64 and np.array_equal(got, table) and cols == codes


# ---- 5. limits and devices ---------------------------------------------------------------------------------------------------------
def test_limits_are_refused_before_any_device():
    with pytest.raises(ValueError, match="R <= 4096"):
        ContingencyTable(4097, [1, 2])
    with pytest.raises(ValueError, match="G <= 4095"):
        ContingencyTable(4, range(1, 4097))
    with pytest.raises(ValueError):
        ContingencyTable(0, [1])
    with pytest.raises(ValueError, match="D <= 128"):
        GroupedMoments([1, 2], 129)
    with pytest.raises(ValueError, match="G <= 4095"):
        GroupedMoments(range(1, 4097), 4)
    with pytest.raises(ValueError, match="workgroups"):
        GroupedMoments([1, 2], 4, workgroups=4097)
    with pytest.raises(ValueError, match="Gc \\* D"):
        ops.chk_strata_moment_dims(65, 127)
    with pytest.raises(ValueError, match="Gc <= 128"):
        ops.chk_strata_moment_dims(129, 4)
    ops.chk_strata_table_dims(4096, 4095)                                        # R G <= 2^24 follows from the limits of R and G
    assert 4096 * 4095 <= ops.STRATA_MAX_CELLS
    assert GroupedMoments(range(1, 301), 128).window == 64 and GroupedMoments(range(1, 301), 12).window == 128
    # the raw calls check sizes before they look at the device: CPU tensors with sizes out of limits are a ValueError
    x = torch.zeros(1, 1, 4, 129)
    codes, vocab = torch.ones(1, 4, dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    z = torch.zeros(1, 129, dtype=torch.float64)
    with pytest.raises(ValueError, match="D <= 128"):
        ops.strata_moments(x, codes, None, vocab, 0, 1, torch.zeros(129), torch.zeros(1, dtype=torch.int64), z, z.clone(), None, None,
                           torch.zeros(256, dtype=torch.uint8))
    with pytest.raises(ValueError, match="R <= 4096"):
        ops.strata_contingency(torch.zeros(1, 1, 4, dtype=torch.int32), codes, None, vocab, torch.zeros(4097, 1, dtype=torch.int64),
                               torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))


@pytest.mark.parametrize("temporal", [0, 1])
@pytest.mark.parametrize("d", [1, 4, 12, 64, 128])
def test_workspace_covers_every_shorter_window(d, temporal):
    """GroupedMoments sizes one workspace for its window and walks the last, shorter chunk of a vocabulary with it: a shorter window
    has smaller slabs but may run more workgroups, and must still fit."""
    lib = _lib.load()
    top = min(128, 8192 // d)
    for workgroups in (0, 7):
        sizes = [lib.frl_strata_workspace_bytes(gc, d, temporal, workgroups) for gc in range(1, top + 1)]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert lib.frl_strata_workspace_bytes(top + 1, d, temporal, 0) == 0          # past Gc <= 128 or Gc D <= 8192
    assert lib.frl_strata_workspace_bytes(1, d, temporal, 4097) == 0


def test_cpu_tensors_are_refused():
    labels, codes = torch.zeros(2, 8, dtype=torch.int32), torch.ones(2, 8, dtype=torch.int32)
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        ContingencyTable(3, [1, 2]).partial_fit(labels, codes)
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        ContingencyTable(3).partial_fit(labels, codes)
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        GroupedMoments([1, 2], 4).partial_fit(torch.zeros(2, 2, 4, 4), codes.view(2, 2, 4))
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        ops.strata_workspace(2, 4, False, "cpu")
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        EvtAccumulators(4, None, codes=[1, 2]).add_pixels(codes.view(2, 2, 4), torch.zeros(2, 2, 4, 4), torch.zeros(2, 3, 2, 4, 4))
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        S.ysfc_evt_histogram(torch.zeros(2, 3, 8), codes, None, evt_codes=[1, 2])
    with pytest.raises(_lib.FrlHipError, match="GPU"):
        ops.strata_contingency(torch.zeros(1, 1, 4, dtype=torch.int32), torch.ones(1, 4, dtype=torch.int32), None, torch.tensor([1], dtype=torch.int32),
                               torch.zeros(2, 1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
