"""GPU parity of the fused EVT soft-neighbourhood loss (csrc/evt_soft_neighborhood.hip) against the fixtures written by the REFERENCE's
functions (tests/golden/make_evt_golden.py) and, for shapes not committed, against the float64 restatement (tests/evt_cases.py).
Bounds: those of the other loss parity tests, 2e-6 * max(1, |loss64|) on losses and mean statistics and 1e-5 * max|grad64| on gradients;
where the float32 reference itself (loss32 / grad32) sits further than that from float64, twice its own deviation (fixed-order fused
reductions should not be worse than twice stock float32).  Counts are equal."""
import json
import os

import numpy as np
import pytest
import torch

import evt_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


@pytest.fixture(scope="module")
def metrics(golden_dir):
    from frl_hip.losses import EvtDiffusionMetric
    with open(os.path.join(golden_dir, "evt_counts_small.json")) as fh:
        counts = json.load(fh)
    return {name: EvtDiffusionMetric(os.path.join(golden_dir, "evt_confusion_small.csv"), counts, **kw).to(DEV)
            for name, kw in EC.METRIC_SETTINGS.items()}


def _case(golden_dir, metrics, name):
    fx = _fx(golden_dir, f"evt_{name}")
    kw = dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), min_valid_anchors=int(fx["min_valid_anchors"]))
    return fx, metrics[str(fx["metric"])], kw, torch.from_numpy(fx["emb"]), torch.from_numpy(fx["codes"])


def _check_loss(got, want, what, ref32=None):
    got, want = float(got.detach()) if torch.is_tensor(got) else float(got), float(want)
    own = abs(float(ref32) - want) if ref32 is not None else 0.0
    bound = max(2e-6 * max(1.0, abs(want)), 2.0 * own)
    print(f"{what}: got {got!r} want {want!r} dev {abs(got - want):.3e} float32 reference dev {own:.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound, what


def _check_grad(g, g64, what, g32=None):
    g64 = np.asarray(g64, dtype=np.float64)
    scale = np.abs(g64).max(initial=0.0)
    own = np.abs(np.asarray(g32, dtype=np.float64) - g64).max(initial=0.0) if g32 is not None else 0.0
    bound = max(1e-5 * scale, 2.0 * own)
    dev = np.abs(g.detach().double().cpu().numpy().reshape(g64.shape) - g64).max(initial=0.0)
    print(f"{what} grad: dev {dev:.3e} max|g64| {scale:.3e} float32 reference dev {own:.3e} bound {bound:.3e}")
    assert np.isfinite(dev) and dev <= bound, what


def _check_stats(stats, want, what, early=False):
    """early: the reference returned before its diagnostics, so the expectation carries the counts and the first three means only."""
    keys = EC.COUNT_KEYS + (EC.MEAN_KEYS[:3] if early else EC.MEAN_KEYS)
    assert set(keys) <= set(want), f"{what}: the expectation lacks {sorted(set(keys) - set(want))}"
    for key in EC.COUNT_KEYS:
        assert stats[key] == int(want[key]), f"{what} {key}: {stats[key]} != {want[key]}"
    for key in keys[len(EC.COUNT_KEYS):]:
        _check_loss(stats[key], want[key], f"{what} {key}")


def _fx_stats(fx, s=None):
    out = {k[5:]: float(np.atleast_1d(fx[k])[0 if s is None else s]) for k in fx.files if k.startswith("stat_")}
    return {k: v for k, v in out.items() if not np.isnan(v)}


def _run(emb, codes, metric, kw, factor=1.0):
    from frl_hip.losses import evt_soft_neighborhood_loss
    e = emb.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = evt_soft_neighborhood_loss(e, codes.to(DEV), metric, **kw)
    (factor * loss).backward()
    return loss.detach(), stats, e.grad


def _run_batched(emb, codes, seg, metric, kw, factor=1.0, **extra):
    from frl_hip.losses import evt_soft_neighborhood_loss_batched
    e = emb.detach().to(DEV).clone().requires_grad_(True)
    loss, stats = evt_soft_neighborhood_loss_batched(e, codes.to(DEV), seg, metric, **kw, **extra)
    (factor * loss.sum()).backward()
    return loss.detach(), stats, e.grad


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_single_call_matches_reference_fixture(golden_dir, metrics, name):
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, name)
    loss, stats, g = _run(emb, codes, metric, kw)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and g.dtype == torch.float32 and g.shape == emb.shape
    _check_loss(loss, fx["loss64"], name, fx["loss32"])
    _check_stats(stats, _fx_stats(fx), name, early=name == "d")
    assert torch.isfinite(g).all()
    _check_grad(g, fx["grad64"], name, fx["grad32"])
    assert "median_d_learned" not in stats and "mean_rank_confused" not in stats
    if name == "d":
        assert float(loss) == 0.0 and not g.any() and stats["n_anchors_valid"] == 3
    if name == "e":                                                      # the identical pairs: zero pair term, the rest of the rows as usual
        assert g[2].abs().max() > 0 and g[5].abs().max() > 0
    loss2, _, g2 = _run(emb, codes, metric, kw)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)               # identical bits from run to run


def test_batched_form_matches_fixture_and_single_calls(golden_dir, metrics):
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, "f")
    seg = fx["seg"].tolist()
    loss, stats, g = _run_batched(emb, codes, seg, metric, kw, reduction="sum")
    per = stats["per_segment_loss"]
    assert per.shape == (3,) and per.is_cuda and per.dtype == torch.float32 and float(loss) == float(per.sum())
    for s in range(3):
        _check_loss(per[s], fx["loss64"][s], f"f segment {s}", fx["loss32"][s])
        _check_stats(stats["per_segment"][s], _fx_stats(fx, s), f"f segment {s}", early=s == 1)
    _check_grad(g, fx["grad64"], "f", fx["grad32"])
    assert float(per[1]) == 0.0 and not g[seg[1]:seg[2]].any()
    assert stats["n_anchors_in"] == 181 and stats["n_anchors_valid"] == int(fx["stat_n_anchors_valid"].sum())
    for s in range(3):                                                   # the same rows through the single call: the same bits
        ls, ss, gs = _run(emb[seg[s]:seg[s + 1]], codes[seg[s]:seg[s + 1]], metric, kw)
        assert torch.equal(ls, per[s]) and torch.equal(gs, g[seg[s]:seg[s + 1]])
        assert ss == stats["per_segment"][s]
    loss2, _, g2 = _run_batched(emb, codes, seg, metric, kw, reduction="sum")
    assert torch.equal(loss, loss2) and torch.equal(g, g2)
    lm, _, _ = _run_batched(emb, codes, seg, metric, kw)                 # "mean": over all three segments, the zero one included
    assert float(lm) == float(per.sum() / 3)
    ln, _, _ = _run_batched(emb, codes, torch.tensor(seg), metric, kw, reduction="none")
    assert torch.equal(ln, per)


def test_empty_segments(golden_dir, metrics):
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, "a")
    la, _, ga = _run(emb, codes, metric, kw)
    loss, stats, g = _run_batched(emb, codes, [0, 0, 48, 48], metric, kw, reduction="none")
    assert loss.tolist() == [0.0, float(la), 0.0] and torch.equal(g, ga)
    assert [s["n_anchors_in"] for s in stats["per_segment"]] == [0, 48, 0]


def test_bfloat16_embeddings(golden_dir, metrics):
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, "a")
    emb16 = emb.to(torch.bfloat16)
    loss16, stats16, g16 = _run(emb16, codes, metric, kw)
    loss32, stats32, g32 = _run(emb16.float(), codes, metric, kw)
    assert loss16.dtype == torch.float32 and g16.dtype == torch.bfloat16
    assert torch.equal(loss16, loss32) and stats16 == stats32            # upcast on load: exactly the float32 path on the upcast inputs
    assert torch.equal(g16, g32.to(torch.bfloat16))


def test_upstream_factor_and_segment_weights(golden_dir, metrics):
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, "f")
    seg = fx["seg"].tolist()
    idx = EC.code_index(codes, sorted(metric.valid_codes))
    sw = torch.tensor([0.5, 2.0, 1.5])
    want_l, _, want_g = EC.evt_f64(emb, idx, metric._S, metric._freq_weights, seg, seg_weights=sw, upstream=[3.0 / 3] * 3, **kw)
    loss, stats, g = _run_batched(emb, codes, seg, metric, kw, factor=3.0, segment_weights=sw.to(DEV))
    _check_loss(loss, sum(w * lo for w, lo in zip(sw.tolist(), want_l)) / 3, "weighted mean")
    _check_grad(g, want_g.numpy(), "3 * weighted mean")
    _, _, g7 = _run(emb[:48], codes[:48], metric, kw, factor=-7.0)
    _check_grad(g7, -7.0 * fx["grad64"][:48], "upstream -7", -7.0 * fx["grad32"][:48])
    _, _, g0 = _run_batched(emb, codes, seg, metric, kw, segment_weights=torch.zeros(3, device=DEV))
    assert not g0.any()


def test_wide_shape_matches_the_restatement(metrics):
    metric = metrics["b"]
    kept = sorted(metric.valid_codes)
    emb = EC.make_embeddings(130, 256, 431, scale=0.125)
    codes = EC.make_codes(130, 432, kept, [-5, 7999, 0], 0.1)
    kw = dict(tau_ref=0.3, tau_learned=0.7, min_valid_anchors=4)
    want_l, want_s, want_g = EC.evt_f64(emb, EC.code_index(codes, kept), metric._S, metric._freq_weights, [0, 65, 130], **kw)
    loss, stats, g = _run_batched(emb, codes, [0, 65, 130], metric, kw, reduction="none")
    for s in range(2):
        _check_loss(loss[s], want_l[s], f"D=256 segment {s}")
        _check_stats(stats["per_segment"][s], want_s[s], f"D=256 segment {s}")
    _check_grad(g, want_g.numpy(), "D=256")
    loss2, _, g2 = _run_batched(emb, codes, [0, 65, 130], metric, kw, reduction="none")
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


def test_long_segment_matches_the_restatement(metrics):
    # one segment of 300 rows over three codes: more rows than the 256 threads that sum a segment's rows, ten row tiles, five column tiles
    metric = metrics["b"]
    kept = sorted(metric.valid_codes)
    emb = EC.make_embeddings(300, 4, 433)
    codes = EC.make_codes(300, 434, kept[:3])
    kw = dict(tau_ref=0.3, tau_learned=0.7, min_valid_anchors=4)
    want_l, want_s, want_g = EC.evt_f64(emb, EC.code_index(codes, kept), metric._S, metric._freq_weights, [0, 300], **kw)
    loss, stats, g = _run(emb, codes, metric, kw)
    assert stats["n_rows_active"] == 300
    _check_loss(loss, want_l[0], "N=300 D=4")
    _check_stats(stats, want_s[0], "N=300 D=4")
    _check_grad(g, want_g.numpy(), "N=300 D=4")
    loss2, _, g2 = _run(emb, codes, metric, kw)
    assert torch.equal(loss, loss2) and torch.equal(g, g2)


def test_out_of_range_index_is_unknown_and_flagged(golden_dir, metrics):
    from frl_hip import ops
    fx, metric, kw, emb, codes = _case(golden_dir, metrics, "a")
    idx = metric.code_index(codes.to(DEV))
    hi, lo = idx.clone(), idx.clone()
    hi[7], lo[7] = metric.n_codes, -1
    seg_host = torch.tensor([0, 48], dtype=torch.int32)
    args = (metric._S, metric._freq_weights, seg_host.to(DEV), seg_host)
    ops.index_errors()
    out_lo = ops.evt_soft_nbr_fwd(emb.to(DEV), lo, *args)
    assert not ops.index_errors()
    out_hi = ops.evt_soft_nbr_fwd(emb.to(DEV), hi, *args)
    assert ops.index_errors() and torch.equal(out_hi[0], out_lo[0]) and torch.equal(out_hi[2], out_lo[2])
    ones = torch.ones(1, device=DEV)
    assert torch.equal(ops.evt_soft_nbr_bwd(emb.to(DEV), hi, *args, 0.5, 0.5, out_hi[2], out_hi[0], ones),
                       ops.evt_soft_nbr_bwd(emb.to(DEV), lo, *args, 0.5, 0.5, out_lo[2], out_lo[0], ones))
    from frl_hip._lib import FrlHipError
    with pytest.raises(FrlHipError, match="segment offsets"):
        ops.evt_soft_nbr_fwd(emb.to(DEV), lo, metric._S, metric._freq_weights, seg_host.to(DEV), torch.tensor([0, 40], dtype=torch.int32))
