"""EVT soft-neighbourhood loss, host side: the metric port against the fixtures the REFERENCE's EvtDiffusionMetric wrote
(tests/golden/make_evt_golden.py), the device-free code lookup, the float64 restatement (tests/evt_cases.py) against the reference's
loss64 / grad64, the fixtures themselves and the public surface (signatures, declarations, no CPU fallback)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import evt_cases as EC
from frl_hip.losses import EvtDiffusionMetric, evt_soft_neighborhood_loss, evt_soft_neighborhood_loss_batched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fx(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"{name}.npz"))


def _metric(golden_dir, name, **extra):
    with open(os.path.join(golden_dir, "evt_counts_small.json")) as fh:
        counts = json.load(fh)
    return EvtDiffusionMetric(os.path.join(golden_dir, "evt_confusion_small.csv"), counts, **{**EC.METRIC_SETTINGS[name], **extra})


def _close(got, want, what, rel=1e-12):
    """Relative to the largest expected entry; an all-zero expectation is met exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    dev, scale = np.abs(got - want).max(initial=0.0), np.abs(want).max(initial=0.0)
    assert np.isfinite(dev) and dev <= rel * scale, f"{what}: dev {dev:.3e} of {scale:.3e}"


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_metric_port_reproduces_the_reference_metric(golden_dir, name):
    fx, m = _fx(golden_dir, f"evt_metric_{name}"), _metric(golden_dir, name)
    assert sorted(m.valid_codes) == fx["codes"].tolist() and m.n_codes == len(fx["codes"])
    assert m._S.dtype == torch.float32 and np.array_equal(m._S.numpy(), fx["S"])
    assert m._freq_weights.dtype == torch.float32 and np.array_equal(m._freq_weights.numpy(), fx["weights"])
    assert np.abs(fx["S"] - fx["S"].T).max() > 0.05                      # the diffused similarity is not symmetric
    assert fx["weights"].max() == 10.0 and fx["weights"].min() < 0.01    # the cap, and the dominant type


def test_metric_table_and_counts_are_what_they_claim(golden_dir):
    with open(os.path.join(golden_dir, "evt_confusion_small.csv")) as fh:
        lines = fh.read().splitlines()
    assert lines[0].endswith("Row Totals,Percent Row Agreement") and len(lines) == 1 + 14 + 2
    assert lines[-2].startswith("Column Totals,") and lines[-1].startswith("Percent Column Agreement,")
    with open(os.path.join(golden_dir, "evt_counts_small.json")) as fh:
        counts = json.load(fh)
    assert all(isinstance(k, str) for k in counts) and sum(v < 100 for v in counts.values()) == 1
    table_codes = {int(ln.split(",")[0]) for ln in lines[1:15]}
    assert len({int(k) for k in counts} - table_codes) == 1 and len(table_codes - {int(k) for k in counts}) == 1
    kept = set(_fx(golden_dir, "evt_metric_a")["codes"].tolist())
    assert len(kept) == 10 and kept < table_codes                       # too few pixels, too few samples, the all-zero row, no count
    rows = {int(ln.split(",")[0]): [float(v) for v in ln.split(",")[1:15]] for ln in lines[1:15]}
    assert sum(1 for r in rows.values() if sum(r) == 0) == 1 and sum(1 for r in rows.values() if 0 < sum(r) < 30) == 1


def test_metric_filters_and_error(golden_dir):
    with pytest.raises(ValueError, match="Fewer than 2 EVT codes"):
        _metric(golden_dir, "a", min_count=10 ** 9)
    with pytest.raises(ValueError, match="Fewer than 2 EVT codes"):
        _metric(golden_dir, "a", min_confusion_samples=10 ** 6)
    loose = _metric(golden_dir, "a", min_confusion_samples=0, min_count=0)
    assert loose.n_codes == 13                                           # every table code that has a count, the all-zero row included
    s = loose._S.double()
    _close(s.sum(dim=1).numpy(), np.ones(13), "rows of a power of a stochastic matrix sum to 1", rel=1e-6)
    assert inspect.signature(EvtDiffusionMetric.__init__).parameters["max_weight"].default == 10.0
    sig = inspect.signature(EvtDiffusionMetric.__init__)
    assert list(sig.parameters)[1:] == ["confusion_csv", "code_counts", "min_count", "min_confusion_samples", "diffusion_steps",
                                        "laplace_smoothing", "binary_threshold", "max_weight"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [100, 30, 2, 0.0, 0.0, 10.0]


def test_code_index_agrees_with_the_dict_lookup(golden_dir):
    m = _metric(golden_dir, "a")
    kept = sorted(m.valid_codes)
    g = torch.Generator().manual_seed(7)
    codes = torch.cat([torch.randint(6990, 7340, (4000,), generator=g), torch.tensor(kept), torch.tensor([-1, -7011, 0, kept[-1] + 1, 10 ** 9,
                                                                                                             -10 ** 9, kept[0] - 1])])
    want = EC.code_index(codes, kept)
    for dtype in (torch.int64, torch.int32):
        got = m.code_index(codes.to(dtype))
        assert got.dtype == torch.int32 and torch.equal(got.to(torch.int64), want)
    assert (want >= 0).sum() > len(kept) and (want < 0).sum() > 1000
    assert m.code_index(codes.reshape(1, -1)).shape == (1, codes.numel())
    d_ref, valid = m.reference_distances(codes[:300])
    w = m.anchor_weights(codes[:300])
    ix = want[:300]
    assert torch.equal(valid, ix >= 0) and d_ref.dtype == torch.float32 and w.dtype == torch.float32
    for i in range(0, 300, 7):                                           # what the reference's per-anchor lookups return
        assert float(w[i]) == (float(m._freq_weights[ix[i]]) if ix[i] >= 0 else 0.0)
        for j in range(0, 300, 11):
            known = ix[i] >= 0 and ix[j] >= 0
            assert float(d_ref[i, j]) == (float(1.0 - m._S[ix[i], ix[j]]) if known else 1.0)
    assert m.to("cpu") is m


def _case(golden_dir, name):
    fx = _fx(golden_dir, f"evt_{name}")
    mx = _fx(golden_dir, f"evt_metric_{str(fx['metric'])}")
    kw = dict(tau_ref=float(fx["tau_ref"]), tau_learned=float(fx["tau_learned"]), min_valid_anchors=int(fx["min_valid_anchors"]))
    idx = EC.code_index(fx["codes"], mx["codes"])
    return fx, mx, kw, torch.from_numpy(fx["emb"]), idx, torch.from_numpy(mx["S"]), torch.from_numpy(mx["weights"])


@pytest.mark.parametrize("name", EC.CASES)
def test_restatement_matches_reference_fixture(golden_dir, name):
    fx, mx, kw, emb, idx, S, w = _case(golden_dir, name)
    losses, stats, grad = EC.evt_f64(emb, idx, S, w, fx["seg"], **kw)
    seg = fx["seg"].tolist()
    for s, (lo, want) in enumerate(zip(losses, np.atleast_1d(fx["loss64"]))):          # each segment against its own value
        _close(lo, want, f"{name} loss, segment {s}")
        _close(grad.numpy()[seg[s]:seg[s + 1]], fx["grad64"][seg[s]:seg[s + 1]], f"{name} grad, segment {s}")
    assert np.isfinite(fx["grad64"]).all() and fx["grad64"].dtype == np.float64
    early = {"d": [0], "f": [1]}.get(name, [])                           # the segments where the reference returns early, with six keys
    for s, st in enumerate(stats):
        have = {k for k in EC.COUNT_KEYS + EC.MEAN_KEYS if "stat_" + k in fx.files and not np.isnan(np.atleast_1d(fx["stat_" + k])[s])}
        assert have == set(EC.COUNT_KEYS + (EC.MEAN_KEYS[:3] if s in early else EC.MEAN_KEYS)), f"{name} segment {s}: fixture keys {sorted(have)}"
        for key in EC.COUNT_KEYS + EC.MEAN_KEYS:
            if key not in have:
                continue
            want = np.atleast_1d(fx["stat_" + key])[s]
            if key in EC.COUNT_KEYS:
                assert st[key] == int(want), f"{name} {key}"
            else:
                _close(st[key], want, f"{name} {key}", rel=2.0 ** -22 if key == "n_confused_pairs" else 1e-12)   # (averaged in float32 there)
    assert os.path.getsize(os.path.join(golden_dir, f"evt_{name}.npz")) < 256 * 1024


def test_fixture_cases_are_the_ones_they_claim(golden_dir):
    fx = {c: _case(golden_dir, c) for c in EC.CASES}
    assert {c: fx[c][0]["emb"].shape for c in EC.CASES} == {"a": (48, 64), "b": (200, 64), "c": (37, 12), "d": (9, 64), "e": (16, 64), "f": (181, 64)}
    assert (fx["a"][4] >= 0).all()
    unknown = (fx["b"][4] < 0).float().mean()
    assert 0.08 < unknown < 0.25 and str(fx["b"][0]["metric"]) == "b" and (fx["b"][0]["codes"] < 0).any()
    ic = fx["c"][4]
    assert str(fx["c"][0]["metric"]) == "c" and (ic == ic[0]).sum() == 36 and int(fx["c"][0]["stat_n_rows_active"]) == 1
    d = fx["d"][0]
    assert (fx["d"][4] >= 0).sum() == 3 and float(d["loss64"]) == 0.0 and not d["grad64"].any()
    e = fx["e"][0]["emb"]
    assert (e[2] == e[5]).all() and (e[9] == e[12]).all() and len({int(fx["e"][4][k]) for k in (2, 5)}) == 2 and e.shape[0] <= 25
    f = fx["f"][0]
    assert f["seg"].tolist() == [0, 48, 51, 181] and f["loss64"].shape == (3,) and f["loss64"][1] == 0.0 and not f["grad64"][48:51].any()
    for c in EC.CASES:
        emb = fx[c][0]["emb"]
        assert emb.dtype == np.float32 and (emb * 256 == np.round(emb * 256)).all()


def test_restated_gradient_matches_finite_differences(golden_dir):
    fx, mx, kw, emb, idx, S, w = _case(golden_dir, "a")
    _, _, grad = EC.segment_f64(emb, idx, S, w, **kw)
    e = emb.double()
    h = 1e-6
    for i, c in [(0, 0), (3, 17), (20, 63), (47, 5), (31, 40)]:
        up, dn = e.clone(), e.clone()
        up[i, c] += h
        dn[i, c] -= h
        fd = (EC.segment_f64(up, idx, S, w, **kw)[0] - EC.segment_f64(dn, idx, S, w, **kw)[0]) / (2 * h)
        assert abs(fd - float(grad[i, c])) <= 1e-7 * float(grad.abs().max()) + 1e-11, (i, c, fd, float(grad[i, c]))


def test_header_and_loader_declare_the_entry_points():
    from frl_hip import _lib
    with open(os.path.join(ROOT, "include", "frl_hip.h")) as fh:
        header = fh.read()
    for name in ("frl_evt_soft_nbr_fwd", "frl_evt_soft_nbr_bwd"):
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl is not None, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == decl.group(1).count(",") + 1


def test_signatures_match_reference():
    sig = inspect.signature(evt_soft_neighborhood_loss)
    assert list(sig.parameters) == ["embeddings", "evt_codes", "metric", "tau_ref", "tau_learned", "min_valid_anchors"]
    assert [p.default for p in list(sig.parameters.values())[3:]] == [0.5, 0.5, 4]
    sig = inspect.signature(evt_soft_neighborhood_loss_batched)
    assert list(sig.parameters) == ["embeddings", "evt_codes", "segment_offsets", "metric", "tau_ref", "tau_learned", "min_valid_anchors",
                                    "segment_weights", "reduction"]
    assert [p.default for p in list(sig.parameters.values())[4:]] == [0.5, 0.5, 4, None, "mean"]


def test_cpu_tensors_are_refused_and_arguments_checked(golden_dir):
    from frl_hip._lib import FrlHipError
    m = _metric(golden_dir, "a")
    emb, codes = torch.randn(12, 8), torch.tensor(sorted(m.valid_codes))[torch.arange(12) % m.n_codes]
    with pytest.raises(FrlHipError, match="GPU"):
        evt_soft_neighborhood_loss(emb, codes, m)
    with pytest.raises(FrlHipError, match="GPU"):
        evt_soft_neighborhood_loss_batched(emb, codes, [0, 5, 12], m)
    with pytest.raises(ValueError, match="256"):
        evt_soft_neighborhood_loss(torch.randn(12, 257), codes, m)
    with pytest.raises(ValueError, match="segment_offsets"):
        evt_soft_neighborhood_loss_batched(emb, codes, [0, 7, 5, 12], m)
    with pytest.raises(ValueError, match="segment_offsets"):
        evt_soft_neighborhood_loss_batched(emb, codes, [0, 5, 11], m)
    with pytest.raises(ValueError, match="reduction"):
        evt_soft_neighborhood_loss_batched(emb, codes, [0, 12], m, reduction="median")
    with pytest.raises(ValueError, match="segment_weights"):
        evt_soft_neighborhood_loss_batched(emb, codes, [0, 5, 12], m, segment_weights=torch.ones(3))
