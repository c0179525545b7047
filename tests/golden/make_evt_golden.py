"""Writes the EVT soft-neighbourhood fixtures by running the REFERENCE's EvtDiffusionMetric and evt_soft_neighborhood_loss
(frl/losses/evt_soft_neighborhood.py), importable where the reference tree is present (they need torch, numpy and pandas).  The reference
does not travel; only these files do.

evt_confusion_small.csv: a synthetic contingency table of 14 integer codes in the layout of the combined EVT table: the `Row Totals` and
`Percent Row Agreement` columns, the `Column Totals` and `Percent Column Agreement` rows, one code with fewer than 30 samples and one whose
row and column are all zero.  evt_counts_small.json: code -> pixel count with string keys; one code sits below min_count = 100, one code
of the counts is absent from the table and one code of the table is absent from the counts.

evt_metric_{a,b,c}.npz: the kept codes, S [K, K] float32 and the frequency weights [K] float32 of the reference's metric with the
defaults (a), laplace_smoothing = 0.1 and diffusion_steps = 3 (b), binary_threshold = 0.05 (c).

evt_{a..f}.npz: the seeded inputs on a 2^-8 grid (tests/evt_cases.py draws them: emb, codes, seg, the parameters), the metric's name,
loss64 / the stats / grad64 from the reference in float64, loss32 / grad32 from the same function in float32 on the CPU (how far the
reference itself sits from float64).  Case f holds three segments; its values come from three reference calls (loss64, loss32 and every
stat_* are [3] arrays, NaN where the reference's early return has no such key).

    python tests/golden/make_evt_golden.py        (in the build container, FRL_REFERENCE or /root/reference present)
"""
import csv
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.environ.get("FRL_REFERENCE", "/root/reference"), "frl"))
sys.path.insert(0, os.path.dirname(HERE))
from losses.evt_soft_neighborhood import EvtDiffusionMetric, evt_soft_neighborhood_loss  # noqa: E402

import evt_cases as EC  # noqa: E402

CSV = os.path.join(HERE, "evt_confusion_small.csv")
COUNTS = os.path.join(HERE, "evt_counts_small.json")
CODES = [7011, 7016, 7023, 7055, 7070, 7102, 7125, 7147, 7171, 7192, 7232, 7292, 7301, 7324]
FEW, EMPTY, RARE, NO_COUNT, NOT_IN_TABLE = 7171, 7232, 7292, 7301, 7999   # < 30 samples | all-zero | < min_count pixels | no count | no row


def write_table():
    g = np.random.default_rng(500)
    n = len(CODES)
    table = np.zeros((n, n), dtype=np.int64)
    for a in range(n):
        table[a, a] = int(g.integers(40, 400))
        for b in range(n):
            near = abs(a - b) in (1, 2) or (a * 5 + b * 3) % 11 == 0    # neighbours in the list confuse, plus a scatter; not symmetric
            if a != b and near and g.random() < 0.7:
                table[a, b] = int(g.integers(1, 60))
    few, empty = CODES.index(FEW), CODES.index(EMPTY)
    table[few, :] = 0
    table[few, few], table[few, few - 1] = 9, 4                         # 13 samples
    table[empty, :] = 0
    table[:, empty] = 0
    with open(CSV, "w", newline="") as fh:
        out = csv.writer(fh)
        out.writerow(["", *CODES, "Row Totals", "Percent Row Agreement"])
        for a, code in enumerate(CODES):
            total = int(table[a].sum())
            out.writerow([code, *table[a].tolist(), total, round(100.0 * table[a, a] / total, 2) if total else 0.0])
        col = table.sum(axis=0)
        out.writerow(["Column Totals", *col.tolist(), int(table.sum()), ""])
        out.writerow(["Percent Column Agreement", *[round(100.0 * table[b, b] / col[b], 2) if col[b] else 0.0 for b in range(n)], "",
                      round(100.0 * np.trace(table) / table.sum(), 2)])
    counts = {str(c): int(g.integers(300, 4000)) for c in CODES if c != NO_COUNT}
    counts[str(CODES[0])] = 250000                                      # a dominant type: the others' weights rise towards the cap
    counts[str(CODES[5])] = 120                                         # and a scarce one that passes min_count: its weight is capped
    counts[str(RARE)] = 50
    counts[str(NOT_IN_TABLE)] = 5000
    with open(COUNTS, "w") as fh:
        json.dump(counts, fh, indent=0, sort_keys=True)
    return counts


def write_metrics(counts):
    metrics = {}
    for name, kw in EC.METRIC_SETTINGS.items():
        m = EvtDiffusionMetric(CSV, counts, **kw)
        kept = sorted(m.valid_codes)
        assert [m._code_to_idx[c] for c in kept] == list(range(len(kept)))
        np.savez_compressed(os.path.join(HERE, f"evt_metric_{name}.npz"), codes=np.asarray(kept, dtype=np.int64), S=m._S.numpy(),
                            weights=m._freq_weights.numpy(), **{k: np.float64(v) for k, v in kw.items()})
        print("metric", name, kw, "K", len(kept), "asymmetry", float((m._S - m._S.T).abs().max()), "weights", m._freq_weights.tolist())
        metrics[name] = (m, kept)
    return metrics


def run_reference(metric, emb, codes, dtype, kw):
    z = emb.clone().to(dtype).requires_grad_(True)
    loss, stats = evt_soft_neighborhood_loss(z, codes, metric, **kw)
    loss.backward()
    return float(loss.detach()), stats, (torch.zeros_like(z) if z.grad is None else z.grad).numpy()


def write_case(name, metrics):
    metric, kept = metrics[EC.CASE_METRIC[name]]
    dropped = [c for c in CODES if c not in kept] + [NOT_IN_TABLE, -3, 0, 9001]
    case = EC.make_case(name, kept, dropped)
    kw = {k: case[k] for k in ("tau_ref", "tau_learned", "min_valid_anchors")}
    seg = case["seg"]
    res = {dt: [run_reference(metric, case["emb"][a:b], case["codes"][a:b], dt, kw) for a, b in zip(seg[:-1], seg[1:])]
           for dt in (torch.float64, torch.float32)}
    single = len(seg) == 2
    pick = (lambda v: v[0]) if single else (lambda v: np.asarray(v))
    arrays = dict(emb=case["emb"].numpy(), codes=case["codes"].numpy(), seg=np.asarray(seg, dtype=np.int64), metric=np.str_(EC.CASE_METRIC[name]),
                  **{k: np.float64(v) for k, v in kw.items()})
    arrays["loss64"] = pick([np.float64(r[0]) for r in res[torch.float64]])
    arrays["loss32"] = pick([np.float64(r[0]) for r in res[torch.float32]])
    arrays["grad64"] = np.concatenate([r[2] for r in res[torch.float64]])
    arrays["grad32"] = np.concatenate([r[2] for r in res[torch.float32]])
    for key in sorted({k for r in res[torch.float64] for k in r[1]}):
        arrays["stat_" + key] = pick([np.float64(r[1].get(key, np.nan)) for r in res[torch.float64]])
    path = os.path.join(HERE, f"evt_{name}.npz")
    np.savez_compressed(path, **arrays)
    g64, g32 = arrays["grad64"], arrays["grad32"]
    gmax = max(np.abs(g64).max(), 1e-30)
    print(name, tuple(case["emb"].shape), "loss64", arrays["loss64"], "valid", arrays["stat_n_anchors_valid"], "active", arrays["stat_n_rows_active"],
          "f32 loss dev", np.abs(arrays["loss32"] - arrays["loss64"]).max(), "f32 grad dev / max", np.abs(g32 - g64).max() / gmax,
          "finite", bool(np.isfinite(g64).all()), os.path.getsize(path), "bytes")


def main():
    metrics = write_metrics(write_table())
    for name in EC.CASES:
        write_case(name, metrics)


if __name__ == "__main__":
    main()
