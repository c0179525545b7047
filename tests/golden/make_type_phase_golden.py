"""Writes tests/golden/type_baseline_{a,b,c,d,e,w}.npz and tests/golden/leakage_{a..d}.npz.

The reference has no callable for either piece: the type-local baseline (frl/training/representation/step.py:922-928) and the
phase-type leakage loss (step.py:1015-1021) are inline in process_batch.  So this maker evaluates those formulas with stock torch ops in
float64 (matmul, fill_diagonal_, topk, indexing, mean; autograd for the gradient), written here from the formulas: the fixtures pin the
package to the FORMULA, not to a reference function, and this script needs no reference checkout.

Inputs are regenerated from seeds by tests/type_phase_cases.py; the fixtures hold expected outputs only.
type_baseline_*: idx int16 [N, k], s_hat64 [N, C], and the shape and seed of the case.
leakage_*: loss64, dh64 = d loss / d h of the rows `rows` (every row, or every 4th and the last in b), dh_max = max |dh| over all rows.

Each baseline case asserts that its seed is the first of 0..31 without a tie among any row's k + 1 largest similarities and that the
float32 similarities equal the float64 ones; each leakage case that loss64 >= 0.1 (the direction C / loss is ill-conditioned near zero).

    python tests/golden/make_type_phase_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import type_phase_cases as TP  # noqa: E402


def write_baseline(name):
    n, kw, k_nbrs, t, c, denom, seed = TP.BASELINE_CASES[name]
    z_k, spec, _ = TP.baseline_inputs(name)
    assert seed == TP.first_tie_free_seed(n, kw, k_nbrs, denom), f"{name}: the seed of the case table is not the first tie-free one"
    sim32 = z_k @ z_k.T
    z64, spec64 = z_k.double(), spec.double()
    sim = z64 @ z64.T
    assert torch.equal(sim32.double(), sim), f"{name}: a float32 similarity is not exact"
    sim.fill_diagonal_(float("-inf"))
    k = min(k_nbrs, n - 1)
    assert TP.tied_rows(z_k, k) == 0
    idx = sim.topk(k, dim=1).indices                                     # no ties: the order is the only one
    s_hat = spec64.mean(dim=1)[idx].mean(dim=1)
    assert not bool((idx == torch.arange(n).unsqueeze(1)).any())
    path = os.path.join(HERE, f"type_baseline_{name}.npz")
    np.savez_compressed(path, idx=idx.numpy().astype(np.int16), s_hat64=s_hat.numpy(), shape=np.array([n, kw, k, t, c], dtype=np.int64),
                        seed=np.int64(seed))
    print(f"type_baseline_{name}", (n, kw, k, t, c), "seed", seed, os.path.getsize(path), "bytes")


def write_leakage(name):
    n, p, dz, seed, offset, every = TP.LEAKAGE_CASES[name]
    h, z = TP.leakage_inputs(name)
    h64 = h.double().requires_grad_(True)
    z_sg = z.double().detach()
    h_c = h64 - h64.mean(0, keepdim=True)
    z_c = z_sg - z_sg.mean(0, keepdim=True)
    cross_cov = h_c.T @ z_c / max(n - 1, 1)
    loss = cross_cov.pow(2).sum().sqrt()
    loss.backward()
    loss = loss.detach()
    assert float(loss) >= 0.1, f"{name}: loss64 {float(loss)} < 0.1"
    if offset >= 10:                                                     # the pivot case: every column mean far from zero
        assert float((h.double().mean(0).abs() / h.double().std(0)).min()) > 0.5 * offset
        assert float((z.double().mean(0).abs() / z.double().std(0)).min()) > 0.5 * offset
    dh = h64.grad
    rows = TP.kept_rows(n, every)
    path = os.path.join(HERE, f"leakage_{name}.npz")
    np.savez_compressed(path, loss64=np.float64(float(loss)), rows=rows.numpy(), dh64=dh[rows].numpy(), dh_max=np.float64(float(dh.abs().max())),
                        shape=np.array([n, p, dz], dtype=np.int64))
    print(f"leakage_{name}", (n, p, dz), "loss64", float(loss), "max|dh|", float(dh.abs().max()), os.path.getsize(path), "bytes")


def main():
    for name in TP.BASELINE_CASES:
        write_baseline(name)
    for name in TP.LEAKAGE_CASES:
        write_leakage(name)


if __name__ == "__main__":
    main()
