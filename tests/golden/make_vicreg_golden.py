"""Writes tests/golden/vicreg_{a..e}.npz by running the REFERENCE's variance_covariance_loss (frl/losses/variance_covariance.py:14-88,
importable where the reference tree is present: it needs torch only).  The reference does not travel; only these arrays do:
the seeded float32 inputs, the weights / target / eps, loss64 (total, variance, covariance) and grad64 = d total / dX evaluated in
float64, and loss32 / grad32 from the same function evaluated in float32 on the CPU (how far the reference itself sits from float64).

    python tests/golden/make_vicreg_golden.py        (in the build container, /root/reference present)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference/frl")
from losses.variance_covariance import variance_covariance_loss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def rows(n, d, seed, offset=0.0, scale=1.0, mix=0.5):
    g = torch.Generator().manual_seed(seed)
    w = torch.eye(d, dtype=torch.float64) + mix * torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
    return ((torch.randn(n, d, generator=g, dtype=torch.float64) @ w) * scale + offset).float()


def grid(x):
    """Inputs on a 2^-8 grid: exactly float32- (and float64-) representable, and the stored array compresses below the size limit."""
    return (torch.round(x.double() * 256.0) / 256.0).float()


def case_b():
    x = rows(400, 12, 102, mix=0.3)
    x[:, :6] *= 0.4                                   # std below the target on half of the columns: the hinge is active on those only
    x[:, 6:] *= 1.8
    return x


def case_e():
    x = rows(2, 20, 105)
    x[:, 3] = 0.75                                    # constant column: std = sqrt(eps), finite hinge gradient
    return x


CASES = {
    "a": (grid(rows(300, 64, 101)), dict(variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4)),
    "b": (grid(case_b()), dict(variance_weight=25.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4)),
    "c": (grid(rows(150, 128, 103)), dict(variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4)),
    "d": (grid(rows(257, 64, 104, offset=50.0, scale=0.5, mix=0.0)), dict(variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4)),
    "e": (grid(case_e()), dict(variance_weight=0.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4)),
}


def evaluate(x, kw, dtype):
    t = x.detach().clone().to(dtype).requires_grad_(True)
    out = variance_covariance_loss(t, **kw)
    out[0].backward()
    return np.array([float(o.detach()) for o in out], dtype=np.float64), t.grad.numpy()


def main():
    for name, (x, kw) in CASES.items():
        l64, g64 = evaluate(x, kw, torch.float64)
        l32, g32 = evaluate(x, kw, torch.float32)
        path = os.path.join(HERE, f"vicreg_{name}.npz")
        np.savez_compressed(path, x=x.numpy(), loss64=l64, grad64=g64, loss32=l32, grad32=g32,
                            **{k: np.float64(v) for k, v in kw.items()})
        print(name, tuple(x.shape), l64, "f32 loss dev", np.abs(l32 - l64).max(), "f32 grad dev / max",
              np.abs(g32 - g64).max() / max(np.abs(g64).max(), 1e-30), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
