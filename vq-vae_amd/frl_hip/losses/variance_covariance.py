"""VICReg variance-covariance loss on the HIP path: `variance_covariance_loss`, `variance_loss` and `covariance_loss` with the
reference's signatures and semantics (frl/losses/variance_covariance.py:14-155; callers frl/training/representation/step.py:551,623).

    mu = mean_rows(X), Xc = X - mu, cov = Xc^T Xc / (N-1), std_j = sqrt(cov_jj + eps)
    variance_loss   = mean_j relu(variance_target - std_j)
    covariance_loss = sum_{j != k} cov_jk^2 / D
    total           = variance_weight * variance_loss + covariance_weight * covariance_loss

Forward: one pass over the rows (column sums and the D x D Gram about a pivot, the mean of the first 64 rows, per-workgroup f32 slabs summed in a fixed order) and a
one-workgroup finalise.  Backward: one kernel, dX = (X - mu) A with
    A = (4 cw / (D (N-1))) offdiag(cov) - diag(vw 1[std_j < variance_target] / (D (N-1) std_j)),
where cw / vw fold the upstream gradients of all three outputs, read on the device (no host sync: a captured step replays it).  Loss and
gradient are bit-reproducible.  Rows are float32 or bfloat16, 1 <= D <= 128; the statistics and the three returned losses are float32
whatever the row dtype (the reference returns the row dtype), the gradient has the dtype of the rows.  N < 2 returns three float32
zeros and launches nothing.
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops


class _VicRegFn(Function):
    @staticmethod
    def forward(ctx, x, vw, cw, target, eps):
        losses, cov, centre = ops.vicreg_fwd(x, vw, cw, target, eps, want_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(x, cov, centre)
        ctx.hp = (vw, cw, target, eps)
        return losses[0], losses[1], losses[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_total, g_var, g_cov):
        x, cov, centre = ctx.saved_tensors
        g3 = torch.stack([g_total.reshape(()), g_var.reshape(()), g_cov.reshape(())]).to(torch.float32)
        return ops.vicreg_bwd(x, cov, centre, g3, *ctx.hp), None, None, None, None


def _rows(embeddings: torch.Tensor) -> torch.Tensor:
    if embeddings.dim() != 2:
        raise ValueError(f"Expected 2D tensor [N, D], got shape {embeddings.shape}")
    return embeddings


def _zero(embeddings: torch.Tensor) -> torch.Tensor:
    return torch.tensor(0.0, device=embeddings.device, dtype=torch.float32)      # float32 like every N >= 2 result


def _apply(embeddings, vw, cw, target, eps):
    x = embeddings if embeddings.dtype in (torch.float32, torch.bfloat16) else embeddings.float()
    return _VicRegFn.apply(x.contiguous(), float(vw), float(cw), float(target), float(eps))


def variance_covariance_loss(embeddings: torch.Tensor, variance_weight: float = 1.0, covariance_weight: float = 1.0,
                             variance_target: float = 1.0, eps: float = 1e-4) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """embeddings [N, D] -> (total_loss, variance_loss, covariance_loss), each differentiable."""
    _rows(embeddings)
    if embeddings.shape[0] < 2:                       # no meaningful statistics (the reference returns the same three zeros)
        zero = _zero(embeddings)
        return zero, zero, zero
    return _apply(embeddings, variance_weight, covariance_weight, variance_target, eps)


def variance_loss(embeddings: torch.Tensor, target: float = 1.0, eps: float = 1e-4) -> torch.Tensor:
    """Only the variance component: mean_j relu(target - std_j)."""
    _rows(embeddings)
    if embeddings.shape[0] < 2:
        return _zero(embeddings)
    return _apply(embeddings, 1.0, 0.0, target, eps)[1]


def covariance_loss(embeddings: torch.Tensor, eps: float = 1e-4) -> torch.Tensor:
    """Only the covariance component: sum_{j != k} cov_jk^2 / D (eps is accepted for the reference's signature and unused, as there)."""
    _rows(embeddings)
    if embeddings.shape[0] < 2:
        return _zero(embeddings)
    return _apply(embeddings, 0.0, 1.0, 1.0, eps)[2]
