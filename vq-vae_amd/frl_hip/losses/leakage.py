"""Phase-type leakage loss on the HIP path: the Frobenius norm of the cross-covariance between the time-averaged pre-FiLM bottleneck
output h [N, P] and the stop-gradient type embedding z_type [N, Dz] (frl/training/representation/step.py:1008-1025, inline in
process_batch).

    h_c = h - mean_rows(h), z_c = z - mean_rows(z), C = h_c^T z_c / max(N - 1, 1), loss = sqrt(sum C^2)
    d loss / d h[n, p] = g * sum_d z_c[n, d] C[p, d] / (max(N - 1, 1) * loss)

Forward: one pass over the rows (cross moments about a pivot, the mean of the first 64 rows, per-workgroup f32 slabs summed in a fixed
order) and a one-workgroup finalise in double.  Backward: one kernel; the upstream factor is read on the device (no host sync: a captured
step replays it).  z_type is detached inside: the gradient goes to h only.  Loss and gradient are bit-reproducible.  Rows are float32 or
bfloat16 each, P <= 64, Dz <= 128; the loss is float32, the gradient has the dtype of h.

Deviation from the reference: where the loss is exactly zero (N = 1, constant columns, exact orthogonality) the gradient is ZERO here;
the reference's autograd returns NaN there (the derivative of sqrt at 0).
"""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops


class _LeakageFn(Function):
    @staticmethod
    def forward(ctx, h, z):
        stats, cmat, centre = ops.leakage_fwd(h, z, want_grad=ctx.needs_input_grad[0])
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(z, cmat, centre, stats)
            ctx.h_meta = (h.shape[1], h.dtype)
        return stats[0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, cmat, centre, stats = ctx.saved_tensors
        p, dtype = ctx.h_meta
        return ops.leakage_bwd(z, cmat, centre, stats, g.reshape(1).to(torch.float32).contiguous(), p, dtype), None


def phase_type_leakage_loss(h: torch.Tensor, z_type: torch.Tensor) -> torch.Tensor:
    """h [N, P <= 64], z_type [N, Dz <= 128], float32 or bfloat16 each, on the GPU -> 0-dim float32 loss, differentiable in h only
    (z_type is detached; dh has h's dtype; zero, not NaN, where the loss is zero).  No host read: the call can be captured in a graph."""
    if h.dim() != 2 or z_type.dim() != 2:
        raise ValueError(f"expected h [N, P] and z_type [N, Dz], got {tuple(h.shape)} and {tuple(z_type.shape)}")
    h = h if h.dtype in (torch.float32, torch.bfloat16) else h.float()
    z = z_type.detach()
    z = z if z.dtype in (torch.float32, torch.bfloat16) else z.float()
    h, z = h.contiguous(), z.contiguous()
    ops.chk_leakage(h, z, "phase_type_leakage_loss")
    return _LeakageFn.apply(h, z)
