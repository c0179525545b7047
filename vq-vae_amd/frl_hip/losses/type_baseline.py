"""Type-local spectral baseline of the cross-patch phase block: the `spectral_features` that `phase_neighborhood_loss` reads on every
step with phase anchors (frl/training/representation/step.py:907-931, inline in process_batch).

    z_k = type_projection(z_type)                       rank-K left vectors of the centred type embeddings (stock torch, randomised)
    sim(i, j) = sum_c z_k[i, c] z_k[j, c]               float32
    neighbours of i = the k = min(k_nbrs, N - 1) rows j != i of largest sim, ordered by (similarity descending, index ascending)
    S_mean[j, c] = mean_t spec[j, t, c]
    S_hat[i, c]  = (1 / k) sum over the neighbours of S_mean[j, c], summed in rank order
    out[i, t, c] = spec[i, t, c] - S_hat[i, c]

The reference forms `sim` as a full [N, N] float32 array (133 MB at 16 x 360 anchors, 950 MB at 16 x 964) for one `topk`.  Here
`frl_type_baseline` (csrc/type_baseline.hip) streams the candidate rows past one wave per anchor, which keeps its k best in a sorted
list one rank per lane: nothing N x N and nothing N x k x C is written.  `torch.topk` leaves equal similarities unordered; the order here
is fixed, as in `build_phase_pairs`.  A NaN similarity ranks as -inf.  Results are bit-identical from run to run.
"""
from __future__ import annotations

import torch

from .. import ops


def type_projection(z_type: torch.Tensor, rank: int = 8) -> torch.Tensor:
    """z_type [N, D] -> [N, rank]: the top `rank` left singular vectors of the column-centred embeddings, by torch.pca_lowrank
    (step.py:913-915).  Stock torch ops on purpose: the algorithm is randomised (it draws from torch's generator) and small; the columns
    are orthonormal.  Gradients follow torch's own rules; the reference's caller and `type_local_baseline` use the result as data."""
    if z_type.dim() != 2:
        raise ValueError(f"type_projection: expected z_type [N, D], got {tuple(z_type.shape)}")
    if not 1 <= int(rank) <= min(z_type.shape):
        raise ValueError(f"type_projection: rank must be in 1..min(N, D) = {min(z_type.shape)}, got {rank}")
    z_c = z_type - z_type.mean(0, keepdim=True)
    u, _, _ = torch.pca_lowrank(z_c, q=int(rank), center=False)
    return u


def type_local_baseline(z_k: torch.Tensor, spec: torch.Tensor, k_nbrs: int = 20, return_parts: bool = False):
    """z_k [N, K] float32 (1 <= K <= 64), spec [N, T, C] float32 (C <= 256), both contiguous and on the GPU, N >= 2,
    1 <= k_nbrs <= 64 -> spec_demeaned [N, T, C] float32; with return_parts=True (spec_demeaned, s_hat [N, C] float32,
    topk_idx [N, k] int64), k = min(k_nbrs, N - 1).

    Not differentiable: both inputs are data or stop-gradient in the reference, and the outputs carry no graph whatever the inputs
    require.  No host read and no synchronisation: every output size follows from the shapes, so the call can be captured in a graph.
    Limits raise ValueError before a device is needed; CPU tensors raise FrlHipError."""
    ops.chk_type_baseline(z_k, spec, k_nbrs)
    with torch.no_grad():
        out, s_hat, idx = ops.type_baseline(z_k.detach(), spec.detach(), int(k_nbrs))
    return (out, s_hat, idx) if return_parts else out
