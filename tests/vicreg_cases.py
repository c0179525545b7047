"""Plain-torch float64 restatement of the VICReg variance-covariance loss and of its closed-form gradient, for the shapes too large to
commit as fixtures (tests/test_gpu_vicreg.py) and checked against the reference-written fixtures (tests/test_cpu_vicreg.py).

    mu = mean_rows(X), Xc = X - mu, cov = Xc^T Xc / (N-1), std_j = sqrt(cov_jj + eps)
    variance_loss = mean_j relu(target - std_j), covariance_loss = sum_{j != k} cov_jk^2 / D
    d(g_t total + g_v variance + g_c covariance) / dX = Xc A,
    A = (4 cwe / (D (N-1))) offdiag(cov) - diag(vwe 1[std_j < target] / (D (N-1) std_j)),  cwe = g_t cw + g_c,  vwe = g_t vw + g_v
"""
import torch


def vicreg_f64(x, variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4, upstream=(1.0, 0.0, 0.0)):
    """x [N, D] (any dtype, read as float64) -> ((total, variance_loss, covariance_loss) python floats, gradient float64 [N, D] of
    upstream[0] * total + upstream[1] * variance_loss + upstream[2] * covariance_loss)."""
    x = x.detach().to("cpu", torch.float64)
    n, d = x.shape
    if n < 2:
        return (0.0, 0.0, 0.0), torch.zeros_like(x)
    xc = x - x.mean(dim=0, keepdim=True)
    cov = xc.T @ xc / (n - 1)
    std = torch.sqrt(torch.diagonal(cov) + eps)
    vl = torch.relu(variance_target - std).mean()
    off = cov - torch.diag(torch.diagonal(cov))
    cl = (off ** 2).sum() / d
    total = variance_weight * vl + covariance_weight * cl
    g_t, g_v, g_c = (float(u) for u in upstream)
    cwe, vwe = g_t * covariance_weight + g_c, g_t * variance_weight + g_v
    a = (4.0 * cwe / (d * (n - 1))) * off - torch.diag(vwe * (std < variance_target).to(torch.float64) / (d * (n - 1) * std))
    return (float(total), float(vl), float(cl)), xc @ a


def make_rows(n, d, seed, offset=0.0, scale=1.0, mix=0.5):
    """Seeded rows with correlated columns: white noise times (I + mix * random matrix / sqrt(d)), scaled and shifted; float32."""
    g = torch.Generator().manual_seed(seed)
    w = torch.eye(d, dtype=torch.float64) + mix * torch.randn(d, d, generator=g, dtype=torch.float64) / d ** 0.5
    x = torch.randn(n, d, generator=g, dtype=torch.float64) @ w
    return (x * scale + offset).float()


def vicreg_torch(x, variance_weight=1.0, covariance_weight=1.0, variance_target=1.0, eps=1e-4):
    """The same formula with stock differentiable torch ops in the dtype and on the device of x -> total (autograd does the backward)."""
    n, d = x.shape
    xc = x - x.mean(dim=0, keepdim=True)
    std = torch.sqrt(xc.var(dim=0) + eps)
    vl = torch.relu(variance_target - std).mean()
    cov = xc.T @ xc / (n - 1)
    off = cov - torch.diag(torch.diagonal(cov))
    return variance_weight * vl + covariance_weight * (off ** 2).sum() / d
