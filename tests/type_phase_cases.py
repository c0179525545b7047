"""Plain-torch float64 restatements of the type-local spectral baseline (losses.type_local_baseline) and of the phase-type leakage loss
(losses.phase_type_leakage_loss), checked against the fixtures of tests/golden/make_type_phase_golden.py (tests/test_cpu_type_phase.py)
and used where no fixture is committed (tests/test_gpu_type_baseline.py, tests/test_gpu_leakage.py); the seeded input makers; and the
case tables.  The reference has no callable for either piece (both are inline in process_batch): the fixtures pin the FORMULAS.

    baseline:  sim = z_k z_k^T, never itself; the k = min(k_nbrs, N - 1) largest per row ordered by (similarity descending, index
               ascending); S_hat = mean over them of mean_t spec; out = spec - S_hat
    leakage:   C = h_c^T z_c / max(N - 1, 1) over column-centred rows, loss = sqrt(sum C^2),
               d loss / d h = upstream z_c C^T / (max(N - 1, 1) loss), ZERO where loss == 0 (torch's autograd gives NaN there)
"""
import torch

import soft_neighborhood_cases as SC

# name -> (N, K, k_nbrs, T, C, grid denominator of z_k, seed).  The seed is the first of 0..31 at which no row has a tie among its k + 1
# largest similarities (the maker asserts it); z_k on the 1/512 or 1/1024 grid in [-1, 1): every float32 inner product is exact in any
# summation order (product bits + log2 K <= 24), so the float32 ranking is the float64 one.
BASELINE_CASES = {
    "a": (37, 8, 20, 15, 7, 512, 0),          # one workgroup, a partial tile, C no multiple of 4
    "b": (203, 8, 20, 15, 16, 512, 1),        # several workgroups, four tiles with a partial last one
    "c": (12, 8, 20, 15, 16, 512, 0),         # k_nbrs above N - 1: k = 11
    "d": (1031, 8, 64, 4, 8, 1024, 7),        # every lane holds a rank; 17 tiles
    "e": (130, 3, 1, 5, 4, 512, 0),           # k = 1, K no multiple of 4
    "w": (70, 8, 20, 32, 130, 512, 0),        # the wide demean path: lanes stride over C, element by element
}

# name -> (N, P, Dz, seed, offset of the column means in standard deviations, every: rows of dh kept in the fixture)
LEAKAGE_CASES = {
    "a": (37, 12, 64, 701, 0.0, 1),
    "b": (1031, 12, 64, 711, 50.0, 4),        # the pivot path; several slabs
    "c": (70, 5, 7, 721, 1.0, 1),
    "d": (2, 12, 64, 731, 0.0, 1),
}


# ---------------------------------------------------------------------------------------------------------------------------
# type-local baseline
# ---------------------------------------------------------------------------------------------------------------------------
def make_z(n, kw, denom, seed):
    """z_k [N, K] float32 on the 1 / denom grid in [-1, 1), drawn column by column."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-denom, denom, (kw, n), generator=g).float() / float(denom)).T.contiguous()


def make_spec(n, t, c, seed):
    return SC.make_points(n, t, c, 9000 + seed)


def similarities_f64(z_k):
    z = z_k.detach().to("cpu", torch.float64)
    sim = z @ z.T
    sim.fill_diagonal_(float("-inf"))
    return sim


def tied_rows(z_k, k):
    """Number of rows with two equal values among their k + 1 largest similarities (never itself)."""
    head = torch.sort(similarities_f64(z_k), dim=1, descending=True).values[:, :k + 1]
    return int((head[:, 1:] == head[:, :-1]).any(dim=1).sum())


def first_tie_free_seed(n, kw, k_nbrs, denom):
    k = min(k_nbrs, n - 1)
    for seed in range(32):
        if tied_rows(make_z(n, kw, denom, seed), k) == 0:
            return seed
    raise AssertionError(f"no tie-free seed in 0..31 for N {n} K {kw} k {k} on the 1/{denom} grid")


def baseline_inputs(name):
    """-> (z_k [N, K] float32, spec [N, T, C] float32, k_nbrs) of a fixture case."""
    n, kw, k_nbrs, t, c, denom, seed = BASELINE_CASES[name]
    return make_z(n, kw, denom, seed), make_spec(n, t, c, seed), k_nbrs


def type_baseline_f64(z_k, spec, k_nbrs=20):
    """-> (spec_demeaned float64 [N, T, C], s_hat float64 [N, C], topk_idx int64 [N, k])."""
    n = z_k.shape[0]
    k = min(int(k_nbrs), n - 1)
    sim = similarities_f64(z_k)
    idx = torch.argsort(sim, dim=1, descending=True, stable=True)[:, :k]   # stable: equal similarities keep ascending index
    s = spec.detach().to("cpu", torch.float64)
    s_hat = s.mean(dim=1)[idx].mean(dim=1)
    return s - s_hat.unsqueeze(1), s_hat, idx


def type_baseline_rows_f64(z_k, spec, k_nbrs, rows):
    """The same for the anchors `rows` only (no [N, N] array: for N too large for one): -> (s_hat float64 [R, C], topk_idx int64 [R, k])."""
    z = z_k.detach().to("cpu", torch.float64)
    k = min(int(k_nbrs), z.shape[0] - 1)
    rows = torch.as_tensor(rows, dtype=torch.int64)
    sim = z[rows] @ z.T
    sim[torch.arange(rows.numel()), rows] = float("-inf")
    idx = torch.argsort(sim, dim=1, descending=True, stable=True)[:, :k]
    return spec.detach().to("cpu", torch.float64).mean(dim=1)[idx].mean(dim=1), idx


def baseline_bound(spec, k):
    """|float32 kernel - float64| on s_hat and on spec_demeaned: two ordered float32 sums of T and k terms, a division after each, one
    subtraction, doubled for FMA and order freedom."""
    t = spec.shape[1]
    return 2.0 * (t + k + 2) * 2.0 ** -24 * float(spec.abs().max())


def make_monotone(n=130):
    """z_k[j] = (j / 64 - 1, 0, ...): for the anchors with a positive first coordinate every later candidate displaces the list; for
    the negative ones none does after the first tile."""
    z = torch.zeros(n, 4)
    z[:, 0] = torch.arange(n).float() / 64.0 - 1.0
    return z


# ---------------------------------------------------------------------------------------------------------------------------
# leakage
# ---------------------------------------------------------------------------------------------------------------------------
def make_leakage_inputs(n, p, dz, seed, offset=0.0):
    """-> (h [N, P], z [N, Dz]) float32 on the 2^-8 grid: h carries a planted linear image of z plus noise, so the loss is well away
    from zero; every column mean sits `offset` standard deviations from zero."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, dz, generator=g, dtype=torch.float64)
    w = torch.randn(dz, p, generator=g, dtype=torch.float64) / dz ** 0.5
    h = 0.7 * (z @ w) + 0.5 * torch.randn(n, p, generator=g, dtype=torch.float64)
    return SC.grid(h + offset * float(h.std())), SC.grid(z + offset * float(z.std()))


def leakage_inputs(name):
    n, p, dz, seed, offset, _ = LEAKAGE_CASES[name]
    return make_leakage_inputs(n, p, dz, seed, offset)


def leakage_f64(h, z, upstream=1.0):
    """-> (loss python float, d (upstream * loss) / d h float64 [N, P]; zeros where the loss is zero)."""
    h, z = h.detach().to("cpu", torch.float64), z.detach().to("cpu", torch.float64)
    n = h.shape[0]
    den = float(max(n - 1, 1))
    h_c, z_c = h - h.mean(0, keepdim=True), z - z.mean(0, keepdim=True)
    c = h_c.T @ z_c / den
    loss = float(torch.sqrt((c ** 2).sum()))
    if loss == 0.0:
        return 0.0, torch.zeros_like(h)
    return loss, upstream * (z_c @ c.T) / (den * loss)


def kept_rows(n, every):
    rows = list(range(0, n, every))
    if rows[-1] != n - 1:
        rows.append(n - 1)
    return torch.tensor(rows, dtype=torch.int64)
