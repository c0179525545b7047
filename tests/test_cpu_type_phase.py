"""The float64 restatements of the type-local baseline and of the phase-type leakage loss (tests/type_phase_cases.py) against the
fixtures of tests/golden/make_type_phase_golden.py (stock torch in float64 on the formulas of step.py:922-928 and :1015-1021): indices
equal, floats to 1e-12; the closed-form leakage gradient against autograd; the (similarity, index) order on tied similarities; the
type_projection helper; and the argument errors of the package's Python layer that need no GPU."""
import os

import numpy as np
import pytest
import torch

import type_phase_cases as TP

B_CASES, L_CASES = list(TP.BASELINE_CASES), list(TP.LEAKAGE_CASES)


def _fx(golden_dir, kind, name):
    return np.load(os.path.join(golden_dir, f"{kind}_{name}.npz"))


@pytest.mark.parametrize("name", B_CASES)
def test_baseline_restatement_reproduces_the_fixture(golden_dir, name):
    fx = _fx(golden_dir, "type_baseline", name)
    z_k, spec, k_nbrs = TP.baseline_inputs(name)
    n, kw, k, t, c = (int(v) for v in fx["shape"])
    assert z_k.shape == (n, kw) and spec.shape == (n, t, c) and k == min(k_nbrs, n - 1) and int(fx["seed"]) == TP.BASELINE_CASES[name][6]
    out, s_hat, idx = TP.type_baseline_f64(z_k, spec, k_nbrs)
    assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), fx["idx"].astype(np.int64))
    assert np.abs(s_hat.numpy() - fx["s_hat64"]).max() <= 1e-12
    assert np.abs(out.numpy() - (spec.double().numpy() - fx["s_hat64"][:, None, :])).max() <= 1e-12
    assert not bool((idx == torch.arange(n).unsqueeze(1)).any())


@pytest.mark.parametrize("name", B_CASES)
def test_baseline_inputs_rank_alike_in_float32_and_float64(name):
    """What lets the GPU test ask for equal indices: exact float32 similarities and no tie among any row's k + 1 largest."""
    z_k, _, k_nbrs = TP.baseline_inputs(name)
    n, kw, _, _, _, denom, seed = TP.BASELINE_CASES[name]
    assert int(np.ceil(np.log2(denom * denom))) + int(np.ceil(np.log2(kw))) <= 24
    assert torch.equal((z_k @ z_k.T).double(), z_k.double() @ z_k.double().T)
    assert TP.tied_rows(z_k, min(k_nbrs, n - 1)) == 0


def test_baseline_fixtures_hold_what_they_are_there_for(golden_dir):
    shapes = {name: tuple(int(v) for v in _fx(golden_dir, "type_baseline", name)["shape"]) for name in B_CASES}
    assert shapes["a"][0] < 64 and shapes["a"][4] % 4 != 0
    assert 3 * 64 < shapes["b"][0] < 4 * 64 and shapes["b"][0] % 4 != 0
    assert shapes["c"][2] == shapes["c"][0] - 1 == 11
    assert shapes["d"][2] == 64 and (shapes["d"][0] + 63) // 64 == 17
    assert shapes["e"][2] == 1 and shapes["e"][1] == 3
    assert shapes["w"][4] > 128 and shapes["w"][4] % 4 != 0


def test_tied_similarities_follow_similarity_then_index():
    z = TP.baseline_inputs("a")[0]
    z = torch.cat([z, z[:20], torch.zeros(3, 8)])                       # duplicated rows and zero rows: many exact ties
    n, k = z.shape[0], 20
    assert TP.tied_rows(z, k) > n // 3
    _, _, idx = TP.type_baseline_f64(z, torch.zeros(n, 1, 1), k)
    sim = TP.similarities_f64(z)
    for i in range(n):                                                  # a plain loop: sort the (-similarity, index) tuples
        want = sorted((-float(sim[i, j]), j) for j in range(n) if j != i)[:k]
        assert [j for _, j in want] == idx[i].tolist()


@pytest.mark.parametrize("name", L_CASES)
def test_leakage_restatement_reproduces_the_fixture(golden_dir, name):
    fx = _fx(golden_dir, "leakage", name)
    h, z = TP.leakage_inputs(name)
    assert tuple(int(v) for v in fx["shape"]) == (h.shape[0], h.shape[1], z.shape[1])
    loss, dh = TP.leakage_f64(h, z)
    assert float(fx["loss64"]) >= 0.1 and abs(loss - float(fx["loss64"])) <= 1e-12
    assert np.array_equal(fx["rows"], TP.kept_rows(h.shape[0], TP.LEAKAGE_CASES[name][5]).numpy())
    assert np.abs(dh[torch.from_numpy(fx["rows"])].numpy() - fx["dh64"]).max() <= 1e-12
    assert abs(float(dh.abs().max()) - float(fx["dh_max"])) <= 1e-12


@pytest.mark.parametrize("name", L_CASES)
@pytest.mark.parametrize("upstream", [1.0, -2.5])
def test_leakage_closed_form_gradient_matches_autograd(name, upstream):
    h, z = TP.leakage_inputs(name)
    h64 = h.double().requires_grad_(True)
    z64 = z.double()
    n = h.shape[0]
    cov = (h64 - h64.mean(0, keepdim=True)).T @ (z64 - z64.mean(0, keepdim=True)) / max(n - 1, 1)
    loss = cov.pow(2).sum().sqrt()
    (upstream * loss).backward()
    want_loss, dh = TP.leakage_f64(h, z, upstream=upstream)
    assert abs(float(loss.detach()) - want_loss) <= 1e-12
    assert float((dh - h64.grad).abs().max()) <= 1e-12


def test_leakage_case_b_sits_far_from_zero():
    h, z = TP.leakage_inputs("b")
    assert float((h.double().mean(0).abs() / h.double().std(0)).min()) > 25 and float((z.double().mean(0).abs() / z.double().std(0)).min()) > 25


def test_leakage_zero_loss_has_zero_gradient():
    """Where torch's autograd returns NaN (the derivative of sqrt at 0) the restatement, like the package, returns zeros."""
    h, z = TP.leakage_inputs("a")
    for hh, zz in ((h[:1], z[:1]), (torch.full_like(h, 37.125), z), (h, torch.full_like(z, -3.0))):
        loss, dh = TP.leakage_f64(hh, zz)
        assert loss == 0.0 and dh.shape == hh.shape and not bool(dh.any())


def test_type_projection_shape_and_orthonormality():
    from frl_hip.losses import type_projection
    g = torch.Generator().manual_seed(741)                              # eight strong directions over unit noise, means well off zero
    z = 4.0 * torch.randn(300, 8, generator=g) @ torch.randn(8, 64, generator=g) / 8 ** 0.5 + torch.randn(300, 64, generator=g) + 5.0
    torch.manual_seed(0)
    u = type_projection(z, rank=8)
    assert u.shape == (300, 8) and u.dtype == torch.float32
    assert float((u.T @ u - torch.eye(8)).abs().max()) <= 1e-5
    assert float(u.sum(0).abs().max()) <= 1e-4                          # the columns of a centred matrix's left vectors sum to zero
    # it spans the top of the centred spectrum: the projection keeps what the exact rank-8 truncation keeps, to the randomised method's accuracy
    z_c = (z - z.mean(0, keepdim=True)).double()
    s = torch.linalg.svdvals(z_c)
    kept = float(((u.double().T @ z_c) ** 2).sum())
    assert kept <= float((s[:8] ** 2).sum()) * (1 + 1e-9) and kept >= 0.9 * float((s[:8] ** 2).sum())
    with pytest.raises(ValueError, match="rank must be in"):
        type_projection(z, rank=65)
    with pytest.raises(ValueError, match=r"expected z_type \[N, D\]"):
        type_projection(z[0])


def test_python_layer_argument_errors():
    from frl_hip import _lib
    from frl_hip.losses import phase_type_leakage_loss, type_local_baseline
    z_k, spec, _ = TP.baseline_inputs("a")
    with pytest.raises(ValueError, match="K must be in 1..64"):
        type_local_baseline(torch.zeros(37, 65), spec)
    with pytest.raises(ValueError, match="k_nbrs must be in 1..64"):
        type_local_baseline(z_k, spec, k_nbrs=65)
    with pytest.raises(ValueError, match="k_nbrs must be in 1..64"):
        type_local_baseline(z_k, spec, k_nbrs=0)
    with pytest.raises(ValueError, match="1 <= C <= 256"):
        type_local_baseline(z_k, torch.zeros(37, 2, 257))
    with pytest.raises(ValueError, match="T must be positive"):
        type_local_baseline(z_k, torch.zeros(37, 0, 7))
    with pytest.raises(ValueError, match="N >= 2"):
        type_local_baseline(z_k[:1], spec[:1])
    with pytest.raises(ValueError, match="z_k has 36 rows and spec 37"):
        type_local_baseline(z_k[:36], spec)
    with pytest.raises(ValueError, match=r"expected z_k \[N, K\] and spec \[N, T, C\]"):
        type_local_baseline(z_k, spec[:, 0])
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(z_k.double(), spec)
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(z_k, spec.to(torch.bfloat16))
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(z_k, spec.transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(torch.zeros(8, 37).T, spec)
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):    # a CPU tensor raises: there is no CPU path
        type_local_baseline(z_k, spec)
    h, z = TP.leakage_inputs("a")
    with pytest.raises(ValueError, match="P <= 64"):
        phase_type_leakage_loss(torch.zeros(37, 65), z)
    with pytest.raises(ValueError, match="Dz <= 128"):
        phase_type_leakage_loss(h, torch.zeros(37, 129))
    with pytest.raises(ValueError, match=r"expected h \[N, P\] and z \[N, Dz\]"):
        phase_type_leakage_loss(h[:36], z)
    with pytest.raises(ValueError, match=r"expected h \[N, P\] and z_type \[N, Dz\]"):
        phase_type_leakage_loss(h, z[0])
    with pytest.raises(ValueError, match="N >= 1"):
        phase_type_leakage_loss(h[:0], z[:0])
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):
        phase_type_leakage_loss(h, z)


def test_abi_refuses_out_of_range_arguments_before_any_launch():
    """Plain range tests of the host side: every refusal comes back as a negative code with a message, no device needed."""
    import ctypes
    from frl_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def baseline(n=8, kw=8, t=2, c=4, k=3, ws=p, ws_bytes=1 << 20, z=p):
        return lib.frl_type_baseline(z, p, n, kw, t, c, k, p, p, p, ws, ws_bytes, None)

    for kw_args, msg in ((dict(n=1, k=1), "N >= 2"), (dict(kw=0), "K must be"), (dict(kw=65), "K must be"), (dict(k=0), "k must be"),
                         (dict(k=65, n=100), "k must be"), (dict(k=8), "k must be"), (dict(c=257), "C <= 256"), (dict(c=0), "C <= 256"),
                         (dict(t=0), "T must be positive"), (dict(z=None), "null pointer"), (dict(ws=None), "workspace too small"),
                         (dict(ws_bytes=8 * 4 * 4 - 1), "workspace too small")):
        assert baseline(**kw_args) < 0, kw_args
        assert msg in lib.frl_last_error().decode(), (kw_args, lib.frl_last_error())
    assert lib.frl_type_baseline_workspace_bytes(8, 4) == 8 * 4 * 4 and lib.frl_type_baseline_workspace_bytes(0, 4) == 0

    def fwd(n=8, pp=4, dz=8, hd=0, zd=0, ws_bytes=1 << 20, cmat=p, centre=p):
        return lib.frl_leakage_fwd(p, hd, p, zd, n, pp, dz, p, cmat, centre, p, ws_bytes, None)

    for kw_args, msg in ((dict(n=0), "rows"), (dict(pp=65), "P <= 64"), (dict(pp=0), "P <= 64"), (dict(dz=129), "Dz <= 128"), (dict(hd=2), "dtypes"),
                         (dict(zd=7), "dtypes"), (dict(cmat=None), "go together"), (dict(ws_bytes=16), "workspace too small")):
        assert fwd(**kw_args) < 0, kw_args
        assert msg in lib.frl_last_error().decode(), (kw_args, lib.frl_last_error())
    assert lib.frl_leakage_bwd(p, 0, p, p, p, None, 8, 4, 8, p, 0, None) < 0 and "NULL" in lib.frl_last_error().decode()
    assert lib.frl_leakage_bwd(p, 0, p, p, p, p, 8, 65, 8, p, 0, None) < 0
    assert lib.frl_leakage_workspace_bytes(100, 12, 64) == (2 + 1) * (12 * 64 + 12 + 64) * 4
    assert lib.frl_leakage_workspace_bytes(10 ** 6, 12, 64) == (256 + 1) * (12 * 64 + 12 + 64) * 4
