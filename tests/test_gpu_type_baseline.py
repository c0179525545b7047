"""GPU parity of the type-local spectral baseline (csrc/type_baseline.hip behind losses.type_local_baseline) against the fixtures of
tests/golden/make_type_phase_golden.py and, where no fixture is committed, against the float64 restatement (tests/type_phase_cases.py,
pinned to the fixtures by tests/test_cpu_type_phase.py).

Bounds.  topk_idx is equal, order included: the inputs sit on a dyadic grid on which every float32 inner product is exact in any
summation order, so the float32 ranking is the float64 one, and ties follow (similarity descending, index ascending) on both sides.
s_hat and spec_demeaned are within 2 (T + k + 2) 2^-24 max|spec| absolutely: two ordered float32 sums of T and k terms, a division
after each, one subtraction, doubled for FMA and order freedom."""
import os

import numpy as np
import pytest
import torch

import soft_neighborhood_cases as SC
import type_phase_cases as TP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = list(TP.BASELINE_CASES)


def _run(z_k, spec, k_nbrs):
    from frl_hip.losses import type_local_baseline
    out, s_hat, idx = type_local_baseline(z_k.to(DEV), spec.to(DEV), k_nbrs, return_parts=True)
    n, k = z_k.shape[0], min(k_nbrs, z_k.shape[0] - 1)
    assert out.dtype == torch.float32 and out.shape == spec.shape and s_hat.dtype == torch.float32 and s_hat.shape == (n, spec.shape[2])
    assert idx.dtype == torch.int64 and idx.shape == (n, k) and out.is_cuda and s_hat.is_cuda and idx.is_cuda
    assert not out.requires_grad and not s_hat.requires_grad
    assert not bool((idx == torch.arange(n, device=DEV).unsqueeze(1)).any()), "an anchor is among its own neighbours"
    return out, s_hat, idx


def _check_floats(out, s_hat, spec, s_hat64, k, what):
    bound = TP.baseline_bound(spec, k)
    s_hat64 = torch.as_tensor(s_hat64, dtype=torch.float64)
    dev_s = float((s_hat.double().cpu() - s_hat64).abs().max())
    dev_o = float((out.double().cpu() - (spec.double() - s_hat64.unsqueeze(1))).abs().max())
    print(f"{what}: s_hat dev / bound {dev_s / bound:.3f}, spec_demeaned dev / bound {dev_o / bound:.3f} (bound {bound:.3e})")
    assert dev_s <= bound and dev_o <= bound, what


def _check_against_restatement(z_k, spec, k_nbrs, what):
    out, s_hat, idx = _run(z_k, spec, k_nbrs)
    _, s_hat64, idx64 = TP.type_baseline_f64(z_k, spec, k_nbrs)
    assert torch.equal((z_k @ z_k.T).double(), z_k.double() @ z_k.double().T), "the case's float32 similarities are not exact"
    assert torch.equal(idx.cpu(), idx64), what
    _check_floats(out, s_hat, spec, s_hat64, idx64.shape[1], what)
    return out, s_hat, idx


@pytest.mark.parametrize("name", CASES)
def test_fixture(golden_dir, name):
    from frl_hip.losses import type_local_baseline
    fx = np.load(os.path.join(golden_dir, f"type_baseline_{name}.npz"))
    z_k, spec, k_nbrs = TP.baseline_inputs(name)
    out, s_hat, idx = _run(z_k, spec, k_nbrs)
    assert np.array_equal(idx.cpu().numpy(), fx["idx"].astype(np.int64)), "topk_idx differs from the fixture"
    _check_floats(out, s_hat, spec, fx["s_hat64"], idx.shape[1], name)
    only = type_local_baseline(z_k.to(DEV), spec.to(DEV), k_nbrs)       # return_parts=False: the same bits
    assert torch.is_tensor(only) and torch.equal(only, out)
    out2, s_hat2, idx2 = _run(z_k, spec, k_nbrs)                         # identical bits from run to run
    assert torch.equal(out, out2) and torch.equal(s_hat, s_hat2) and torch.equal(idx, idx2)


def test_monotone_similarities():
    """One-dimensional z_k rising with the index: for an anchor with a positive coordinate every later candidate displaces the list
    (the neighbours are the last rows, descending); for a negative one none does after the first tile (the first rows, ascending)."""
    z_k = TP.make_monotone(130)
    _, _, idx = _check_against_restatement(z_k, TP.make_spec(130, 3, 4, 31), 20, "monotone")
    idx = idx.cpu()
    assert idx[129].tolist() == list(range(128, 108, -1)) and idx[100].tolist() == list(range(129, 109, -1))
    assert idx[0].tolist() == list(range(1, 21)) and idx[5].tolist() == [0, 1, 2, 3, 4] + list(range(6, 21))
    assert idx[64].tolist() == list(range(20))                          # the zero row: every similarity ties at 0


def test_tied_similarities_follow_similarity_then_index():
    z = TP.baseline_inputs("a")[0]
    z_k = torch.cat([z, z[:20], torch.zeros(3, 8)])                     # duplicated rows and zero rows
    z_k[7] = 0.0                                                        # and a zero row among the first
    n = z_k.shape[0]
    assert TP.tied_rows(z_k, 20) > n // 3
    _check_against_restatement(z_k, TP.make_spec(n, 5, 7, 32), 20, "duplicated and zero rows")


def test_self_similarity_is_the_largest():
    """Rows whose similarity with themselves exceeds every other: -inf on the diagonal in the reference, `never itself` here."""
    z_k, spec, _ = TP.baseline_inputs("b")
    z_k = z_k.clone()
    z_k[::7] *= 0.5                                                     # mixed norms (still on the grid): some rows' largest similarity is another's
    sim = z_k.double() @ z_k.double().T
    assert int((sim.argmax(dim=1) == torch.arange(z_k.shape[0])).sum()) > z_k.shape[0] // 2
    _check_against_restatement(z_k, spec, 20, "self-similarity largest")


@pytest.mark.parametrize("n,kw,k_nbrs,t,c", [(2, 8, 20, 3, 4), (9, 64, 64, 2, 256), (65, 1, 64, 1, 1), (257, 5, 33, 7, 12)])
def test_limits_and_odd_shapes(n, kw, k_nbrs, t, c):
    """N = 2 (k = 1), the widest projection and spectra, a single column and year, widths that are no multiple of 4."""
    z_k, spec = TP.make_z(n, kw, 512, 40 + n), TP.make_spec(n, t, c, 50 + n)
    _check_against_restatement(z_k, spec, k_nbrs, f"N {n} K {kw} k {k_nbrs} T {t} C {c}")


def test_more_anchors_than_a_score_row_in_lds_would_hold():
    """10007 anchors (the kNN kernels that keep their scores in LDS stop near 9900), checked on a sample of anchors: the first and last
    of the batch, of a workgroup and of a tile."""
    n, k = 10007, 20
    z_k, spec = TP.make_z(n, 4, 512, 61), TP.make_spec(n, 2, 4, 62)
    out, s_hat, idx = _run(z_k, spec, k)
    rows = sorted({0, 1, 3, 4, 63, 64, 4095, 4096, 9983, 9984, 10003, 10004, 10005, 10006} | set(range(17, n, 397)))
    s_hat64, idx64 = TP.type_baseline_rows_f64(z_k, spec, k, rows)
    assert torch.equal(idx.cpu()[rows], idx64)
    bound = TP.baseline_bound(spec, k)
    dev = float((s_hat.double().cpu()[rows] - s_hat64).abs().max())
    dev_o = float((out.double().cpu()[rows] - (spec.double()[rows] - s_hat64.unsqueeze(1))).abs().max())
    print(f"N {n}: s_hat dev / bound {dev / bound:.3f}, spec_demeaned dev / bound {dev_o / bound:.3f}")
    assert dev <= bound and dev_o <= bound
    assert int(idx.min()) >= 0 and int(idx.max()) < n


def test_rows_at_an_odd_storage_offset():
    """Contiguous views that start one element into their buffers: no 16-byte alignment, the same values: identical bits."""
    z_k, spec, k_nbrs = TP.baseline_inputs("b")
    zb, sb = torch.zeros(z_k.numel() + 1, device=DEV), torch.zeros(spec.numel() + 1, device=DEV)
    zv, sv = zb[1:].view(z_k.shape), sb[1:].view(spec.shape)
    zv.copy_(z_k)
    sv.copy_(spec)
    assert zv.is_contiguous() and zv.data_ptr() % 16 != 0 and sv.data_ptr() % 16 != 0
    from frl_hip.losses import type_local_baseline
    got = type_local_baseline(zv, sv, k_nbrs, return_parts=True)
    want = _run(z_k, spec, k_nbrs)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_output_feeds_phase_neighborhood_loss():
    """The hand-over of dtype, device and layout: the demeaned spectra against the restated baseline's, through the loss, within the
    bound of tests/test_gpu_soft_neighborhood.py for a loss (2e-6 max(1, |loss|))."""
    from frl_hip.losses import phase_neighborhood_loss, type_local_baseline
    z_k, spec, k_nbrs = TP.baseline_inputs("b")
    n, t = spec.shape[:2]
    ysfc = SC.make_ysfc(n, t, 71).to(DEV)
    g = torch.Generator().manual_seed(72)
    pairs = torch.randint(0, n, (300, 2), generator=g).to(DEV)
    weights = SC.make_weights(300, 73).to(DEV)
    phase = SC.make_points(n, t, 12, 74, 0.25).to(DEV)
    got_spec = type_local_baseline(z_k.to(DEV), spec.to(DEV), k_nbrs)
    want_spec = TP.type_baseline_f64(z_k, spec, k_nbrs)[0].float().to(DEV)
    kw = dict(pair_weights=weights, tau_ref=1.0, tau_learned=1.0)
    got, st_got = phase_neighborhood_loss(got_spec, phase, ysfc, pairs, **kw)
    want, st_want = phase_neighborhood_loss(want_spec, phase, ysfc, pairs, **kw)
    raw, _ = phase_neighborhood_loss(spec.to(DEV), phase, ysfc, pairs, **kw)
    bound = 2e-6 * max(1.0, abs(float(want)))
    print(f"loss {float(got)!r} against {float(want)!r}: dev {abs(float(got) - float(want)):.3e} bound {bound:.3e}; without the baseline {float(raw)!r}")
    assert float(want) > 0 and st_got["n_pairs_sufficient_overlap"] == st_want["n_pairs_sufficient_overlap"] > 0
    assert abs(float(got) - float(want)) <= bound
    # the baseline does move this loss, by well over the bound (it shifts whole pixels, so only the cross-pixel term feels it): handing
    # the raw spectra through, or another pixel's baseline, would not pass
    assert abs(float(raw) - float(want)) > 10 * bound


def test_inputs_that_require_grad_give_outputs_without_a_graph():
    z_k, spec, k_nbrs = TP.baseline_inputs("a")
    from frl_hip.losses import type_local_baseline
    out = type_local_baseline(z_k.to(DEV).requires_grad_(True), spec.to(DEV).requires_grad_(True), k_nbrs)
    assert not out.requires_grad and out.grad_fn is None


def test_graph_capture_replays_on_new_inputs():
    """No host read and no synchronisation: the call is captured once and replayed on other values."""
    from frl_hip.losses import type_local_baseline
    za, sa, k_nbrs = TP.baseline_inputs("b")
    zb, sb = TP.make_z(203, 8, 512, 5), TP.make_spec(203, 15, 16, 6)
    z_in, s_in = za.to(DEV).clone(), sa.to(DEV).clone()
    type_local_baseline(z_in, s_in, k_nbrs)                             # warm-up: the library is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, s_hat, idx = type_local_baseline(z_in, s_in, k_nbrs, return_parts=True)
    for z_k, spec in ((zb, sb), (za, sa)):
        z_in.copy_(z_k)
        s_in.copy_(spec)
        graph.replay()
        torch.cuda.synchronize()
        want = _run(z_k, spec, k_nbrs)
        assert torch.equal(out, want[0]) and torch.equal(s_hat, want[1]) and torch.equal(idx, want[2])


def test_device_side_argument_errors():
    from frl_hip.losses import type_local_baseline
    z_k, spec, _ = TP.baseline_inputs("a")
    z_k, spec = z_k.to(DEV), spec.to(DEV)
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(z_k, spec.transpose(1, 2))
    with pytest.raises(ValueError, match="contiguous float32"):
        type_local_baseline(z_k.to(torch.bfloat16), spec)
    with pytest.raises(ValueError, match="k_nbrs must be in 1..64"):
        type_local_baseline(z_k, spec, 65)
    with pytest.raises(ValueError, match="N >= 2"):
        type_local_baseline(z_k[:1], spec[:1])
    from frl_hip import _lib
    with pytest.raises(_lib.FrlHipError, match="no CPU fallback"):
        type_local_baseline(z_k, spec.cpu())
