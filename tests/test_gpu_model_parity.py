"""Model-level parity on the GPU: frl_hip RepresentationModel / VQVAE vs the golden vectors generated from the reference
(encoder: pinned) and vs the oracle's VQ-VAE step (quantizer / decoder: parity unpinned by the reference)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frl_oracle as O  # noqa: E402

DEV = "cuda:0"
TINY_KW = dict(type_in_channels=8, phase_in_channels=8, z_type_dim=8, z_phase_dim=4, type_encoder_channels=(16, 8),
               type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
               phase_tcn_dropout=0.0, phase_tcn_num_groups=4)


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def _state(fx):
    return {k[6:]: torch.from_numpy(fx[k]).float() for k in fx.files if k.startswith("state.")}


def maxabs(a, b):
    return float(np.abs(a.detach().float().cpu().numpy().astype(np.float64) - np.asarray(b, dtype=np.float64)).max())


@pytest.mark.parametrize("seed", [0, 1])
def test_tiny_forward_backward_matches_reference_golden(golden_dir, seed):
    from frl_hip.models import RepresentationModel
    fx = _load(golden_dir, f"tiny_seed{seed}")
    m = RepresentationModel(**TINY_KW).to(DEV)
    missing = m.load_state_dict(_state(fx), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    m.eval()
    tile = torch.from_numpy(fx["tile"]).float().to(DEV)
    x_type = tile.mean(1).permute(0, 3, 1, 2).contiguous().requires_grad_(True)      # [B,C,H,W]
    x_phase = tile.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)           # [B,C,T,H,W]
    z, gate = m(x_type, return_gate=True)
    assert z.shape == (2, 8, 8, 8) and maxabs(z, fx["z_type"]) < 1e-5 and maxabs(gate, fx["gate"]) < 1e-5
    h = m.encoder(x_type.detach().permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    assert maxabs(h, fx["h"]) < 1e-5
    zp = m.forward_phase(x_phase, z.detach())
    assert zp.shape == (2, 4, 5, 8, 8) and maxabs(zp, fx["z_phase"]) < 1e-5
    loss = z.float().pow(2).mean() + zp.float().pow(2).mean()
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    loss.backward()
    assert maxabs(x_type.grad, fx["grad.x_type"]) < 1e-6 + 1e-4 * np.abs(fx["grad.x_type"]).max()
    assert maxabs(x_phase.grad, fx["grad.x_phase"]) < 1e-6 + 1e-4 * np.abs(fx["grad.x_phase"]).max()
    for name, p in m.named_parameters():
        ref = fx["grad." + name]
        assert maxabs(p.grad, ref) <= 1e-6 + 2e-4 * np.abs(ref).max(), name
    # sparse path == dense path at the same pixels (representation.py:385-388)
    yx = fx["loc_yx"]
    xpx = x_phase.detach()[0][:, :, yx[:, 0], yx[:, 1]].permute(2, 0, 1).contiguous()
    zpx = z.detach()[0][:, yx[:, 0], yx[:, 1]].permute(1, 0).contiguous()
    zl, gam, bet, hpre = m.forward_phase_at_locations(xpx, zpx, return_film=True, return_pre_film=True)
    assert zl.shape == (7, 5, 4) and maxabs(zl, fx["loc_z"]) < 1e-5
    assert maxabs(gam, fx["loc_gamma"]) < 1e-5 and maxabs(bet, fx["loc_beta"]) < 1e-5 and maxabs(hpre, fx["loc_hpre"]) < 1e-5


def test_full_size_tile_within_1e5_of_reference(golden_dir):
    """BASELINE north_star tolerance: latents within 1e-5 (float32 parity mode) of the reference CPU path."""
    from frl_hip.models import RepresentationModel
    fx = _load(golden_dir, "full_seed0")
    m = RepresentationModel(64, 64, type_encoder_dropout=0.0, phase_tcn_dropout=0.0).to(DEV).eval()
    sd = _state(fx)
    # the reference default has Dropout2d modules (indices 0,1,2,3 | 4,5); dropout-free build has (0,1,2 | 3,4)
    remap = {"encoder.layers.4.weight": "encoder.layers.3.weight", "encoder.layers.5.weight": "encoder.layers.4.weight",
             "encoder.layers.5.bias": "encoder.layers.4.bias"}
    sd = {remap.get(k, k): v for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    tile = torch.from_numpy(fx["tile"]).float().to(DEV)
    x_type = tile.mean(1)
    z, gate = m.forward_nhwc(x_type, return_gate=True)
    assert maxabs(z.permute(0, 3, 1, 2), fx["z_type"]) < 1e-5
    assert maxabs(gate.permute(0, 3, 1, 2), fx["gate"]) < 1e-5
    zp = m.forward_phase_nhwc(tile, z)
    assert maxabs(zp.permute(0, 4, 1, 2, 3), fx["z_phase"]) < 1e-5


def test_reference_default_state_dict_keys_load_with_dropout_modules(golden_dir):
    from frl_hip.models import RepresentationModel
    fx = _load(golden_dir, "full_seed0")
    m = RepresentationModel(64, 64)       # class defaults: dropout 0.1 -> Sequential indices 0,1,2,3,4,5
    res = m.load_state_dict(_state(fx), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sum(p.numel() for p in m.parameters()) == 238788


def test_min_gate_and_projection(golden_dir):
    from frl_hip.models import RepresentationModel
    fx = _load(golden_dir, "tiny_mingate_proj")
    kw = dict(TINY_KW, phase_in_channels=16)
    m = RepresentationModel(**kw).to(DEV).eval()
    m.load_state_dict(_state(fx), strict=True)
    m.set_spatial_min_gate(float(fx["min_gate"]))
    tile = torch.from_numpy(fx["tile"]).float().to(DEV)
    z, gate = m.forward_nhwc(tile.mean(1), return_gate=True)
    assert maxabs(z.permute(0, 3, 1, 2), fx["z_type"]) < 1e-5 and maxabs(gate.permute(0, 3, 1, 2), fx["gate"]) < 1e-5
    assert gate.min().item() >= float(fx["min_gate"]) - 1e-6
    xp = torch.from_numpy(fx["xp16"]).float().to(DEV)                    # [N,16,T]
    out = m.phase_tcn(xp.permute(2, 0, 1).unsqueeze(0).contiguous())[0].permute(1, 2, 0)
    assert maxabs(out, fx["tcn_out"]) < 1e-5
    m.set_spatial_min_gate(1.0)                                           # gate floor 1 => output == encoder output
    z1 = m.forward_nhwc(tile.mean(1))
    h = m.encoder(tile.mean(1).contiguous())
    assert maxabs(z1, h.detach().cpu().numpy()) < 1e-5


def _vqvae_from_fixture(fx, dtype=torch.float32):
    from frl_hip.models import VQVAE
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, beta=0.25, hidden=16, z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4, compute_dtype=dtype).to(DEV)
    res = m.load_state_dict(_state(fx), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return m


def test_vqvae_step_matches_oracle_fixture(golden_dir):
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    m = _vqvae_from_fixture(fx)
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    m.train()
    out = m.forward_tiles(tiles[0])
    assert np.array_equal(out["idx"].cpu().numpy().astype(np.int64), fx["idx"])          # bit-exact indices
    assert abs(out["loss"].item() - float(fx["loss"])) < 1e-5
    assert abs(out["l_type"].item() - float(fx["l_type"])) < 1e-5 and abs(out["l_phase"].item() - float(fx["l_phase"])) < 1e-5
    assert abs(out["vq_loss"].item() - float(fx["vq_loss"])) < 1e-5
    assert abs(out["perplexity"].item() - float(fx["perplexity"])) < 1e-4
    assert maxabs(out["xhat_type"].permute(0, 3, 1, 2), fx["xhat_type"]) < 1e-5
    out["loss"].backward()
    for name, p in m.named_parameters():
        ref = fx["grad." + name]
        assert maxabs(p.grad, ref) <= 1e-6 + 2e-4 * np.abs(ref).max(), name
    # legacy model(batch) contract
    cont_pred, cat_logits, canopy_pred, vq_loss, perp = m({"tile": tiles[0]})
    assert cat_logits == {} and cont_pred.shape == (2, 8, 8, 8) and canopy_pred.shape == (2, 5, 8, 8, 8)
    assert "quant.codebook" in dict(m.named_parameters()) and m.quant.codebook_size == 16 and m.quant.emb_dim == 8


def test_three_step_loss_trajectory_matches_oracle(golden_dir):
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    m = _vqvae_from_fixture(fx)
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    traj = [tr.step(tiles[i])["loss"].item() for i in range(3)]
    assert np.abs(np.asarray(traj) - fx["traj"]).max() < 2e-5, (traj, fx["traj"])


def test_sixty_step_trajectory_matches_the_oracle_trainer(golden_dir):
    """Longer than the committed 3-step fixture: the HIP trainer and the float64 oracle trainer run side by side for 60 optimiser
    steps over a recycled pool of tiles.  Index flips would show as a jump in loss or perplexity; none is allowed."""
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    tr = VQVAETrainer(_vqvae_from_fixture(fx), lr=1e-3, total_steps=60)
    sd = {k[6:]: torch.from_numpy(fx[k]).double() for k in fx.files if k.startswith("state.")}
    hp = dict(type_encoder_num_groups=4, phase_tcn_num_groups=4, phase_tcn_dilations=(1, 2, 4), beta=0.25)
    otr = O.OracleTrainer(sd, hp, lr=1e-3, total_steps=60)
    pool = torch.randn(4, 2, 5, 8, 8, 8, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    for i in range(60):
        a = tr.step(pool[i % 4].float().to(DEV))
        b = otr.step(pool[i % 4])
        assert abs(a["loss"].item() - float(b["loss"])) < 5e-6, (i, a["loss"].item(), float(b["loss"]))
        assert abs(float(a["perplexity"]) - float(b["perplexity"])) < 1e-4, i


def test_bf16_training_tracks_the_float64_oracle_at_full_channel_width():
    """Performance mode (bf16 activations, float32 master weights) at the production channel widths (64 features, 64 -> 128 -> 64 encoder,
    64-channel TCN, K = 64 codes of 64 dimensions): 20 optimiser steps of the HIP trainer next to the float64 oracle trainer from the
    same initial state on the same tiles.  bf16 cannot reproduce the trajectory bit for bit (indices flip on near-ties once the latents
    differ in the 3rd digit); the loss must stay within 2 % of the oracle's at every step and end lower than it started."""
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer
    torch.manual_seed(3)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    pool = torch.randn(2, 1, 5, 32, 32, 64, generator=torch.Generator().manual_seed(5))    # (one tile per step: the float64 oracle sets the test's run time)
    m.init_codebook_from_tiles(pool[0].to(torch.bfloat16).to(DEV), seed=1)
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    tr = VQVAETrainer(m, lr=3e-4, total_steps=20)
    otr = O.OracleTrainer(sd, dict(beta=0.25), lr=3e-4, total_steps=20)
    la, lb = [], []
    for i in range(20):
        t = pool[i % 2].to(torch.bfloat16)                                        # the oracle sees the same bf16-representable tiles
        la.append(float(tr.step(t.to(DEV))["loss"].detach()))
        lb.append(float(otr.step(t.double())["loss"]))
    rel = [abs(a - b) / abs(b) for a, b in zip(la, lb)]
    assert max(rel) <= 2e-2, (max(rel), la, lb)
    assert la[-1] < la[0] and lb[-1] < lb[0]


def test_single_rank_rccl_reducer_path_matches_plain_trainer(golden_dir):
    """The data-parallel path on ONE rank (RCCL communicator of size 1, hooks forced): gradients flow through the multi-tensor
    pack -> flat buckets -> HipAdamW-in-place route and must reproduce the plain trainer's loss trajectory exactly."""
    import torch.distributed as dist
    from frl_hip.parallel import BucketedGradAllReduce
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    plain = VQVAETrainer(_vqvae_from_fixture(fx), lr=1e-3, total_steps=10)
    ref = [plain.step(tiles[i])["loss"].item() for i in range(3)]
    runs = []
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29731", rank=0, world_size=1, device_id=torch.device(DEV))
    try:
        m = _vqvae_from_fixture(fx)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
        tr.reducer = BucketedGradAllReduce([(n, p) for n, p in m.named_parameters() if p.requires_grad], force_hooks=True)
        assert tr.reducer.active and tr.hip_opt
        got = [tr.step(tiles[i])["loss"].item() for i in range(3)]
        # the isfinite flag rides in the last gradient bucket: a bad batch is skipped through that route as well
        before = {n: p.detach().clone() for n, p in m.named_parameters()}
        bad = tiles[0].clone()
        bad[0, 0, 0, 0, 0] = float("inf")
        tr.step(bad)
        assert all(torch.equal(p.detach(), before[n]) for n, p in m.named_parameters())
        assert tr.opt.applied_and_skipped == (3, 1)
        # The data-parallel step as ONE captured graph: bucket packs, the RCCL all-reduce calls on the side stream and the optimizer that
        # reads the buckets in place are recorded with forward / backward (VQVAETrainer.graph_supported() now admits a GPU reducer).
        # Same kernels, same order: parameters after good / bad / good steps equal the eager data-parallel trainer's bit for bit, with a
        # lambda_vq(step) schedule read from its device scalar at replay time.
        from frl_hip.training.schedules import LambdaVQSchedule
        seq = [tiles[0], tiles[1], bad, tiles[2], tiles[0]]
        for graphed in (False, True):
            m2 = _vqvae_from_fixture(fx)
            sched = LambdaVQSchedule(lambda_vq=1.0, enable=True, schedule="linear", start=0, duration=4, floor=0.25, ceil=1.0)
            t2 = VQVAETrainer(m2, lr=1e-3, total_steps=10, lambda_vq_schedule=sched)
            t2.reducer = BucketedGradAllReduce([(n, p) for n, p in m2.named_parameters() if p.requires_grad], force_hooks=True)
            assert t2.graph_supported() and m2.lambda_vq_dev is not None
            losses = [float((t2.step_graphed(t) if graphed else t2.step(t))["loss"].detach()) for t in seq]
            torch.cuda.synchronize()
            runs.append((m2, t2, losses))
        (ma, ta, la), (mb, tb, lb) = runs
        assert len(tb._graphs) >= 3 and ta.opt.applied_and_skipped == tb.opt.applied_and_skipped == (4, 1)
        assert [x for x in la if x == x] == [x for x in lb if x == x]
        for (n, p_), (_, q_) in zip(ma.named_parameters(), mb.named_parameters()):
            assert torch.equal(p_, q_), n
    finally:
        # the graphs hold captured RCCL collectives of this communicator: release them before the process group shuts it down
        torch.cuda.synchronize()
        for _, t_, _ in runs:
            t_.__dict__.pop("_graphs", None)
        dist.destroy_process_group()
    assert got == ref, (got, ref)


def test_nonfinite_batch_is_skipped_on_device(golden_dir):
    """step.py:1057-1074 semantics without a host sync: a non-finite loss leaves parameters, moments and the update count untouched."""
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    m = _vqvae_from_fixture(fx)
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    tr.step(tiles[0])
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    bad = tiles[1].clone()
    bad[0, 0, 0, 0, 0] = float("nan")
    out = tr.step(bad)
    assert not torch.isfinite(out["loss"]).item()
    for n, p in m.named_parameters():
        assert torch.equal(p.detach(), before[n]), n
    assert tr.opt.applied_and_skipped == (1, 1) and tr.n_skipped == 1
    l2 = tr.step(tiles[1])["loss"].item()                      # training continues; the update count did not advance on the bad batch
    assert np.isfinite(l2) and tr.opt.applied_and_skipped == (2, 1)
    ref = VQVAETrainer(_vqvae_from_fixture(fx), lr=1e-3, total_steps=10)
    ref.step(tiles[0])
    ref.step_idx += 1                                          # the LR schedule advances per batch, skipped or not
    assert abs(ref.step(tiles[1])["loss"].item() - l2) < 1e-6
    for (n, p), (_, q) in zip(m.named_parameters(), ref.model.named_parameters()):
        assert (p - q).abs().max().item() <= 1e-6, n


def test_bf16_mode_tracks_oracle_and_indices_are_exact(golden_dir):
    """Performance mode: bf16 storage cannot meet 1e-5; check agreement at bf16 resolution and that the VQ indices are the
    exact float64 argmin of the bf16 latents the encoder actually produced."""
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    m = _vqvae_from_fixture(fx, torch.bfloat16)
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    out = m.forward_tiles(tiles[0])
    assert abs(out["loss"].item() - float(fx["loss"])) < 0.05 * float(fx["loss"])
    z = out["z_type"].detach().float().cpu().reshape(-1, 8)
    e = m.quant.codebook.detach().cpu().to(torch.bfloat16).float()
    idx_ref = O.vq_argmin_np(z.numpy(), e.numpy())
    assert np.array_equal(out["idx"].cpu().numpy().astype(np.int64), idx_ref)
    out["loss"].backward()
    for name, p in m.named_parameters():
        ref = fx["grad." + name]
        assert np.isfinite(p.grad.cpu().numpy()).all()
        if np.abs(ref).max() > 1e-4:
            cos = float((p.grad.cpu().double().flatten() @ torch.from_numpy(ref).double().flatten()) /
                        (p.grad.cpu().double().norm() * np.linalg.norm(ref) + 1e-30))
            assert cos > 0.97, (name, cos)


def test_ema_quantizer_updates_codebook():
    from frl_hip.models import VQVAE
    torch.manual_seed(0)
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, hidden=16, quantizer="ema", z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4).to(DEV).train()
    assert not m.quant.codebook.requires_grad
    before = m.quant.codebook.detach().clone()
    tile = torch.randn(2, 5, 8, 8, 8, device=DEV)
    out = m.forward_tiles(tile)
    z = out["z_type"].detach().reshape(-1, 8).cpu().double()
    idx = out["idx"].cpu().long()
    cb, cnt, sm = O.vq_ema_update(before.cpu().double(), torch.zeros(16, dtype=torch.float64), before.cpu().double(), z, idx, 0.99, 1e-5)
    assert (m.quant.codebook.detach().cpu().double() - cb).abs().max() <= 1e-5 * max(1.0, cb.abs().max().item())
    out["loss"].backward()
    assert m.quant.codebook.grad is None


def test_nonfinite_batch_leaves_ema_and_codebook_manager_untouched():
    """The isfinite guard covers the state forward() would mutate: with quantizer='ema' and a CodebookManager attached, an Inf tile
    must change neither the EMA running averages, the codebook, nor the manager's usage window, and its (non-finite) rows must never
    seed a code -- step.py:1057-1074 skips the whole batch."""
    from frl_hip.models import VQVAE
    from frl_hip.training.codebook_manager import CodebookManager
    from frl_hip.training.trainer import VQVAETrainer
    torch.manual_seed(0)
    m = VQVAE(in_features=8, codebook_size=16, emb_dim=8, hidden=16, quantizer="ema", z_phase_dim=4, type_encoder_channels=(16, 8),
              type_encoder_dropout=0.0, type_encoder_num_groups=4, spatial_conv_gate_hidden=8, phase_tcn_channels=(8, 8, 8),
              phase_tcn_dropout=0.0, phase_tcn_num_groups=4).to(DEV)
    mgr = CodebookManager(num_codes=16, code_dim=8, reset_every=2, min_count=1)
    m.attach_codebook_manager(mgr)
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    assert tr.hip_opt and m.defer_codebook_hooks and m.quant.defer_ema
    g = torch.Generator().manual_seed(3)
    good = [torch.randn(2, 5, 8, 8, 8, generator=g).to(DEV) for _ in range(3)]
    cb0 = m.quant.codebook.detach().clone()
    tr.step(good[0])
    cb1, n1, s1 = m.quant.codebook.detach().clone(), m.quant.ema_count.clone(), m.quant.ema_sum.clone()
    assert not torch.equal(cb0, cb1)                                  # the good batch did move the codebook
    w1 = mgr.window.clone()
    assert int(w1.sum()) == 2 * 8 * 8
    bad = good[1].clone()
    bad[0, 0, 0, 0, 0] = float("inf")
    out = tr.step(bad)                                                # reset_every = 2: a revival pass runs right after this step
    assert not torch.isfinite(out["loss"]).item()
    assert torch.equal(m.quant.codebook.detach(), cb1) and torch.equal(m.quant.ema_count, n1) and torch.equal(m.quant.ema_sum, s1)
    assert torch.isfinite(m.quant.codebook).all() and int(mgr.revived.item()) == 0 and int(mgr.window.sum()) == 0
    assert tr.opt.applied_and_skipped == (1, 1)
    out = tr.step(good[2])
    assert torch.isfinite(out["loss"]).item() and torch.isfinite(m.quant.codebook).all()
    assert not torch.equal(m.quant.codebook.detach(), cb1) and int(mgr.window.sum()) == 2 * 8 * 8


def test_graph_captured_step_reproduces_the_eager_trajectory(golden_dir):
    """VQVAETrainer.step_graphed replays the whole step (both streams of the forward, autograd backward, clip + AdamW, codebook
    hooks) from a captured hipGraph.  Same kernels on the same inputs: parameters after a run that mixes good batches, a
    non-finite batch (skipped by the device flag inside the graph) and a per-step cosine learning rate (device word) must EQUAL
    those of the eager trainer, and capturing must not consume optimizer steps."""
    from frl_hip.training.codebook_manager import CodebookManager
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    tiles = [t.contiguous() for t in torch.from_numpy(fx["tiles"]).float().to(DEV)]
    bad = tiles[1].clone()
    bad[0, 0, 0, 0, 0] = float("nan")
    seq = [tiles[0], tiles[1], bad, tiles[2], tiles[0], tiles[1]]

    def run(graphed):
        m = _vqvae_from_fixture(fx)
        m.attach_codebook_manager(CodebookManager(num_codes=16, code_dim=8, reset_every=4, min_count=1))
        tr = VQVAETrainer(m, lr=1e-3, total_steps=8)
        losses = []
        for t in seq:
            out = tr.step_graphed(t) if graphed else tr.step(t)
            losses.append(float(out["loss"].detach()))
        torch.cuda.synchronize()
        return m, tr, losses

    m0, tr0, l0 = run(False)
    m1, tr1, l1 = run(True)
    assert tr1.graph_supported() and len(tr1._graphs) == 4                      # one graph per distinct input buffer
    assert tr0.opt.applied_and_skipped == tr1.opt.applied_and_skipped == (5, 1)
    assert np.isnan(l1[2]) and np.isnan(l0[2])
    assert [a for a in l0 if a == a] == [a for a in l1 if a == a]
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), n
    assert torch.equal(m0.codebook_manager.window, m1.codebook_manager.window)
    assert int(m0.codebook_manager.revived.item()) == int(m1.codebook_manager.revived.item())


def test_graphed_step_with_codebook_manager_over_several_revivals(golden_dir):
    """Graph replays run no Python, so the CodebookManager's handles on the encoder rows / guard flag of "the current batch" must be
    those of the graph that just ran: 8 steps over a ring of 3 input buffers with reset_every = 3 (the ring size does not divide it)
    give two revivals, the second one after the manager has forgotten its rows once; a 9th..12th step on fresh tensors overflows
    MAX_GRAPHS = 2 into the trainer's staging graph, which must leave the caller's tensors untouched.  A codebook far from the data
    guarantees dead codes.  Parameters, usage window and revival count equal the eager trainer's bit for bit, and the warm-up steps of
    the first capture leave nothing in the usage window."""
    from frl_hip.training.codebook_manager import CodebookManager
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    ring = [t.contiguous() for t in torch.from_numpy(fx["tiles"]).float().to(DEV)][:3]
    extra = [(ring[i % 3] * (1.0 + 0.01 * i)).contiguous() for i in range(4)]
    keep = [t.clone() for t in ring + extra]

    def run(graphed):
        m = _vqvae_from_fixture(fx)
        with torch.no_grad():
            m.quant.codebook[8:] += 50.0                                          # half of the codes can never win: dead
        mgr = CodebookManager(num_codes=16, code_dim=8, reset_every=3, min_count=1)
        m.attach_codebook_manager(mgr)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=16)
        tr.MAX_GRAPHS = 2
        windows = []
        for i in range(12):
            t = ring[i % 3] if i < 8 else extra[i - 8]
            tr.step_graphed(t) if graphed else tr.step(t)
            windows.append(mgr.window.clone())
        torch.cuda.synchronize()
        return m, tr, mgr, windows

    m0, tr0, g0, w0 = run(False)
    m1, tr1, g1, w1 = run(True)
    assert tr1.graph_supported() and set(tr1._graphs) >= {"staging"} and len(tr1._graphs) == 3
    assert int(w1[0].sum()) == ring[0].shape[0] * ring[0].shape[2] * ring[0].shape[3]  # one batch of rows, not 1 + 2 warm-up batches
    for a, b in zip(w0, w1):
        assert torch.equal(a, b)
    assert int(g0.revived.item()) == int(g1.revived.item()) >= 8 and g1.steps == 12
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), n
    for t, k in zip(ring + extra, keep):
        assert torch.equal(t, k)


def test_graphed_step_sees_state_edited_behind_the_trainer(golden_dir):
    """load_state_dict / manual edits between replays: the packed weight images and the codebook image are rebuilt before the next
    replay, exactly as the eager step does (one step on stale images would apply gradients of the old weights to the new ones)."""
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    tiles = [t.contiguous() for t in torch.from_numpy(fx["tiles"]).float().to(DEV)]

    def run(graphed):
        m = _vqvae_from_fixture(fx)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=8)
        f = tr.step_graphed if graphed else tr.step
        f(tiles[0]); f(tiles[0])
        with torch.no_grad():
            m.encoder.layers[0].weight.mul_(0.5)
            m.quant.codebook.mul_(-1.0)
        out = f(tiles[0])
        loss = float(out["loss"].detach())
        torch.cuda.synchronize()
        return m, loss

    m0, l0 = run(False)
    m1, l1 = run(True)
    assert l0 == l1
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), n


def test_weight_image_cache_changes_nothing_but_the_launch_count():
    """VQVAETrainer(pack_cache=True): the packed MFMA fragment images of all conv weights are kept in the trainer's arena and rewritten
    by one launch behind the optimizer.  The generic repack kernel must reproduce the per-call pack kernels bit for bit: three steps
    with and without the cache end in EQUAL parameters (bf16 hot kernels: pointwise, 3x3, fused TCN and decoder images), and a weight
    edited behind the trainer's back (load_state_dict) is picked up before the next step."""
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer

    def make():
        torch.manual_seed(0)
        m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
                  compute_dtype=torch.bfloat16).to(DEV)
        with torch.no_grad():
            m.quant.codebook.copy_(torch.randn(64, 64, generator=torch.Generator().manual_seed(7)))
        return m

    g = torch.Generator().manual_seed(11)
    tiles = [torch.randn(2, 5, 32, 32, 64, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3)]
    runs = []
    for cached in (False, True):
        m = make()
        tr = VQVAETrainer(m, lr=1e-3, total_steps=10, pack_cache=cached)
        losses = [float(tr.step(t)["loss"].detach()) for t in tiles]
        if cached:
            assert tr.pack_cache is not None and tr.pack_cache.images >= 20
            n_img = tr.pack_cache.images
        else:
            assert tr.pack_cache is None
        # edit a weight behind the trainer's back, then one more step: both must see the new value
        with torch.no_grad():
            m.encoder.layers[0].weight.mul_(0.5)
        losses.append(float(tr.step(tiles[0])["loss"].detach()))
        if cached:
            assert tr.pack_cache.images == n_img                       # nothing new to register after the first step
        runs.append((m, losses))
    (m0, l0), (m1, l1) = runs
    assert l0 == l1
    for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
        assert torch.equal(p, q), n


def test_deferred_reductions_change_nothing_but_the_launch_count():
    """VQVAETrainer(defer_reductions=True): the slab reductions behind the weight-gradient kernels of the backward pass (fused TCN blocks,
    3x3 / 1x1 weight gradients, fused encoder / decoders / FiLM / mixing heads, codebook gradient) are parked and run in ONE launch before
    the optimizer (csrc/defer.hip).  Same summation order: three eager steps and three graph replays with and without deferral end in EQUAL
    parameters; the deferred backward must have parked at least ten jobs; and a backward in which autograd sums two gradients of one
    parameter (used twice) is refused instead of reading a tensor nothing has written yet."""
    from frl_hip import _lib, ops
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer

    def make():
        torch.manual_seed(0)
        m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
                  compute_dtype=torch.bfloat16).to(DEV)
        with torch.no_grad():
            m.quant.codebook.copy_(torch.randn(64, 64, generator=torch.Generator().manual_seed(7)))
        return m

    g = torch.Generator().manual_seed(13)
    tiles = [torch.randn(2, 5, 32, 32, 64, generator=g).to(torch.bfloat16).to(DEV) for _ in range(3)]
    lib = _lib.load()
    for graphed in (False, True):
        runs = []
        for defer in (False, True):
            m = make()
            tr = VQVAETrainer(m, lr=1e-3, total_steps=10, defer_reductions=defer)
            seen = []
            if defer and not graphed:                                  # count the parked jobs of the first step
                orig_exit = ops.deferred_reductions.__exit__

                def counting_exit(self, et, ev, tb):
                    seen.append(lib.frl_defer_pending())
                    return orig_exit(self, et, ev, tb)
                ops.deferred_reductions.__exit__ = counting_exit
            try:
                losses = [float((tr.step_graphed(t) if graphed else tr.step(t))["loss"].detach()) for t in tiles]
            finally:
                if defer and not graphed:
                    ops.deferred_reductions.__exit__ = orig_exit
            if defer and not graphed:
                assert seen and min(seen) >= 10, seen
            assert lib.frl_defer_pending() == 0
            runs.append((m, losses))
        (m0, l0), (m1, l1) = runs
        assert l0 == l1, (graphed, l0, l1)
        for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
            assert torch.equal(p, q), (graphed, n)

    # a parameter with two consumers: autograd adds the two weight gradients at backward time -> refused
    from frl_hip import functional as Fh
    w = torch.nn.Parameter(torch.randn(64, 64, device=DEV) * 0.1)
    x = torch.randn(4096, 64, device=DEV).to(torch.bfloat16).requires_grad_(True)
    with pytest.raises(RuntimeError, match="deferred_reductions"):
        y = Fh.conv1x1(Fh.conv1x1(x, w), w)
        with ops.deferred_reductions([w]):
            y.float().sum().backward()
    assert lib.frl_defer_pending() == 0 and lib.frl_defer_begin() == 0 and lib.frl_defer_abort() == 0     # nothing left open


def test_configs1_train_step_end_to_end():
    """BASELINE configs[1] as bench.py measures it (256 tiles of 5x32x32x64, K = 512, d = 64, bf16): one full train step through the
    HIP path -- VQ indices are the exact float64 argmin of the latents the encoder produced, every loss term is finite, parameters move."""
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=512, emb_dim=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0,
              compute_dtype=torch.bfloat16).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(512, 64, generator=torch.Generator().manual_seed(7)))
    tr = VQVAETrainer(m, lr=1e-4, total_steps=100)
    tile = torch.randn(256, 5, 32, 32, 64, generator=torch.Generator().manual_seed(1234)).to(torch.bfloat16).to(DEV)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    e = m.quant.codebook.detach().cpu().to(torch.bfloat16).double().numpy()      # the kernel rounds the codebook to bf16 for the MFMA
    out = tr.step(tile)
    torch.cuda.synchronize()
    for k in ("loss", "l_type", "l_phase", "vq_loss", "perplexity", "grad_norm"):
        assert torch.isfinite(out[k]).all(), k
    assert tr.opt.applied_and_skipped == (1, 0)
    z = out["z_type"].detach().float().cpu().reshape(-1, 64).double().numpy()
    idx = out["idx"].cpu().numpy().astype(np.int64)
    assert idx.shape == (256 * 32 * 32,)
    ref = np.empty_like(idx)
    e2 = (e * e).sum(1)
    for lo in range(0, z.shape[0], 32768):                                          # float64 brute force, first index on ties
        zz = z[lo:lo + 32768]
        ref[lo:lo + 32768] = np.argmin((zz * zz).sum(1)[:, None] - 2.0 * zz @ e.T + e2[None, :], axis=1)
    bad = np.flatnonzero(ref != idx)
    if bad.size:                                                                    # float64 ties of the expanded form: compare distances
        d_ref = ((z[bad] - e[ref[bad]]) ** 2).sum(1)
        d_got = ((z[bad] - e[idx[bad]]) ** 2).sum(1)
        assert np.all(d_got <= d_ref + 1e-9 * np.maximum(1.0, d_ref)) and np.all((d_got < d_ref - 1e-12) | (idx[bad] <= ref[bad])), bad[:8]
    moved = sum(int(not torch.equal(p.detach(), before[n])) for n, p in m.named_parameters())
    assert moved == len(before)


@pytest.mark.parametrize("name,kw,tile_shape", [
    # BASELINE configs[3]: large codebook K = 8192, d = 128 (encoder channels [128, 128])
    ("cfg4", dict(codebook_size=8192, emb_dim=128), (2, 5, 32, 32, 64)),
    # BASELINE configs[4]: type + phase dual codebook, time = 10, 64 x 64 tiles, K = 1024 each
    ("cfg5", dict(codebook_size=1024, emb_dim=64, phase_codebook_size=1024), (1, 10, 64, 64, 64)),
])
def test_other_baseline_configs_run_and_indices_are_exact(name, kw, tile_shape):
    """The remaining BASELINE.json configurations as parity cases: one bf16 train step runs, every output is finite and the
    (type and phase) code indices are the exact float64 arg-min of the latents the encoder produced."""
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer
    torch.manual_seed(0)
    m = VQVAE(in_features=64, beta=0.25, type_encoder_dropout=0.0, phase_tcn_dropout=0.0, compute_dtype=torch.bfloat16, **kw).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(m.quant.codebook.shape, generator=torch.Generator().manual_seed(7)))
        if hasattr(m, "quant_phase"):
            m.quant_phase.codebook.copy_(torch.randn(m.quant_phase.codebook.shape, generator=torch.Generator().manual_seed(8)) * 0.5)
    tile = torch.randn(*tile_shape, generator=torch.Generator().manual_seed(1)).to(DEV)
    out = m.forward_tiles(tile)
    assert torch.isfinite(out["loss"]).item()
    d = m.quant.emb_dim
    z = out["z_type"].detach().float().cpu().reshape(-1, d)
    e = m.quant.codebook.detach().cpu().to(torch.bfloat16).float()
    assert np.array_equal(out["idx"].cpu().numpy().astype(np.int64), O.vq_argmin_np(z.numpy(), e.numpy()))
    if "idx_phase" in out:
        zp = out["z_phase"].detach().float().cpu().reshape(-1, m.z_phase_dim)
        ep = m.quant_phase.codebook.detach().cpu().to(torch.bfloat16).float()
        assert np.array_equal(out["idx_phase"].cpu().numpy().astype(np.int64), O.vq_argmin_np(zp.numpy(), ep.numpy()))
    tr = VQVAETrainer(m, lr=1e-4, total_steps=10)
    res = tr.step(tile)
    assert torch.isfinite(res["loss"]).item() and torch.isfinite(res["grad_norm"]).all().item()
    assert tr.opt.applied_and_skipped == (1, 0)
    for n, p in m.named_parameters():
        assert torch.isfinite(p).all().item(), n


def test_training_mode_dropout_runs_on_the_hip_path():
    """The live reference configuration trains with input_dropout > 0 and phase_tcn dropout 0.1 (frl_repr_model_v1.yaml:41-45,78):
    a bf16 train step in that mode runs through the HIP kernels, is stochastic, stays finite, and eval() is deterministic."""
    from frl_hip.models import VQVAE
    from frl_hip.training.trainer import VQVAETrainer
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=64, emb_dim=64, type_encoder_dropout=0.1, type_encoder_input_dropout=0.05,
              phase_tcn_dropout=0.1, compute_dtype=torch.bfloat16).to(DEV)
    tile = torch.randn(2, 5, 32, 32, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    m.train()
    a = m.forward_tiles(tile)["loss"].item()
    b = m.forward_tiles(tile)["loss"].item()
    assert np.isfinite(a) and np.isfinite(b) and a != b                         # two dropout realisations
    m.eval()
    assert m.forward_tiles(tile)["loss"].item() == m.forward_tiles(tile)["loss"].item()
    tr = VQVAETrainer(m, lr=1e-4, total_steps=10)
    out = tr.step(tile)
    assert torch.isfinite(out["loss"]).item() and tr.opt.applied_and_skipped == (1, 0)
    m.set_input_dropout_rate(0.2)                                              # per-epoch schedule hook of the reference trainer
    assert torch.isfinite(tr.step(tile)["loss"]).item()


def test_two_rank_data_parallel_matches_single_process(golden_dir, tmp_path):
    """SURVEY 8e acceptance on a small scale: two data-parallel ranks (each half of the batch) end up with the parameters of one
    process trained on the whole batch.  The ranks share the GPU over gloo; everything else is the production route."""
    import subprocess
    import sys
    from frl_hip.training.trainer import VQVAETrainer
    fx_path = os.path.join(golden_dir, "vqvae_tiny_seed0.npz")
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    if fx["tiles"].shape[1] % 2:
        pytest.skip("fixture batch is odd")
    out = str(tmp_path / "ddp_params.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29641", os.path.join(os.path.dirname(__file__), "ddp_gpu_worker.py"), out, fx_path],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    m = _vqvae_from_fixture(fx)
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    for step in range(2):
        tr.step(tiles[step])
    for n, p in m.named_parameters():
        ref = p.detach().cpu().numpy()
        assert np.abs(got[n] - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), n


def test_checkpoint_resume_continues_the_trajectory(golden_dir, tmp_path):
    """Reference-format checkpoint (model + HipAdamW state) written after two steps; a fresh trainer resumed from it takes the same
    third step as the original, bit for bit."""
    from frl_hip.training.checkpointing import CheckpointManager, CheckpointPolicy, build_checkpoint_state, resume_from_checkpoint
    from frl_hip.training.trainer import VQVAETrainer
    fx = _load(golden_dir, "vqvae_tiny_seed0")
    tiles = torch.from_numpy(fx["tiles"]).float().to(DEV)
    m = _vqvae_from_fixture(fx)
    tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
    for i in range(2):
        tr.step(tiles[i])
    mgr = CheckpointManager(tmp_path, CheckpointPolicy(monitor="train/loss"))
    mgr.save(0, build_checkpoint_state(m, tr.opt, epoch=0, metrics={"train/loss": 1.0}), {"train/loss": 1.0})
    want = tr.step(tiles[2])["loss"].item()
    m2 = _vqvae_from_fixture(fx)
    tr2 = VQVAETrainer(m2, lr=1e-3, total_steps=10)
    start, _, _ = resume_from_checkpoint(m2, tr2.opt, tmp_path, device=DEV)
    assert start == 1
    tr2.step_idx = 2                                                     # the LR schedule position travels with the caller's step count
    got = tr2.step(tiles[2])["loss"].item()
    assert got == want
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n


def test_export_codebook_bundle(tmp_path):
    from frl_hip.data.normalization import NormPreset
    from frl_hip.models import VQVAE
    from frl_hip.training.export import decode_codebook, export_codebook
    torch.manual_seed(0)
    m = VQVAE(in_features=64, codebook_size=32, emb_dim=64, compute_dtype=torch.float32).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(32, 64))
    dec = decode_codebook(m)
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    ref = O.decoder_forward(sd, sd["quant.codebook"].reshape(1, 32, 1, 64).permute(0, 3, 1, 2), "decoder_type.").permute(0, 2, 3, 1).reshape(32, 64)
    assert maxabs(dec, ref) < 1e-5
    names = [f"f{i:03d}" for i in range(64)]
    presets = [NormPreset("zscore")] * 64
    stats = [{"mean": float(i), "sd": 2.0} for i in range(64)]
    path = export_codebook(m, tmp_path / "cb", names, presets, stats, usage=torch.full((32,), 1 / 32), years=[2001, 2002], csv=True)
    z = np.load(path)
    assert z["cont_KT"].shape == (64, 64) and z["code_id"].tolist()[:3] == [0, 0, 1] and z["year"].tolist()[:3] == [2001, 2002, 2001]
    assert np.abs(z["cont_KT"][0] - (dec[0].cpu().numpy() * 2.0 + np.arange(64))).max() < 1e-4
    assert z["codes_K3"].shape == (32, 3) and abs(z["codes_K3"][5, 1] - 1 / 32) < 1e-12
    meta = json.loads(str(z["meta"]))
    assert meta["K"] == 32 and meta["T"] == 2 and meta["cont_names"] == names
    assert (tmp_path / "cb_cont_KT.csv").exists() and (tmp_path / "cb_codes_K3.csv").exists()
