"""Code-map inference on the GPU: the decode gather (csrc/codes.hip), VQVAE.encode_tiles / decode_codes against forward_tiles, the
inference variant of the phase chain, VQVAETrainer.evaluate and inference.encode_store."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ gather kernel
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("k,f", [(512, 64), (1024, 64), (512, 12), (1024, 12)])
def test_decode_gather_matches_torch_indexing(dtype, k, f):
    from frl_hip import ops
    g = torch.Generator().manual_seed(k + f)
    table = torch.randn(k, f, generator=g, dtype=torch.float64).to(dtype).to(DEV)
    ops.index_errors()
    for p in (0, 1, 17, 1000, 262144 + 5):
        idx = torch.randint(0, k, (p,), generator=g, dtype=torch.int32).to(DEV)
        out = ops.decode_codes(idx, table)
        assert out.shape == (p, f) and out.dtype == dtype
        assert torch.equal(out, table[idx.long()]), (p, k, f, dtype)
    idx64 = torch.randint(0, k, (3, 7, 5), generator=g).to(DEV)                 # int64, any shape
    assert torch.equal(ops.decode_codes(idx64, table), table[idx64])
    assert not ops.index_errors()


def test_decode_gather_out_of_range_indices(monkeypatch):
    from frl_hip import ops
    k, f = 512, 64
    table = torch.randn(k, f, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16).to(DEV)
    ops.index_errors()
    idx = torch.tensor([3, -1, -k, 5], dtype=torch.int32, device=DEV)           # negatives in [-K, 0) wrap
    assert torch.equal(ops.decode_codes(idx, table), table[torch.tensor([3, k - 1, 0, 5], device=DEV)])
    assert not ops.index_errors()
    idx = torch.tensor([k, -k - 1, 7, 1 << 30], dtype=torch.int32, device=DEV)  # clamped and flagged
    assert torch.equal(ops.decode_codes(idx, table), table[torch.tensor([k - 1, 0, 7, k - 1], device=DEV)])
    assert ops.index_errors() and not ops.index_errors()
    monkeypatch.setenv("FRL_HIP_CHECK_INDICES", "1")
    with pytest.raises(IndexError):
        ops.decode_codes(torch.tensor([0, k], dtype=torch.int32, device=DEV), table)
    ops.decode_codes(torch.tensor([0, -1], dtype=torch.int32, device=DEV), table)   # in range: no raise
    ops.index_errors()


# ------------------------------------------------------------------------------------------------ model-level
def _model(dtype=torch.bfloat16, quantizer="st", phase_k=1024, k=512, seed=0, dropout=0.1):
    from frl_hip.models import VQVAE
    torch.manual_seed(seed)
    m = VQVAE(in_features=64, codebook_size=k, emb_dim=64, beta=0.25, quantizer=quantizer, phase_codebook_size=phase_k,
              type_encoder_dropout=dropout, phase_tcn_dropout=dropout, compute_dtype=dtype).to(DEV)
    with torch.no_grad():
        m.quant.codebook.copy_(torch.randn(k, 64, generator=torch.Generator().manual_seed(7)))
        if quantizer == "ema":
            m.quant.ema_sum.copy_(m.quant.codebook)
            m.quant.ema_count.fill_(1.0)
        if phase_k:
            m.quant_phase.codebook.copy_(torch.randn(phase_k, m.z_phase_dim, generator=torch.Generator().manual_seed(8)) * 0.5)
    return m


def _tiles(b=8, seed=1):
    return torch.randn(b, 5, 32, 32, 64, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _check_against_forward(m, tile, exact_recon: bool = True):
    m.eval()
    with torch.no_grad():
        ref = m.forward_tiles(tile, return_recon=True)
    m.train()                                                                   # encode_tiles runs in eval mode whatever the flag
    enc = m.encode_tiles(tile, return_latents=True)
    assert m.training
    b = tile.shape[0]
    assert enc["idx"].dtype == torch.int32 and enc["idx"].shape == (b, 32, 32)
    assert enc["idx_phase"].shape == (b, 5, 32, 32)
    assert torch.equal(enc["idx"].reshape(-1), ref["idx"])
    assert torch.equal(enc["idx_phase"].reshape(-1), ref["idx_phase"])
    assert torch.equal(enc["z_type"], ref["z_type"])
    assert torch.equal(enc["z_phase"], ref["z_phase"])
    assert torch.equal(enc["counts"], torch.bincount(ref["idx"].long(), minlength=m.quant.codebook_size).int())
    assert float(enc["perplexity"]) == float(ref["perplexity"])
    dec = m.decode_codes(enc["idx"], enc["idx_phase"])
    assert dec["xhat_type"].shape == (b, 32, 32, 64) and dec["xhat_phase"].shape == (b, 5, 32, 32, 64)
    for name in ("xhat_type", "xhat_phase"):
        got, want = dec[name], ref[name].reshape(dec[name].shape)
        assert got.dtype == want.dtype
        if exact_recon:
            assert torch.equal(got, want), name
        else:
            torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6 * float(want.abs().max()))
    return enc


def test_encode_decode_match_forward_tiles_bf16():
    m = _model(torch.bfloat16)
    _check_against_forward(m, _tiles(8))


def test_encode_decode_match_forward_tiles_f32():
    m = _model(torch.float32)
    _check_against_forward(m, _tiles(8), exact_recon=False)


def test_encode_tiles_is_batch_invariant():
    for dtype in (torch.bfloat16, torch.float32):
        m = _model(dtype)
        tile = _tiles(8, seed=3)
        full = m.encode_tiles(tile)
        for i in range(tile.shape[0]):
            one = m.encode_tiles(tile[i:i + 1])
            assert torch.equal(one["idx"][0], full["idx"][i]), (dtype, i)
            assert torch.equal(one["idx_phase"][0], full["idx_phase"][i]), (dtype, i)


def test_encode_tiles_mask_and_phase_only_when_needed():
    m = _model(torch.bfloat16, phase_k=0)
    tile = _tiles(2)
    mask = torch.ones(2, 5, 32, 32, dtype=torch.uint8, device=DEV)
    mask[0, 2, 3, 4] = 0
    enc = m.encode_tiles(tile, mask)
    assert "idx_phase" not in enc and "z_phase" not in enc
    assert enc["valid"].dtype == torch.bool and not bool(enc["valid"][0, 3, 4]) and int(enc["valid"].sum()) == 2 * 32 * 32 - 1
    enc = m.encode_tiles(tile, return_latents=True)
    assert "z_phase" in enc and "idx_phase" not in enc
    with pytest.raises(ValueError):
        m.decode_codes(idx_phase=enc["idx"])


def _state_snapshot(m):
    st = {n: t.detach().clone() for n, t in list(m.named_parameters()) + list(m.named_buffers())}
    lc = [(q.last_counts, q.last_stats) for q in m._quantizers()]
    return st, lc


def _assert_state_equal(m, snap):
    st, lc = snap
    for n, t in list(m.named_parameters()) + list(m.named_buffers()):
        assert torch.equal(t.detach(), st[n]), n
    for q, (c, s) in zip(m._quantizers(), lc):
        assert q.last_counts is c and q.last_stats is s


def test_inference_mutates_nothing():
    from frl_hip.training.codebook_manager import CodebookManager
    from frl_hip.training.trainer import VQVAETrainer
    m = _model(torch.bfloat16, quantizer="ema")
    mgr = CodebookManager(m.quant.codebook_size, 64, reset_every=100)
    m.attach_codebook_manager(mgr)
    tr = VQVAETrainer(m, lr=1e-4, total_steps=10)
    tile = _tiles(4)
    tr.step(tile)                                                              # manager window and EMA state exist
    torch.cuda.synchronize()
    snap = _state_snapshot(m)
    win = None if mgr.window is None else mgr.window.clone()
    m.train()
    rng = torch.cuda.get_rng_state()
    enc = m.encode_tiles(tile)
    m.decode_codes(enc["idx"], enc["idx_phase"])
    res = tr.evaluate([tile, {"tile": tile, "mask": None}])
    assert res["batches"] == 2
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    assert m.training and tr.step_idx == 1
    _assert_state_equal(m, snap)
    assert (win is None and mgr.window is None) or torch.equal(mgr.window, win)


def test_evaluate_matches_manual_loop():
    from frl_hip.training.trainer import VQVAETrainer
    m = _model(torch.bfloat16)
    tr = VQVAETrainer(m, lr=1e-4, total_steps=10)
    batches = [_tiles(4, seed=s) for s in range(3)]
    mask = torch.ones(4, 5, 32, 32, dtype=torch.uint8, device=DEV)
    mask[:, :, :5] = 0
    items = [batches[0], {"tile": batches[1], "mask": mask}, batches[2]]
    res = tr.evaluate(items)
    m.eval()
    sums = dict(loss=0.0, l_type=0.0, l_phase=0.0, vq_loss=0.0)
    counts = torch.zeros(m.quant.codebook_size, dtype=torch.int64, device=DEV)
    counts_p = torch.zeros(m.quant_phase.codebook_size, dtype=torch.int64, device=DEV)
    with torch.no_grad():
        for it in items:
            t, mk = (it["tile"], it["mask"]) if isinstance(it, dict) else (it, None)
            out = m.forward_tiles(t, mk)
            for key in sums:
                sums[key] += float(out[key])
            counts += torch.bincount(out["idx"].long(), minlength=m.quant.codebook_size)
            counts_p += torch.bincount(out["idx_phase"].long(), minlength=m.quant_phase.codebook_size)
    m.train()
    assert res["batches"] == 3 and res["skipped"] == 0
    for key in sums:
        assert abs(res[key] - sums[key] / 3) <= 1e-6 * max(1.0, abs(sums[key] / 3)), key
    assert torch.equal(res["counts"], counts) and torch.equal(res["counts_phase"], counts_p)
    assert res["codes_used"] == int((counts > 0).sum())
    p = counts.double() / counts.sum()
    p = p[p > 0]
    assert abs(res["perplexity"] - float(torch.exp(-(p * p.log()).sum()))) < 1e-6 * res["perplexity"]
    assert tr.evaluate(items, max_batches=1)["batches"] == 1


@pytest.mark.parametrize("graphed", [True, False])
def test_evaluate_interleaved_with_training(graphed):
    from frl_hip.training.trainer import VQVAETrainer
    tiles = [_tiles(4, seed=10 + s) for s in range(4)]
    finals = []
    for with_eval in (False, True):
        m = _model(torch.bfloat16, seed=0, dropout=0.0)
        tr = VQVAETrainer(m, lr=1e-3, total_steps=10)
        step = tr.step_graphed if graphed else tr.step
        for i, t in enumerate(tiles):
            step(t)
            if with_eval and i == 1:
                tr.evaluate([_tiles(2, seed=99), _tiles(6, seed=98)])
        torch.cuda.synchronize()
        finals.append({n: p.detach().clone() for n, p in m.named_parameters()})
    for n in finals[0]:
        assert torch.equal(finals[0][n], finals[1][n]), n


def test_decode_after_optimizer_step_uses_new_weights():
    from frl_hip.training.trainer import VQVAETrainer
    m = _model(torch.bfloat16)
    tr = VQVAETrainer(m, lr=1e-2, total_steps=10)
    tile = _tiles(4)
    enc = m.encode_tiles(tile)
    before = m.decode_codes(enc["idx"], enc["idx_phase"])
    tr.step(tile)
    after = m.decode_codes(enc["idx"], enc["idx_phase"])
    assert not torch.equal(before["xhat_type"], after["xhat_type"])
    assert not torch.equal(before["xhat_phase"], after["xhat_phase"])
    m.eval()
    with torch.no_grad():                                                       # the new weights, through the training forward's route
        zq = m.quant.codebook.detach().to(torch.bfloat16)[enc["idx"].reshape(-1).long()].reshape(4, 32, 32, 64)
        tgt = torch.zeros(4, 32, 32, 64, dtype=torch.bfloat16, device=DEV)
        _, xhat = m._decode_loss(m.decoder_type, zq, tgt, None, True)
    m.train()
    assert torch.equal(after["xhat_type"], xhat)


# ------------------------------------------------------------------------------------------------ store-level
def test_encode_store_small_raster(tmp_path):
    from frl_hip.data import ChunkTileDataset, TilePrefetcher
    from frl_hip.data.tile_store import TileStore, write_tile_store
    from frl_hip.inference import encode_store, place_tiles
    rng = np.random.default_rng(5)
    t, ny, nx, f = 5, 80, 72, 64
    cube = rng.standard_normal((t, ny, nx, f)).astype(np.float32)
    nan_px = [(0, 3, 4), (2, 40, 70), (4, 79, 0), (1, 33, 33)]
    for (tt, y, x) in nan_px:
        cube[tt, y, x, :] = np.nan
    write_tile_store(str(tmp_path / "store"), cube, (64, 64), dtype="float16")
    store = TileStore(str(tmp_path / "store"))
    m = _model(torch.bfloat16)
    res = encode_store(m, store, tile=32, batch_size=3, device=DEV, out=str(tmp_path / "codes"))
    codes, valid = res["codes"], res["valid"]
    assert codes.shape == (ny, nx) and codes.dtype == np.int32 and (codes >= 0).all()
    assert res["codes_phase"].shape == (t, ny, nx) and (res["codes_phase"] >= 0).all()
    exp_valid = np.ones((ny, nx), dtype=np.uint8)
    for (_, y, x) in nan_px:
        exp_valid[y, x] = 0
    np.testing.assert_array_equal(valid, exp_valid)
    assert res["counts"].dtype == np.int64 and int(res["counts"].sum()) == int(exp_valid.sum())
    # per tile, on the same normalised tiles
    ds = ChunkTileDataset(store, 32)
    ref = np.full((ny, nx), -1, dtype=np.int32)
    ref_p = np.full((t, ny, nx), -1, dtype=np.int32)
    for item in TilePrefetcher(ds, [[i] for i in range(len(ds))], device=DEV, depth=2, workers=2):
        enc = m.encode_tiles(item["tile"], item["mask"])
        win = [ds.spatial_window(i) for i in item["indices"]]
        place_tiles(ref, win, enc["idx"].cpu().numpy())
        place_tiles(ref_p, win, enc["idx_phase"].cpu().numpy())
    np.testing.assert_array_equal(codes, ref)
    np.testing.assert_array_equal(res["codes_phase"], ref_p)
    back = np.load(res["path"])
    for key in ("codes", "valid", "codes_phase", "counts"):
        np.testing.assert_array_equal(back[key], res[key])
    assert res["meta"]["shape"] == [t, ny, nx, f] and res["meta"]["codebook_size"] == 512
