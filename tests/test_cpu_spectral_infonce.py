"""CPU checks of the global spectral InfoNCE block (frl_hip.losses.spectral_infonce): the restatement of tests/spectral_infonce_cases.py
against a literal transcription of the reference's loop (frl/training/representation/step.py:751-769), the draw map, the fixtures against
the seeded makers, the epoch-0 tau sweep against its inline formula, and the argument errors, which are raised before the library loads."""
import os

import numpy as np
import pytest
import torch

import frl_oracle as O
import spectral_infonce_cases as SC
from frl_hip.losses import (cross_patch_negatives, global_spectral_infonce, pair_similarity, pair_similarity_stats, spectral_neg_tau_sweep)
from frl_hip.losses.spectral_infonce import negatives_per_patch_pair


def _reference_loop(n_patches):
    """step.py:758-765 as written: the (pi, pj) of every block, in order."""
    out = []
    for pi in range(n_patches):
        for pj in range(n_patches):
            if pi == pj:
                continue
            out.append((pi, pj))
    return out


@pytest.mark.parametrize("s", [2, 3, 5])
def test_block_enumeration_is_the_reference_loop(s):
    assert SC.blocks(s) == _reference_loop(s)
    # and through the pairs: with every draw 0 negative q is (first anchor of pi, first anchor of pj) of its block
    offsets, n_per = SC.offsets_of([3 + p for p in range(s)]), 2
    pairs = SC.negative_pairs(offsets, n_per, np.zeros((n_per * s * (s - 1), 2), dtype=np.int64))
    want = [(offsets[pi], offsets[pj]) for pi, pj in _reference_loop(s) for _ in range(n_per)]
    assert pairs.tolist() == [list(w) for w in want]
    # the array form of the picks is the scalar rule applied in the reference's order
    draws = SC.make_draws(n_per * s * (s - 1), 40 + s)
    want = [(SC.pick(draws[q][0], offsets[pi], offsets[pi + 1]), SC.pick(draws[q][1], offsets[pj], offsets[pj + 1]))
            for q, (pi, pj) in enumerate((pi, pj) for pi, pj in _reference_loop(s) for _ in range(n_per))]
    assert SC.negative_pairs(offsets, n_per, draws).tolist() == [list(w) for w in want]


@pytest.mark.parametrize("count", [1, 2, 3, 7, 329, 964, 2 ** 20 + 1, 2 ** 31 - 1])
def test_draw_map_covers_the_patch_and_never_leaves_it(count):
    lo = 11
    assert SC.pick(0, lo, lo + count) == lo
    assert SC.pick(SC.DRAW_TOP, lo, lo + count) == lo + count - 1
    draws = np.random.default_rng(count % 1000).integers(0, 2 ** 31, 200)
    got = [SC.pick(d, lo, lo + count) for d in draws]
    assert min(got) >= lo and max(got) < lo + count
    if count <= 7:                                                     # every anchor of a small patch is reachable
        assert {SC.pick(d, 0, count) for d in range(0, 2 ** 31, 2 ** 31 // 64)} == set(range(count))


@pytest.mark.parametrize("neg,n,s,want", [(20, 67, 3, 223), (3, 48, 3, 24), (20, 80, 2, 800), (1, 85, 5, 4), (1, 6, 3, 1), (0, 50, 4, 1), (20, 10, 1, 0),
                                          (20, 16 * 329, 16, 438)])
def test_n_per_rule(neg, n, s, want):
    assert SC.n_per_of(neg, n, s) == want == negatives_per_patch_pair(neg, n, s)
    if s > 1:
        assert want == max(1, neg * n // (s * (s - 1)))                # step.py:753-755


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_fixtures_reproduce_from_the_seeded_makers(golden_dir, case):
    """The fixtures hold the reference's outputs; the restatement and the float64 oracles give the same from the seeded inputs."""
    fx = np.load(os.path.join(golden_dir, f"spectral_infonce_{case}.npz"))
    c, inp = SC.CASES[case], SC.make_inputs(case)
    pairs, dist, w = SC.negatives(inp["spec"], inp["offsets"], inp["n_per"], inp["draws"])
    assert np.array_equal(pairs, fx["neg"])
    assert np.abs(dist - fx["neg_dist"]).max() <= 1e-12 * max(1.0, dist.max()) and np.abs(w - fx["neg_w"]).max() <= 1e-12
    pos, _ = O.mutual_knn_pairs_np(inp["spec"], inp["coords"], inp["offsets"], c["k"], SC.MIN_SPATIAL)
    assert np.array_equal(pos, fx["pos"])
    stats = SC.sim_stats(inp["z"], pos) + SC.sim_stats(inp["z"], pairs)
    assert np.abs(np.asarray(stats) - fx["stats"]).max() <= 1e-12 * max(1.0, np.abs(fx["stats"]).max())
    z = torch.from_numpy(inp["z"]).double().requires_grad_(True)
    loss = O.contrastive_loss_oracle(z, torch.from_numpy(pos), torch.from_numpy(pairs), None, torch.from_numpy(w), SC.TEMPERATURE, "l2")
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-12 * max(1.0, abs(float(fx["loss"])))
    assert np.abs(z.grad.numpy() - fx["grad"]).max() <= 1e-12 * max(1.0, np.abs(fx["grad"]).max())
    # what the cases are there for
    assert inp["n_per"] == {"a": 223, "b": 24, "c": 800, "d": 4}[case]
    if case == "c":
        assert (fx["neg_w"] == SC.MIN_W).sum() > 0 and (fx["neg_w"] > SC.MIN_W).sum() > 0
    assert pairs[0].tolist() == [inp["offsets"][0], inp["offsets"][1]]                                  # the planted draws: first anchors,
    assert pairs[1].tolist() == [inp["offsets"][1] - 1, inp["offsets"][2] - 1]                          # then last anchors of block (0, 1)


def test_tau_sweep_equals_the_inline_formula():
    """step.py:774-783 on a CPU tensor.  The sweep evaluates all taus in one batched expression; float32 means of values in [0.05, 1] over a
    few thousand entries agree with the one-row evaluation to a few float32 roundings (1e-6), the quantiles interpolate the same two
    sorted entries (1e-6 as well)."""
    nsd = torch.from_numpy(np.abs(np.random.default_rng(5).standard_normal(3001)).astype(np.float32) * 3.0)
    min_w = 0.05
    got = spectral_neg_tau_sweep(nsd, min_w)
    want = {
        t: {
            'neg_mean': (1.0 - torch.exp(-nsd / t)).clamp(min=min_w, max=1.0).mean().item(),
            'neg_q25': torch.quantile((1.0 - torch.exp(-nsd / t)).clamp(min=min_w, max=1.0), 0.25).item(),
            'neg_q50': torch.quantile((1.0 - torch.exp(-nsd / t)).clamp(min=min_w, max=1.0), 0.50).item(),
        }
        for t in [0.5, 1.0, 2.0, 5.0, 10.0, 20.0, 50.0]
    }
    assert list(got) == list(want)
    for t in want:
        assert set(got[t]) == {"neg_mean", "neg_q25", "neg_q50"}
        for key in want[t]:
            assert abs(got[t][key] - want[t][key]) <= 1e-6, (t, key)
    assert spectral_neg_tau_sweep(torch.zeros(0)) == {}
    assert list(spectral_neg_tau_sweep(nsd, min_w, taus=(3.0,))) == [3.0]


def test_c_abi_argument_errors_need_no_device():
    """frl_spectral_negatives and frl_pair_sims report argument errors before any HIP call, and empty calls are no-ops: none of these
    calls touches a device (there is none here)."""
    import ctypes
    from frl_hip import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def neg(c=4, s=2, n_per=3, q=6, tau=1.0, spec=p, offsets=p, draws=p, pairs=p, dist=p, weights=p, n=10):
        return lib.frl_spectral_negatives(spec, n, c, offsets, s, n_per, draws, q, tau, 0.05, pairs, dist, weights, None, None)

    def sims(d=4, t=5, n=10, emb=p, pairs=p, out=p, stats=None, ws=None, ws_bytes=0):
        return lib.frl_pair_sims(emb, n, d, pairs, t, out, stats, None, ws, ws_bytes, None)

    assert neg(q=0, s=1, n_per=0) == 0 and neg(q=0, spec=None, offsets=None, draws=None, pairs=None, dist=None, weights=None) == 0
    for kw in (dict(c=0), dict(c=257), dict(s=1), dict(s=1, q=3), dict(q=7), dict(n_per=0), dict(q=-1), dict(tau=0.0), dict(n=0),
               dict(spec=None), dict(offsets=None), dict(draws=None), dict(pairs=None), dict(dist=None), dict(weights=None)):
        assert neg(**kw) < 0, kw
        assert lib.frl_last_error()
    assert sims(t=0, emb=None, pairs=None, out=None) == 0
    for kw in (dict(d=0), dict(d=257), dict(t=-1), dict(n=0), dict(emb=None), dict(pairs=None), dict(out=None), dict(stats=p), dict(stats=p, ws=p, ws_bytes=8)):
        assert sims(**kw) < 0, kw
    assert lib.frl_pair_sims_workspace_bytes(0) == 0
    assert lib.frl_pair_sims_workspace_bytes(1) == 16 and lib.frl_pair_sims_workspace_bytes(17) == 32
    assert lib.frl_pair_sims_workspace_bytes(10 ** 9) == lib.frl_pair_sims_workspace_bytes(10 ** 7)      # the grid is capped


def test_argument_errors_come_before_the_library(monkeypatch):
    """Every ValueError of the public functions is raised on CPU tensors, before libfrlhip is loaded or a GPU is asked for."""
    from frl_hip import _lib

    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")

    monkeypatch.setattr(_lib, "load", no_library)
    spec = torch.randn(12, 5)
    ok = [0, 4, 12]
    with pytest.raises(ValueError, match="start at 0"):
        cross_patch_negatives(spec, [1, 4, 12])
    with pytest.raises(ValueError, match="end at"):
        cross_patch_negatives(spec, [0, 4, 11])
    with pytest.raises(ValueError, match="decrease"):
        cross_patch_negatives(spec, [0, 8, 4, 12])
    with pytest.raises(ValueError, match="at least one anchor"):
        cross_patch_negatives(spec, [0, 4, 4, 12])
    with pytest.raises(ValueError, match="at least one anchor"):
        cross_patch_negatives(spec, torch.tensor([0, 0, 12]))
    with pytest.raises(ValueError, match="channels"):
        cross_patch_negatives(torch.randn(12, 257), ok)
    with pytest.raises(ValueError, match="tau"):
        cross_patch_negatives(spec, ok, tau=0.0)
    n_per = negatives_per_patch_pair(20, 12, 2)
    q = 2 * n_per
    with pytest.raises(ValueError, match="draws must be"):
        cross_patch_negatives(spec, ok, draws=torch.zeros(q, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="draws must be"):
        cross_patch_negatives(spec, ok, draws=torch.zeros(q + 1, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="draws must be"):
        cross_patch_negatives(spec, ok, draws=torch.zeros(q, 2, dtype=torch.float32))
    for bad in (-1, 2 ** 31):
        draws = torch.zeros(q, 2, dtype=torch.int64)
        draws[3, 1] = bad
        with pytest.raises(ValueError, match=r"\[0, 2\^31\)"):
            cross_patch_negatives(spec, ok, draws=draws)
    z = torch.randn(12, 8)
    coords = [torch.zeros(4, 2, dtype=torch.long), torch.zeros(8, 2, dtype=torch.long)]
    with pytest.raises(ValueError, match="at least one anchor"):
        global_spectral_infonce(z, spec, coords, [0, 12, 12])
    with pytest.raises(ValueError, match="entries"):
        global_spectral_infonce(z, spec, coords, [0, 4, 8, 12])
    with pytest.raises(ValueError):
        global_spectral_infonce(z, spec[:11], coords, ok)
    with pytest.raises(ValueError):
        pair_similarity(z, torch.zeros(3, 3, dtype=torch.long))
    # valid arguments on CPU tensors: no fallback, and still no library
    for call in (lambda: cross_patch_negatives(spec, ok), lambda: pair_similarity(z, torch.zeros(3, 2, dtype=torch.long)),
                 lambda: pair_similarity_stats(z, torch.zeros(3, 2, dtype=torch.long), torch.zeros(3, 2, dtype=torch.long), 0.07)):
        with pytest.raises(_lib.FrlHipError):
            call()
    # the empty ends need neither
    empty = torch.zeros(0, 2, dtype=torch.long)
    assert pair_similarity_stats(z, empty, torch.zeros(3, 2, dtype=torch.long), 0.07) is None
    assert pair_similarity_stats(z, torch.zeros(3, 2, dtype=torch.long), empty, 0.07) is None
    loss, info = global_spectral_infonce(torch.zeros(0, 8), torch.zeros(0, 5), [], [0])
    assert loss.dim() == 0 and loss.item() == 0.0 and info["n_pos"] == 0 and info["n_neg"] == 0 and info["sim_stats"] is None
    assert info["pos_pairs"].shape == (0, 2) and info["neg_pairs"].shape == (0, 2) and info["neg_weights"].shape == (0,)
