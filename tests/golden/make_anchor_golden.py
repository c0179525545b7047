"""Writes tests/golden/anchor_grid.npz, anchor_supplement.npz and anchor_weights.npz by running the REFERENCE's
frl/data/sampling/anchor_sampling.py, loaded by path.  The reference does not travel; only these arrays do.  Inputs come from the seeded
makers of tests/anchor_cases.py: a 24 x 20 mask with a hole ("small") and a 70 x 67 mask ("large").

anchor_grid: per case c and seed s, jitter_c_s [2] (the two randint draws of sample_anchors_grid, row first, recorded by re-seeding and
repeating them) and grid_c_s [G, 2], for the (mask, stride, border, jitter_radius, seeds) of anchor_cases.GRID_CASES.  The maker asserts
that the seeds reach -radius and +radius on both axes, that one case has a grid row at exactly H - border - 1, that the 70 x 67 case has
4158 points, that the (16, 10) case on 24 x 20 is empty and that the reference itself raises for (16, 16) there (torch.arange
refuses a start beyond its end), so that case has no fixture.
anchor_supplement: torch's randperm / multinomial streams cannot be matched, so candidate sets are pinned (the grid
points, which come first and are checked against sample_anchors_grid, are stripped).  all_<mask>: the reference called with
supplement_n above the number of valid pixels returns every valid pixel.  positive_<mask>: called with weights and supplement_n = the number of valid pixels of positive weight it
returns exactly those (a negative weight is clamped out).  zero_<mask>: with all-zero weights it returns supplement_n uniform picks.
Keys are row * W + col, sorted (zero_*: in the reference's order).
anchor_weights: invfreq_<case> = _apply_inverse_frequency and resolve_<case> = resolve_supplement_weights on the cases of
anchor_cases.invfreq_cases / RESOLVE_CASES, bit for bit.  The maker asserts that -0.0 and 0.0 share one count.

    FRL_REFERENCE=<checkout of the reference> python tests/golden/make_anchor_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
_spec = importlib.util.spec_from_file_location(
    "reference_anchor_sampling", os.path.join(os.environ["FRL_REFERENCE"], "frl", "data", "sampling", "anchor_sampling.py"))
REF = importlib.util.module_from_spec(_spec)
sys.modules["reference_anchor_sampling"] = REF                      # dataclasses look the module up while it is being executed
_spec.loader.exec_module(REF)

import anchor_cases as AC  # noqa: E402


def save(name, arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    print(name, os.path.getsize(path), "bytes")


def main():
    masks = AC.fixture_masks()
    weights = AC.fixture_weights()

    grid = {f"mask_{k}": v for k, v in masks.items()}
    last_row = False
    for c, (name, stride, border, radius, seeds) in enumerate(AC.GRID_CASES):
        mask_t = torch.from_numpy(masks[name])
        h, w = masks[name].shape
        seen = set()
        for seed in seeds:
            jr = jc = 0
            if radius > 0:
                torch.manual_seed(seed)
                jr = torch.randint(-radius, radius + 1, (1,)).item()
                jc = torch.randint(-radius, radius + 1, (1,)).item()
            torch.manual_seed(seed)
            out = REF.sample_anchors_grid(mask_t, stride=stride, border=border, jitter_radius=radius).numpy()
            seen |= {("r", jr), ("c", jc)}
            rows = range(border + jr, h - border, stride)
            last_row |= len(rows) > 0 and rows[-1] == h - border - 1 and bool((out[:, 0] == h - border - 1).any())
            grid[f"jitter_{c}_{seed}"] = np.asarray([jr, jc], dtype=np.int32)
            grid[f"grid_{c}_{seed}"] = out.astype(np.int32)
        if radius > 0:
            assert {("r", -radius), ("r", radius), ("c", -radius), ("c", radius)} <= seen, f"case {c}: the seeds miss an extreme jitter: {seen}"
        print(f"anchor_grid case {c} ({name}, {stride}, {border}, {radius}): {[len(grid[f'grid_{c}_{s}']) for s in seeds]} points")
    assert last_row, "no case has a grid row at exactly H - border - 1"
    assert len(grid["grid_2_0"]) == int(masks["large"][2:68, 2:65].sum()) and 66 * 63 == 4158
    assert len(grid["grid_3_0"]) == 0
    name, stride, border, radius = AC.RAISING_GRID
    try:
        REF.sample_anchors_grid(torch.from_numpy(masks[name]), stride=stride, border=border, jitter_radius=radius)
        raise AssertionError("the reference no longer raises for a grid origin beyond H - border")
    except RuntimeError:
        pass
    save("anchor_grid.npz", grid)

    sup = {}
    for name, mask in masks.items():
        mask_t = torch.from_numpy(mask)
        h, w = mask.shape
        kw = AC.SUPPLEMENT_GRID[name]
        g = REF.sample_anchors_grid(mask_t, **kw).numpy()

        def strip(rows):
            assert np.array_equal(rows[:len(g)], g)
            return rows[len(g):]
        n_valid = int(mask.sum())
        torch.manual_seed(1)
        out = strip(REF.sample_anchors_grid_plus_supplement(mask_t, supplement_n=n_valid + 5, **kw).numpy())
        assert len(out) == n_valid
        sup[f"all_{name}"] = np.sort(AC.keys_of(out, w)).astype(np.int32)
        assert np.array_equal(sup[f"all_{name}"], np.nonzero(mask.reshape(-1))[0])
        wgt = weights[name]
        positive = mask & (wgt > 0)
        assert (wgt[mask] < 0).any() and (wgt[mask] == 0).any()
        torch.manual_seed(2)
        out = strip(REF.sample_anchors_grid_plus_supplement(mask_t, supplement_n=int(positive.sum()), weights=torch.from_numpy(wgt), **kw).numpy())
        sup[f"weights_{name}"] = wgt
        sup[f"positive_{name}"] = np.sort(AC.keys_of(out, w)).astype(np.int32)
        assert np.array_equal(sup[f"positive_{name}"], np.nonzero(positive.reshape(-1))[0]), "the reference left the positive-weight pixels"
        torch.manual_seed(3)
        out = strip(REF.sample_anchors_grid_plus_supplement(mask_t, supplement_n=10, weights=torch.zeros(h, w), **kw).numpy())
        assert len(out) == 10 and len(set(AC.keys_of(out, w).tolist())) == 10 and mask[out[:, 0], out[:, 1]].all()
        sup[f"zero_{name}"] = AC.keys_of(out, w).astype(np.int32)
        print(f"anchor_supplement {name}: {n_valid} valid, {int(positive.sum())} of positive weight")
    save("anchor_supplement.npz", sup)

    wts = {}
    for name, (data, valid, listed) in AC.invfreq_cases().items():
        out = REF._apply_inverse_frequency(torch.from_numpy(data), torch.from_numpy(valid), valid_values=listed).numpy()
        assert out.dtype == np.float32
        wts[f"invfreq_{name}"] = out
        print(f"anchor_weights invfreq {name}: {len(np.unique(out))} distinct weights, {int((out > 0).sum())} positive")
    codes, valid, _ = AC.invfreq_cases()["codes"]
    zeros = valid & (codes == 0)
    assert np.signbit(codes[zeros]).any() and not np.signbit(codes[zeros]).all()
    assert len(np.unique(wts["invfreq_codes"][zeros])) == 1 and wts["invfreq_codes"][zeros][0] == np.float32(1) / np.float32(zeros.sum())
    many, large, _ = AC.invfreq_cases()["many"]
    assert len(np.unique(many[large & np.isfinite(many)])) > 550
    assert np.array_equal(wts["invfreq_nothing_listed"], valid.astype(np.float32))
    sample = AC.resolve_sample()
    for name, specs in AC.RESOLVE_CASES.items():
        ref_specs = [REF.WeightSpec(channel=ch, transform=tr, valid_values=vv) for ch, tr, vv in specs]
        wts[f"resolve_{name}"] = REF.resolve_supplement_weights(sample, ref_specs).numpy()
        print(f"anchor_weights resolve {name}: {int((wts[f'resolve_{name}'] > 0).sum())} positive")
    save("anchor_weights.npz", wts)


if __name__ == "__main__":
    main()
