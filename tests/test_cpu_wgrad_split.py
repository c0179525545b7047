"""The workgroup split of the merged 3x3 weight-gradient launch (frl_hip/wgrad_split.py, the Python mirror of c3v_multi_split in
csrc/conv3x3_wgrad.hip): the figures of the benchmark shape, one tile per workgroup whenever the tiles fit, the invariants the kernel
relies on, and the reason the split keeps the single call's bits: the chains of the fixed-order slab reduction."""
import os

import pytest

from frl_hip import wgrad_split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_benchmark_shape_gives_64_64_128_workgroups_of_16_items():
    sp = S.split(256, 32, 32, [64, 64, 128])
    assert [j["nwg"] for j in sp] == [64, 64, 128] and [j["first_wg"] for j in sp] == [0, 64, 128]
    assert [j["items"] for j in sp] == [16, 16, 16] and all(j["tpw"] == 4 and j["nunits"] == 4 for j in sp)
    assert all(j["tiles"] == 1024 and j["nslab"] == 64 for j in sp)
    # 64 slabs per job instead of 256 per call: 38 MB instead of 151 MB
    assert S.workspace_bytes(256, 32, 32, [64, 64, 128]) == 4 * 64 * (2 * S.slab_floats(64) + S.slab_floats(128))
    assert 37e6 < S.workspace_bytes(256, 32, 32, [64, 64, 128]) < 38e6


@pytest.mark.parametrize("B,H,W,cin", [(2, 32, 32, [64, 64, 128]), (1, 8, 32, [64, 64, 128]), (2, 24, 96, [64, 64, 128]), (64, 8, 32, [64, 128, 64, 64]),
                                        (85, 8, 32, [64, 64, 128]), (256, 8, 32, [128]), (1, 8, 32, [64])])
def test_one_tile_per_workgroup_whenever_the_tiles_fit(B, H, W, cin):
    tiles = B * (H // 8) * (W // 32)
    assert tiles * len(cin) <= S.BUDGET
    sp = S.split(B, H, W, cin)
    assert all(j["tpw"] == 1 and j["nunits"] == 1 and j["nwg"] == tiles and j["nslab"] == tiles for j in sp)
    assert [j["first_wg"] for j in sp] == [k * tiles for k in range(len(cin))]


@pytest.mark.parametrize("B,H,W,cin,want", [
    (100, 24, 32, [64, 64, 128], [(64, 2), (64, 2), (128, 2)]),      # 300 tiles: units of 2 tiles, 150 busy units, chains of 3 or 2 busy units
    (256, 32, 32, [64, 64], [(64, 4), (64, 4)]),
    (300, 8, 32, [64], [(64, 2)]),
    (100, 24, 32, [64, 256], [(64, 2), (256, 2)]),
])
def test_chained_units(B, H, W, cin, want):
    sp = S.split(B, H, W, cin)
    assert [(j["nwg"], j["tpw"]) for j in sp] == want and all(j["nunits"] == 4 and j["nslab"] == 64 for j in sp)


def test_shapes_the_merged_launch_leaves_alone():
    assert S.split(86, 8, 32, [64, 64, 128]) is None                 # 86 tiles: three jobs do not fit, and the single call has no 256 slabs
    assert S.split(100, 24, 32, [64, 512, 64]) is None               # 10 chunks
    assert S.split(2, 32, 16, [64, 64]) is None


@pytest.mark.parametrize("tiles", [256, 257, 300, 511, 512, 513, 1024, 4097])
def test_chains_are_the_chains_of_the_slab_reduction(tiles):
    """frl_reduce.hpp at 256 slabs: thread group g adds, per partial sum m, the slabs g + 8m + 64t for t = 0..3 in that order, then combines
    the 8 x 8 partial sums in a fixed tree.  At 64 slabs the same tree takes ONE slab per partial sum, g + 8m.  So slab k of the merged call
    must be ((unit k + unit k + 64) + unit k + 128) + unit k + 192, with the single call's units; idle units are zero slabs there."""
    def reduction_chains(nslab):
        chains = {}
        for g in range(8):
            k = g
            while k + 56 < nslab:
                for m in range(8):
                    chains.setdefault((g, m), []).append(k + 8 * m)
                k += 64
            assert k >= nslab                                        # (no remainder loop at 64 or 256 slabs)
        return chains
    single, merged = reduction_chains(256), reduction_chains(64)
    assert single.keys() == merged.keys()
    j = S.split(tiles, 8, 32, [64, 128])[1]
    tpw, busy = j["tpw"], -(-tiles // j["tpw"])
    assert tpw == -(-tiles // 256) and busy <= 256
    covered = []
    for key, (k,) in ((key, v) for key, v in merged.items()):
        units = [k + 64 * t for t in range(j["nunits"])]
        assert units == single[key]
        covered += [u for u in units if u < busy]
    assert sorted(covered) == list(range(busy)) and all(k < busy for k in range(64))   # every busy unit once; no workgroup without a tile


def test_eligibility():
    assert S.eligible(256, 32, 32, [64, 64, 128], [64, 64, 64])
    assert not S.eligible(2, 32, 32, [64, 64], [64, 128])             # a single output slice per job
    assert not S.eligible(2, 32, 16, [64, 64], [64, 64]) and not S.eligible(2, 12, 32, [64, 64], [64, 64])
    assert not S.eligible(2, 32, 32, [64, 96], [64, 64]) and not S.eligible(2, 32, 32, [64] * 5, [64] * 5)
    assert not S.eligible(2, 32, 32, [], [])


def test_mirror_names_the_constants_of_the_source():
    src = open(os.path.join(ROOT, "vq-vae_amd", "csrc", "conv3x3_wgrad.hip"), encoding="utf-8").read()
    assert f"#define C3V_BUDGET {S.BUDGET}" in src and f"#define C3V_MAX_JOBS {S.MAX_JOBS}" in src
    assert f"#define C3V_CHAIN {S.CHAIN}" in src and f"#define C3V_MAX_ENTRIES {S.MAX_ENTRIES}" in src
    assert f"#define C3V_TH {S.BAND_TH}" in src and f"#define C3V_TW {S.BAND_TW}" in src
    assert "return tiles * njobs <= C3V_BUDGET || (tiles >= C3V_BUDGET && chunks <= C3V_MAX_ENTRIES);" in src
    red = open(os.path.join(ROOT, "vq-vae_amd", "csrc", "frl_reduce.hpp"), encoding="utf-8").read()
    assert "for (; k + 56 < nslab; k += 64) {" in red and "s3 += slab[(int64_t)(k + 24) * n + i];" in red
