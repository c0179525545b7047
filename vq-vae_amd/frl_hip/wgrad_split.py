"""The workgroup split of the merged 3x3 weight-gradient launch, mirrored from csrc/conv3x3_wgrad.hip (c3v_multi_supported,
c3v_multi_split) in plain Python: what the tests and tools reason with.  A function of the shapes alone.

Every job of a merged call is a bf16 3x3 weight gradient over images of one shape (B, H, W) cut into 8 x 32-pixel bands (tiles); a work
item is (one tile, 64 input channels).  The split keeps every reduced gradient bit for bit the single call's.  With a budget of 256
workgroups:
  * the jobs' tiles together fit the budget: every workgroup owns one tile (all chunks of it) and writes one slab, as in the single call;
  * tiles >= 256: the single call runs 256 workgroups of tpw = ceil(tiles / 256) consecutive tiles (a unit) and its fixed-order reduction
    adds the 256 slabs in chains k, k + 64, k + 128, k + 192.  The merged call gives every (job, 64-channel chunk) 64 workgroups;
    workgroup k runs the four units of chain k one after the other, each accumulated from zero, and adds them up in slab k in that order:
    64 slabs per job, 4 * tpw items per workgroup whatever the job's Cin;
  * anything else (fewer than 256 tiles that do not fit together, more than 8 chunks in all) runs job by job.
"""
from typing import Dict, List, Optional, Sequence

BAND_TH, BAND_TW, BAND_C = 8, 32, 64
BUDGET = 256
CHAIN = 4
MAX_JOBS = 4
MAX_ENTRIES = 8


def tiles_of(B: int, H: int, W: int) -> int:
    return B * (H // BAND_TH) * (W // BAND_TW)


def eligible(B: int, H: int, W: int, cin: Sequence[int], cout: Sequence[int]) -> bool:
    """The shape part of c3v_multi_supported (the dtype is bf16)."""
    if not (1 <= len(cin) <= MAX_JOBS and len(cin) == len(cout) and B > 0 and H > 0 and W > 0 and H % BAND_TH == 0 and W % BAND_TW == 0
            and all(c > 0 and c % BAND_C == 0 for c in cin) and all(c == BAND_C for c in cout)):
        return False
    tiles = tiles_of(B, H, W)
    return tiles * len(cin) <= BUDGET or (tiles >= BUDGET and sum(c // BAND_C for c in cin) <= MAX_ENTRIES)


def split(B: int, H: int, W: int, cin: Sequence[int]) -> Optional[List[Dict[str, int]]]:
    """-> per job: first_wg, nwg (workgroups), nslab, tpw (tiles of a unit), nunits (units a workgroup chains), items (work items of the
    busiest workgroup), tiles; None where the merged launch does not apply."""
    if not eligible(B, H, W, cin, [BAND_C] * len(cin)):
        return None
    tiles = tiles_of(B, H, W)
    out, grid = [], 0
    for c in cin:
        if tiles * len(cin) <= BUDGET:
            j = dict(first_wg=grid, nwg=tiles, nslab=tiles, tpw=1, nunits=1, items=c // BAND_C, tiles=tiles)
        else:
            tpw = -(-tiles // BUDGET)
            j = dict(first_wg=grid, nwg=(BUDGET // CHAIN) * (c // BAND_C), nslab=BUDGET // CHAIN, tpw=tpw, nunits=CHAIN, items=CHAIN * tpw, tiles=tiles)
        out.append(j)
        grid += j["nwg"]
    return out


def slab_floats(cin: int) -> int:
    """float32 values of one slab: [9 taps][64 output channels][Cin] | [64] bias."""
    return 64 * cin * 9 + 64


def workspace_bytes(B: int, H: int, W: int, cin: Sequence[int]) -> int:
    return sum(4 * j["nslab"] * slab_floats(c) for j, c in zip(split(B, H, W, cin), cin))
