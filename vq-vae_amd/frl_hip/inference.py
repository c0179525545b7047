"""Store-level inference: a whole TileStore raster -> VQ code maps.

`encode_store` walks every `tile x tile` patch of the store through the training input pipeline (ChunkTileDataset + TilePrefetcher:
the same normalisation, masking and compute dtype), batched chunk by chunk, encodes each batch with `VQVAE.encode_tiles` and places
each tile's codes at its spatial window.  Tiles are encoded independently, exactly as in training: a pixel near a tile border sees
the encoder's zero padding there (the spatial convolutions do not look across tiles), so its code can differ from the one it would
get inside a larger window.  Overlapping-window inference is not done here.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch


def place_tiles(raster: np.ndarray, windows: Sequence[Tuple[int, int, int, int]], values) -> np.ndarray:
    """Writes values[i] (`[..., tile, tile]`, leading axes matching raster's) into raster[..., r:r+h, c:c+w] for windows[i] =
    (row, col, h, w), cropping the tile to its (h, w) valid part (partial tiles at the raster edge).  Returns `raster`."""
    for win, v in zip(windows, values):
        r, c, h, w = (int(x) for x in win)
        raster[..., r:r + h, c:c + w] = np.asarray(v)[..., :h, :w]
    return raster


@torch.no_grad()
def encode_store(model, store, tile: int = 32, batch_size: int = 256, device="cuda", out: Optional[str] = None,
                 workers: int = 8) -> Dict:
    """model (VQVAE), store (TileStore) -> dict(codes int32 [Y,X], valid uint8 [Y,X], [codes_phase int32 [T,Y,X]], counts int64 [K],
    meta).  Every raster pixel is written exactly once; `valid` is 1 where the pixel has an observation at every time step (the
    type-loss rule).  `counts` is the code histogram over the valid pixels.  With `out`, the arrays are also written to `out` (.npz,
    suffix added when missing) and the meta to the same path with a .json suffix."""
    from .data.tile_loader import ChunkTileDataset, TilePrefetcher

    ds = ChunkTileDataset(store, tile=tile)
    ny, nx = store.shape[1], store.shape[2]
    nt = store.shape[0]
    has_phase = hasattr(model, "quant_phase")
    k = model.quant.codebook_size
    codes = np.full((ny, nx), -1, dtype=np.int32)
    valid = np.zeros((ny, nx), dtype=np.uint8)
    codes_phase = np.full((nt, ny, nx), -1, dtype=np.int32) if has_phase else None
    batches = []
    for members in ds.xy_by_chunk:                               # chunk by chunk: the prefetcher's whole-chunk upload path applies
        for i in range(0, len(members), batch_size):
            batches.append([int(j) for j in members[i:i + batch_size]])
    pf = TilePrefetcher(ds, batches, device=device, out_dtype=model.compute_dtype, max_batch=batch_size, workers=workers)
    for batch in pf:
        enc = model.encode_tiles(batch["tile"], batch["mask"])
        wins = [ds.spatial_window(i) for i in batch["indices"]]
        place_tiles(codes, wins, enc["idx"].cpu().numpy())
        place_tiles(valid, wins, enc["valid"].to(torch.uint8).cpu().numpy())
        if has_phase:
            place_tiles(codes_phase, wins, enc["idx_phase"].cpu().numpy())
    counts = np.bincount(codes[valid.astype(bool)].astype(np.int64), minlength=k).astype(np.int64)
    meta = dict(shape=list(store.shape), tile=int(tile), codebook_size=int(k),
                phase_codebook_size=int(model.quant_phase.codebook_size) if has_phase else 0,
                compute_dtype=str(model.compute_dtype).replace("torch.", ""), features=list(store.meta.get("features", [])))
    res = dict(codes=codes, valid=valid, counts=counts, meta=meta)
    if has_phase:
        res["codes_phase"] = codes_phase
    if out is not None:
        path = out if out.endswith(".npz") else out + ".npz"
        arrays = {k_: v for k_, v in res.items() if k_ != "meta"}
        np.savez(path, **arrays)
        with open(path[:-4] + ".json", "w") as fh:
            json.dump(meta, fh, indent=1)
        res["path"] = path
    return res
