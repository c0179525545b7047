from .anchor_sampling import (AnchorSampler, WeightSpec, build_anchor_sampler, inverse_frequency_weights,  # noqa: F401
                              resolve_supplement_weights, sample_anchors_batched, sample_anchors_grid,
                              sample_anchors_grid_plus_supplement)
from .forest_dataset import ForestDataset, SyntheticTileStream, collate_fn  # noqa: F401
from .normalization import NormPreset, norm_table  # noqa: F401
from .samplers import ChunkBatchSampler, shard_batches  # noqa: F401
from .tile_loader import ChunkTileDataset, TilePrefetcher  # noqa: F401
from .tile_store import TileStore, write_tile_store  # noqa: F401
