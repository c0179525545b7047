from .spatial import (extract_at_locations, extract_temporal_at_locations, spatial_knn_pairs,  # noqa: F401
                      spatial_negative_pairs)
