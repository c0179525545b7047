from .pairs import pairs_mutual_knn_chunked  # noqa: F401
from .contrastive import contrastive_loss  # noqa: F401
from .variance_covariance import variance_covariance_loss, variance_loss, covariance_loss  # noqa: F401
from .soft_neighborhood import (soft_neighborhood_matching_loss, soft_neighborhood_loss_gathered, phase_alignment,  # noqa: F401
                                phase_neighborhood_loss)
from .evt_soft_neighborhood import EvtDiffusionMetric, evt_soft_neighborhood_loss, evt_soft_neighborhood_loss_batched  # noqa: F401
from .phase_margin import (phase_recovery_discrimination_loss, compute_phase_spread_ranking, phase_spread_ranking_gathered,  # noqa: F401
                           phase_spread_ranking_loss)
from .phase_pairs import build_phase_pairs, build_phase_pairs_batched  # noqa: F401
from .spatial_pairs import build_spatial_pairs, build_spatial_pairs_batched  # noqa: F401
from .spectral_infonce import (cross_patch_negatives, pair_similarity, pair_similarity_stats, spectral_neg_tau_sweep,  # noqa: F401
                               global_spectral_infonce)
from .type_baseline import type_local_baseline, type_projection  # noqa: F401
from .leakage import phase_type_leakage_loss  # noqa: F401
