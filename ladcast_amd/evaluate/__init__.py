from .utils import (ensemble_scores, get_acc, get_crps, get_lat_weights_from_lat_tensor, get_normalized_lat_weights_based_on_cos,
                    pointwise_crps_skill, pointwise_crps_spread, rollout_scores)

_DRIVER_NAMES = ("climatology_slots", "score_latent_rollout", "truth_frame_slots")  # evaluate_ens_gpu's, resolved at first use: the
__all__ = ["ensemble_scores", "get_acc", "get_crps", "get_lat_weights_from_lat_tensor", "get_normalized_lat_weights_based_on_cos",  # module
           "pointwise_crps_skill", "pointwise_crps_spread", "rollout_scores", *_DRIVER_NAMES]  # also runs as `python -m`


def __getattr__(name):
    if name in _DRIVER_NAMES:
        from . import evaluate_ens_gpu

        return getattr(evaluate_ens_gpu, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
