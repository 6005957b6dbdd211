from .utils import (EVENT_SCORE_NAMES, FSS_SCORE_NAMES, VALIDATION_SCORE_NAMES, Event, empty_events, empty_fss, empty_products, event_scores, fss_scores, rollout_events, rollout_fss, ensemble_scores, get_acc, get_crps, get_lat_weights_from_lat_tensor,
                    get_normalized_lat_weights_based_on_cos, pointwise_crps_skill, pointwise_crps_spread, rollout_products, rollout_reliability, rollout_scores, rollout_spectrum,
                    validation_scores)
from .regional import NAMED_REGIONS, REGIONAL_SCORE_NAMES, Region, empty_regional, region_mask, regional_scores, rollout_regional

_DRIVER_NAMES = ("climatology_slots", "score_latent_rollout", "truth_frame_slots")  # evaluate_ens_gpu's, resolved at first use: the
_VALIDATE_NAMES = ("NpyLatentStore", "log_validation", "validate_initial_time")  # validate_AR's, likewise
_DENOISE_NAMES = ("denoising_loss", "evaluate_denoising_loss", "push_forward_plan")  # denoise_loss's, likewise
_PRODUCTS_NAMES = ("products_of_latent_rollout",)  # products', likewise
_ENERGY_NAMES = ("ENERGY_NAMES", "EnergyGroup", "empty_energy", "rollout_energy")  # energy's, likewise
_DERIVED_NAMES = ("Derived", "SPHERE_KINDS", "derive_forecast", "derive_table", "derived_metadata", "parse_derived", "sphere_row_tables")  # derived's, likewise
__all__ = ["VALIDATION_SCORE_NAMES", "ensemble_scores", "get_acc", "get_crps", "get_lat_weights_from_lat_tensor",  # module
           "get_normalized_lat_weights_based_on_cos", "pointwise_crps_skill", "pointwise_crps_spread", "rollout_reliability", "rollout_scores", "rollout_spectrum",  # also runs
           "validation_scores", "empty_products", "rollout_products", "EVENT_SCORE_NAMES", "Event", "empty_events", "event_scores", "rollout_events", "FSS_SCORE_NAMES", "empty_fss", "fss_scores", "rollout_fss", "NAMED_REGIONS", "REGIONAL_SCORE_NAMES",
           "Region", "empty_regional", "region_mask", "regional_scores", "rollout_regional", *_DRIVER_NAMES, *_VALIDATE_NAMES, *_DENOISE_NAMES, *_PRODUCTS_NAMES, *_ENERGY_NAMES, *_DERIVED_NAMES]  # as `python -m`


def __getattr__(name):
    if name in _DRIVER_NAMES:
        from . import evaluate_ens_gpu

        return getattr(evaluate_ens_gpu, name)
    if name in _VALIDATE_NAMES:
        from . import validate_AR

        return getattr(validate_AR, name)
    if name in _DENOISE_NAMES:
        from . import denoise_loss

        return getattr(denoise_loss, name)
    if name in _PRODUCTS_NAMES:
        from . import products

        return getattr(products, name)
    if name in _ENERGY_NAMES:
        from . import energy

        return getattr(energy, name)
    if name in _DERIVED_NAMES:
        from . import derived

        return getattr(derived, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
