"""Dataset preparation on the device: the per-variable statistics of the raw fields, the bulk encode into the latent store, the latent
statistics and the day-of-year climatology - the inputs every inference and evaluation entry point starts from.

Reference: ``ladcast/preprocecss/`` (the reference's directory name carries that typo; this package spells it ``preprocess``):
``compute_mean_std_era5.py`` and ``encode_data.py``.  The latent statistics JSON is shipped by the reference without the code that made it,
and the climatology is read by the reference from a ready-made zarr store (``climatology`` / ``compute_climatology`` build it here).
"""
from .climatology import Climatology, frame_slots, slot_of, window_weights
from .stats import FieldMoments, latent_normal_dict, normalization_dict

__all__ = ["Climatology", "FieldMoments", "frame_slots", "latent_normal_dict", "normalization_dict", "slot_of", "window_weights"]
