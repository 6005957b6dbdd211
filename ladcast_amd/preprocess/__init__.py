"""Dataset preparation on the device: the per-variable statistics of the raw fields, the bulk encode into the latent store and the latent
statistics - the three inputs every inference and evaluation entry point starts from.

Reference: ``ladcast/preprocecss/`` (the reference's directory name carries that typo; this package spells it ``preprocess``):
``compute_mean_std_era5.py`` and ``encode_data.py``.  The latent statistics JSON is shipped by the reference without the code that made it.
"""
from .stats import FieldMoments, latent_normal_dict, normalization_dict

__all__ = ["FieldMoments", "latent_normal_dict", "normalization_dict"]
