"""Seeded inputs and the case list of the denoising-loss fixture (tests/golden/denoise_loss_ref.npz), shared by its generator
(tests/golden/make_denoise_loss_golden.py) and the tests: the fixture holds results only.

B = 2 samples of the tiny AR model: 84 channels, one input frame, T = 2 target frames on the 15 x 30 latent grid.  The second sample's
timestamp sits 3 h before a new year, so the +6 h of a push-forward step crosses it."""
import itertools

import torch

from tests.synth import synth_known

B, C, T_IN, T, H, W = 2, 84, 1, 2, 15, 30
TIMESTAMPS = (2018010100, 2018123121)
CLEAN_SEED, NOISE_SEED = 11, 12
INDEX_SETS = {"ends": (0, 999), "mid": (500, 500)}  # both ends of the 1000-entry training schedule; one level for the whole batch
PUSH_FORWARD = (1, 2)
PREDICTION_TYPES = ("epsilon", "v_prediction")
SAMPLER_SEED, SAMPLER_BATCH, SAMPLER_STEPS = 7, 16, (0, 30000)  # Karras_sigmas_lognormal: generator seed, batch, the two `cur_step`s
SUB_STRIDE = 97  # noisy_images / x_in / the model_pred of most cases are kept as every 97th value (tests/synth.py::Sub)


def initial_profile():
    return synth_known(B, T_IN, seed=2)


def clean_images():
    return 0.5 * torch.randn(B, C, T, H, W, generator=torch.Generator().manual_seed(CLEAN_SEED))


def noise():
    """what `torch.manual_seed(NOISE_SEED); torch.randn(shape)` draws (the reference draws from the global generator)"""
    return torch.randn(B, C, T, H, W, generator=torch.Generator().manual_seed(NOISE_SEED))


def timestamps():
    return torch.tensor(TIMESTAMPS, dtype=torch.int64)


def cases():
    """(key, index set name, num_push_forward_steps, lat_weighted_loss, prediction_type) of every fixture case"""
    out = []
    for name, k, lat, pred in itertools.product(INDEX_SETS, PUSH_FORWARD, (False, True), PREDICTION_TYPES):
        out.append((f"{name}_k{k}_lat{int(lat)}_{pred}", name, k, lat, pred))
    return out


def model_pred_key(name, k, pred):
    """model_pred does not depend on the latitude weighting, nor - without push-forward - on the prediction type"""
    return f"model_pred_{name}_k{k}" + ("" if k == 1 else f"_{pred}")
