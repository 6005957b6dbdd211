"""Seeded stand-ins shared by tests/golden/make_validation_golden.py (which runs the reference's `log_validation` on them, on the CPU) and
the validation tests (which run `ladcast_amd.evaluate.log_validation` on them, on the device): a latent store, a chunk sampler and a decoder
made of single IEEE-exact elementwise operations (no matrix product, no transcendental, no reduction), in the spirit of
tests/synth.py::ToyNet - the same bits come out on any CPU and on the GPU, so the fixture pins the driver's structure (which frames, which
timestamps, which chain feeds which chunk) and the scores' definitions, not a kernel's rounding.

Shapes: the reference hard-wires 84 channels on a 120 x 240 grid, so C = 84 and the latent grid is 15 x 30 (decoder: x 8)."""
from datetime import datetime, timedelta
from types import SimpleNamespace

import torch

C, LAT_H, LAT_W, SCALE = 84, 15, 30, 8
N_FRAMES, START, STEP_HOURS = 10, datetime(2018, 1, 1, 0), 6
INIT_TIMES = (START + timedelta(hours=2 * STEP_HOURS), START + timedelta(hours=5 * STEP_HOURS))
ENS, T, R, T_IN, INFERENCE_STEPS = 3, 4, 2, 1, 5
CHANNEL_NAMES = ["z", "q", "t", "u", "v", "w", "u10", "v10", "t2m", "msl", "sst", "tp"]  # 6 x 13 levels + 6 = 84 columns


def latent_frames():
    """(N_FRAMES, C, 15, 30) fp32, torch CPU generator: the same numbers on every machine"""
    return 0.5 * torch.randn(N_FRAMES, C, LAT_H, LAT_W, generator=torch.Generator().manual_seed(11))


def field_statistics():
    g = torch.Generator().manual_seed(12)
    return torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5


def latent_transform(x):
    return x * 2.0 - 0.125


def latent_inv_transform(x):
    return (x + 0.125) * 0.5


class RecordingSampler:
    """`ensemble_AR_sampler`'s call signature; records (sampler_type, timestamp) per call.  Member m, frame r of the chunk:
    (0.75 k - 0.25 k / (1 + |k|)) * (1 + 0.125 m) + 0.0625 (r + 1) + hour / 16 + day / 64 + (0.25 for "pipeline"), k = the last known frame"""

    def __init__(self):
        self.calls = []

    def __call__(self, pipeline, sample_size, return_seq_len, num_inference_steps, known_latents=None, timestamps=None, sampler_type="edm",
                 device="cpu", **_):
        ts = int(timestamps.reshape(-1)[0])
        self.calls.append((sampler_type, ts))
        dev = known_latents.device
        k = known_latents[:, :, -1:].to(torch.float32)
        k = k.expand(sample_size, *k.shape[1:])
        m = torch.arange(sample_size, device=dev, dtype=torch.float32).view(-1, 1, 1, 1, 1)
        r = torch.arange(return_seq_len, device=dev, dtype=torch.float32).view(1, 1, -1, 1, 1)
        base = 0.75 * k - 0.25 * k / (1.0 + k.abs())
        shift = (ts % 100) * 0.0625 + ((ts // 100) % 100) * 0.015625 + (0.25 if sampler_type == "pipeline" else 0.0)  # exact in fp32
        return base * (1.0 + 0.125 * m) + 0.0625 * (r + 1.0) + shift


class UpsampleDecoder:
    """decode(z).sample = (1.5 z - 0.25), every latent cell repeated 8 x 8"""

    def __init__(self, device="cpu"):
        self.device = torch.device(device)

    def decode(self, z):
        y = z * 1.5 - 0.25
        return SimpleNamespace(sample=y.repeat_interleave(SCALE, dim=-2).repeat_interleave(SCALE, dim=-1))
