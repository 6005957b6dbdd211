"""Streaming per-channel statistics on the device (C ABI ``ldc_field_moments``) and the two JSON layouts the rest of the package reads.

``FieldMoments`` keeps ``(n, mean, M2)`` per channel in fp64 on the device; ``update`` merges one batch of fp32 fields into it with one
launch pair and without waiting for the device, NaNs skipped, so a dataset streamed in batches of any size gives the population mean and
standard deviation of the whole - what ``compute_mean_std_era5.py`` takes with xarray's ``.mean(skipna=True)`` / ``.std(skipna=True)``.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import hip


class FieldMoments:
    """``[C][3]`` fp64 device state: count, mean and sum of squared deviations of every channel's non-NaN values seen so far."""

    def __init__(self, C: int, device="cuda"):
        if int(C) < 1:
            raise ValueError(f"FieldMoments needs at least one channel; got {C}")
        self.C = int(C)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FieldMoments runs on the device (no CPU fallback)")
        self.state = torch.empty(self.C, 3, device=self.device, dtype=torch.float64)
        self._started = False  # the first update overwrites the uninitialised state

    def update(self, x: torch.Tensor) -> "FieldMoments":
        """x: fp32 device tensor (B, C, H, W) or (C, H, W); any strides with a contiguous last dimension (a cropped or channel-sliced
        view is read where it is).  One launch pair, no host synchronisation."""
        hip._dev(x)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"FieldMoments.update takes fp32 (B, C, H, W) or (C, H, W) tensors; got {x.dtype} {tuple(x.shape)}")
        B, C, H, W = x.shape
        if C != self.C:
            raise ValueError(f"the batch holds {C} channels, the statistics {self.C}")
        if B == 0:
            return self
        if H < 1 or W < 1:
            raise ValueError(f"empty planes: {tuple(x.shape)}")
        if x.stride(3) != 1 and W > 1:
            raise ValueError("FieldMoments.update needs a contiguous last dimension")
        if H > 1 and x.stride(2) < W:
            raise ValueError("FieldMoments.update needs non-overlapping rows (row stride >= W)")
        hip.field_moments(x, self.state, B=B, C=C, H=H, W=W, batch_stride=x.stride(0), channel_stride=x.stride(1),
                          row_stride=x.stride(2) if H > 1 else max(x.stride(2), W), accumulate=self._started)
        self._started = True
        return self

    def _host(self) -> np.ndarray:
        if not self._started:
            out = np.full((self.C, 3), np.nan)
            out[:, 0] = 0.0
            return out
        return self.state.cpu().numpy()  # the one small device-to-host copy

    def count(self) -> np.ndarray:
        return self._host()[:, 0].astype(np.int64)

    def mean(self) -> np.ndarray:
        """float64 (C,); NaN for a channel without a valid value"""
        return self._host()[:, 1].copy()

    def std(self, ddof: int = 0) -> np.ndarray:
        """float64 (C,): sqrt(M2 / (n - ddof)); ddof = 0 is xarray's and numpy's default.  NaN where n - ddof <= 0."""
        return self.mean_std(ddof)[1]

    def mean_std(self, ddof: int = 0):
        """(mean, std) from one copy of the state"""
        s = self._host()
        dof = s[:, 0] - ddof
        with np.errstate(all="ignore"):
            std = np.where(dof > 0, np.sqrt(s[:, 2] / np.where(dof > 0, dof, 1.0)), np.nan)
        return s[:, 1].copy(), std


def normalization_dict(mean: Sequence[float], std: Sequence[float], variable_names: Sequence[str], levels: Sequence[int],
                       num_atm_vars: Optional[int] = None) -> Dict:
    """The reference's normalisation JSON (static/ERA5_normal_1979_2017.json) from per-channel vectors in channel order: the atmospheric
    variables first, each with one channel per level, then the surface / static ones.  A levelled variable becomes
    ``{"mean": {level: v}, "std": {level: v}}`` with the level keys in the given order (``precompute_mean_std`` iterates the dict), any
    other ``{"mean": v, "std": v}``.  num_atm_vars: how many of the names are levelled; by default whatever makes the channel count
    come out (``len(mean) == num_atm_vars * len(levels) + the rest``)."""
    mean, std = [float(v) for v in np.asarray(mean).reshape(-1)], [float(v) for v in np.asarray(std).reshape(-1)]
    names, levels = list(variable_names), [int(p) for p in levels]
    L, C = len(levels), len(mean)
    if len(std) != C:
        raise ValueError(f"mean holds {C} values, std {len(std)}")
    if len(set(names)) != len(names) or len(set(levels)) != L:
        raise ValueError("variable names and levels must be unique")
    if num_atm_vars is not None:
        n_atm = int(num_atm_vars)
    elif L == 0:
        n_atm = 0
    elif L == 1:
        raise ValueError("one level: pass num_atm_vars, the channel count does not tell the levelled variables apart")
    else:
        n_atm, rest = divmod(C - len(names), L - 1)
        if rest:
            n_atm = -1
    if n_atm < 0 or n_atm > len(names) or (n_atm > 0 and L == 0) or n_atm * L + (len(names) - n_atm) != C:
        raise ValueError(f"{C} channels do not match {len(names)} variable names with {L} levels"
                         + (f" and {n_atm} levelled variables" if n_atm >= 0 else ""))
    out, c = {}, 0
    for i, name in enumerate(names):
        if i < n_atm:
            out[name] = {"mean": {p: mean[c + k] for k, p in enumerate(levels)}, "std": {p: std[c + k] for k, p in enumerate(levels)}}
            c += L
        else:
            out[name] = {"mean": mean[c], "std": std[c]}
            c += 1
    return out


def latent_normal_dict(mean: Sequence[float], std: Sequence[float]) -> Dict:
    """``{"mean": [...], "std": [...]}``: the latent statistics JSON that ``load_latent_transform_args`` reads"""
    mean, std = [float(v) for v in np.asarray(mean).reshape(-1)], [float(v) for v in np.asarray(std).reshape(-1)]
    if len(mean) != len(std) or not mean:
        raise ValueError(f"mean holds {len(mean)} values, std {len(std)}")
    return {"mean": mean, "std": std}
