"""Day-of-year climatology on the device (C ABI ``ldc_climatology_accumulate`` / ``ldc_climatology_smooth``): the
``(366, 4, C, H, W)`` table, day of year by hour 0 / 6 / 12 / 18, that ``evaluate_ens_gpu`` reads as ``--climatology_path``.

Definition.  A frame at time ``t`` belongs to slot ``(dayofyear(t) - 1) * 4 + hours.index(t.hour)`` (the calendar day of year, 1 .. 366:
the index ``evaluate_ens_gpu.climatology_slots`` computes).  Per slot and point the raw state is the count ``n`` of the non-NaN samples
and their fp64 sum ``s``.  With an odd ``window_days``, ``r = (window_days - 1) / 2`` and the weights ``g_k = exp(-k^2 / (2 sigma^2))``,
``k = -r .. r`` (``sigma <= 0``: ``g_k = 1``, a boxcar),

    clim[d, h] = (sum_k g_k s[(d + k) mod 366, h]) / (sum_k g_k n[(d + k) mod 366, h])

rounded to fp32 once and NaN where the denominator is 0: the weighted mean of all samples in the window, each weighted by its day
offset.  Hours are never mixed, the day axis is circular, and day 366 - which holds about a quarter of the samples of the other days -
simply weighs less.  ``window_days = 1`` is the plain mean of each slot.

The defaults ``window_days = 61``, ``sigma_days = 10`` are this package's own choice; the table does not reproduce any published
climatology.
"""
from __future__ import annotations

from datetime import timedelta
from typing import List, Sequence

import numpy as np
import torch

from .. import hip
from ..evaluate.evaluate_ens_gpu import CLIMATOLOGY_HOURS, _to_datetime

DEFAULT_WINDOW_DAYS, DEFAULT_SIGMA_DAYS = 61, 10.0


def slot_of(time, hours: Sequence[int] = CLIMATOLOGY_HOURS) -> int:
    """``(dayofyear - 1) * len(hours) + hours.index(hour)`` of a time (datetime, numpy datetime64, YYYYMMDDHH integer or ISO string);
    ValueError for a time that is not at one of the hours on the full hour"""
    t = _to_datetime(time)
    hours = [int(h) for h in hours]
    if t.hour not in hours or t.minute or t.second or t.microsecond:
        raise ValueError(f"{t.isoformat()} is not at one of the climatology's hours {hours}")
    return (t.timetuple().tm_yday - 1) * len(hours) + hours.index(t.hour)


def frame_slots(start, n: int, step_size_hour: int, hours: Sequence[int] = CLIMATOLOGY_HOURS) -> List[int]:
    """the slots of ``n`` frames ``step_size_hour`` apart, the first at ``start``"""
    t0 = _to_datetime(start)
    return [slot_of(t0 + timedelta(hours=k * int(step_size_hour)), hours) for k in range(int(n))]


def window_weights(window_days: int, sigma_days: float) -> np.ndarray:
    """float64 ``(window_days,)``: ``exp(-k^2 / (2 sigma^2))`` for ``k = -r .. r``; ones for ``sigma_days <= 0``"""
    w = int(window_days)
    if w != window_days or w < 1 or w % 2 == 0:
        raise ValueError(f"window_days must be an odd positive integer; got {window_days}")
    k = np.arange(-(w // 2), w // 2 + 1, dtype=np.float64)
    if sigma_days <= 0:
        return np.ones(w, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * float(sigma_days) ** 2))


class Climatology:
    """the zeroed device state ``sum`` (fp64) and ``count`` (int32), ``[n_days * n_hours][C][H][W]``, of one channel block"""

    def __init__(self, C: int, H: int, W: int, device="cuda", n_days: int = 366, hours: Sequence[int] = CLIMATOLOGY_HOURS):
        self.C, self.H, self.W, self.n_days = int(C), int(H), int(W), int(n_days)
        self.hours = tuple(int(h) for h in hours)
        if min(self.C, self.H, self.W, self.n_days) < 1 or not self.hours:
            raise ValueError(f"Climatology needs positive sizes; got C, H, W = {C}, {H}, {W}, n_days = {n_days}, hours = {hours}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("Climatology runs on the device (no CPU fallback)")
        self.n_slots = self.n_days * len(self.hours)
        self.sum = torch.zeros(self.n_slots, self.C, self.H, self.W, device=self.device, dtype=torch.float64)
        self.count = torch.zeros(self.n_slots, self.C, self.H, self.W, device=self.device, dtype=torch.int32)
        self._frames = np.zeros(self.n_slots, dtype=np.int64)
        self._n_empty = None

    def update(self, x: torch.Tensor, slots: Sequence[int]) -> "Climatology":
        """x: fp32 device tensor (B, C, H, W) or (C, H, W); any strides with a contiguous last dimension (a cropped or channel-sliced
        view is read where it is).  slots: one per frame, each in ``[0, n_days * n_hours)``.  One launch, no host synchronisation."""
        hip._dev(x)
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x.dim() != 4 or x.dtype != torch.float32:
            raise ValueError(f"Climatology.update takes fp32 (B, C, H, W) or (C, H, W) tensors; got {x.dtype} {tuple(x.shape)}")
        B, C, H, W = x.shape
        if (C, H, W) != (self.C, self.H, self.W):
            raise ValueError(f"the batch's frames are {(C, H, W)}, the climatology's {(self.C, self.H, self.W)}")
        slots = [int(s) for s in slots]
        if len(slots) != B:
            raise ValueError(f"{B} frames, {len(slots)} slots")
        if any(not 0 <= s < self.n_slots for s in slots):
            raise ValueError(f"slots {slots} reach outside the {self.n_slots} slots of the climatology")
        if B == 0:
            return self
        if x.stride(3) != 1 and W > 1:
            raise ValueError("Climatology.update needs a contiguous last dimension")
        if H > 1 and x.stride(2) < W:
            raise ValueError("Climatology.update needs non-overlapping rows (row stride >= W)")
        dev_slots = hip.upload_nonblocking(torch.tensor(slots, dtype=torch.int32), x.device)
        hip.climatology_accumulate(x, dev_slots, self.sum, self.count, B=B, C=C, H=H, W=W, n_slots=self.n_slots, batch_stride=x.stride(0),
                                   channel_stride=x.stride(1), row_stride=x.stride(2) if H > 1 else max(x.stride(2), W))
        np.add.at(self._frames, slots, 1)
        return self

    def finish(self, window_days: int = DEFAULT_WINDOW_DAYS, sigma_days: float = DEFAULT_SIGMA_DAYS) -> torch.Tensor:
        """the smoothed table, an fp32 device tensor ``(n_days, n_hours, C, H, W)``; the state is left as it is"""
        g = window_weights(window_days, sigma_days)
        if len(g) > self.n_days:
            raise ValueError(f"window_days = {len(g)} is longer than the {self.n_days} days of the table")
        out = torch.empty(self.n_days, len(self.hours), self.C, self.H, self.W, device=self.device, dtype=torch.float32)
        self._n_empty = torch.zeros(self.C, device=self.device, dtype=torch.int64)
        hip.climatology_smooth(self.sum, self.count, torch.from_numpy(g).to(self.device), out, self._n_empty, n_days=self.n_days,
                               n_hours=len(self.hours), C=self.C, plane=self.H * self.W)
        return out

    def n_empty(self) -> np.ndarray:
        """int64 ``(C,)``: per channel the (day, hour, point) entries of the last ``finish`` with no sample in their window"""
        if self._n_empty is None:
            raise RuntimeError("n_empty() follows finish()")
        return self._n_empty.cpu().numpy()

    def frames_per_slot(self) -> np.ndarray:
        """host int64 ``(n_days, n_hours)``: the frames seen per slot"""
        return self._frames.reshape(self.n_days, len(self.hours)).copy()
