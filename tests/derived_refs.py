"""Host reference of the derived fields (`ladcast_amd.evaluate.derived`, `ldc_derive_fields`), numpy only (a helper module, not a conftest).

Inputs are de-normalised in fp32 exactly as `inv_norm` (csrc/ensemble_common.h) does: divide only if target_std != 1, multiply, add,
each rounded to fp32.  `diff` is one fp32 subtraction; `speed` and `shear` take the differences, squares, sum and root in float64 and
round once to fp32 (`astype(float32)`)."""
from __future__ import annotations

import numpy as np

KIND_CHANNELS = {"speed": 2, "diff": 2, "shear": 4}


def denorm(x, mean=None, std=None, target_std=1.0):
    """one fp32 plane (any shape) of channel statistics `mean`, `std` -> physical units, as `inv_norm` rounds; mean None: unchanged"""
    v = np.asarray(x, dtype=np.float32)
    if mean is None:
        return v
    with np.errstate(all="ignore"):
        if float(target_std) != 1.0:
            v = (v / np.float32(target_std)).astype(np.float32)
        v = (v * np.float32(std)).astype(np.float32)
        return (v + np.float32(mean)).astype(np.float32)


def field(kind, *p):
    """one derived field from its de-normalised fp32 inputs (a, b[, c, d]) -> fp32"""
    assert len(p) == KIND_CHANNELS[kind]
    p = [np.asarray(v, dtype=np.float32) for v in p]
    with np.errstate(all="ignore"):
        if kind == "diff":
            return (p[0] - p[1]).astype(np.float32)
        x, y = p[0].astype(np.float64), p[1].astype(np.float64)
        if kind == "shear":
            x, y = x - p[2].astype(np.float64), y - p[3].astype(np.float64)
        return np.sqrt(x * x + y * y).astype(np.float32)


def derive(x, fields, axis, mean=None, std=None, target_std=1.0):
    """x: fp32 array with the channels on `axis`; fields: (name, kind, channels[, scale]) tuples -> the D derived fields stacked on
    `axis`, fp32"""
    x = np.asarray(x, dtype=np.float32)
    planes = {}

    def plane(c):
        if c not in planes:
            planes[c] = denorm(np.take(x, c, axis=axis), None if mean is None else float(mean[c]), None if std is None else float(std[c]), target_std)
        return planes[c]

    return np.stack([field(f[1], *(plane(int(c)) for c in f[2])) for f in fields], axis=axis)


def ulp_distance(a, b):
    """per element, the number of fp32 values between a and b (0: equal); +0 == -0, NaN == NaN; NaN against a number: 2^32"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)

    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)  # -0.0 -> 0

    d = np.abs(ordered(a) - ordered(b))
    na, nb = np.isnan(a), np.isnan(b)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 32, d))
