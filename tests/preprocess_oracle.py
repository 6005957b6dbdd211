"""Exact-arithmetic oracle and seeded inputs for the dataset statistics (ladcast_amd.preprocess, C ABI ldc_field_moments).

The reference's statistics script (ladcast/preprocecss/compute_mean_std_era5.py) is xarray's `.mean(skipna=True)` / `.std(skipna=True)`
per channel: the population mean and standard deviation (ddof = 0) of the non-NaN values.  That definition is evaluated here without
rounding that matters: every fp32 value is an exact double, `math.fsum` returns the correctly rounded sum of doubles, so
    mean = hi + lo,  hi = fsum(v) / n,  lo = fsum(v - hi) / n            (lo: what the division and hi's rounding lost)
    M2   = fsum((v - hi)^2) - n lo^2
carry a relative error of a few 2^-53 of the DEVIATIONS, not of |mean|.  `fraction_moments` is the same in rational arithmetic, for
the small cases that pin the float version.

The accuracy rule (derived, not measured): the statistics end up as fp32 (`mean_std_from_json` builds fp32 tensors), whose half-ulp is
2^-24 relative; the rule asks for 2^-34, a thousand times inside that, on the scale of the channel's standard deviation:
    |mean - exact| <= 2^-34 std_exact,  |std - exact| <= 2^-34 std_exact,  counts exact,  a constant channel gives std == 0.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

RULE = 2.0 ** -34


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def exact_channel(values):
    """values: fp32 array of one channel (any shape, NaNs skipped) -> dict(n, mean_hi, mean_lo, m2, std)"""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    v = v[~np.isnan(v)].astype(np.float64)
    n = int(v.size)
    if n == 0:
        return dict(n=0, mean_hi=float("nan"), mean_lo=0.0, m2=float("nan"), std=float("nan"))
    hi = math.fsum(v) / n
    d = v - hi
    lo = math.fsum(d) / n
    m2 = max(math.fsum(d * d) - n * lo * lo, 0.0)
    return dict(n=n, mean_hi=hi, mean_lo=lo, m2=m2, std=math.sqrt(m2 / n))


def exact_moments(x):
    """x: fp32 (B, C, H, W) -> list of `exact_channel` per channel"""
    x = np.asarray(x)
    return [exact_channel(x[:, c]) for c in range(x.shape[1])]


def fraction_moments(values):
    """rational arithmetic: (n, mean, population variance) as Fractions (None, None for n == 0)"""
    v = [Fraction(float(t)) for t in np.asarray(values, dtype=np.float32).reshape(-1) if not math.isnan(t)]
    n = len(v)
    if n == 0:
        return 0, None, None
    mean = sum(v) / n
    return n, mean, sum((t - mean) ** 2 for t in v) / n


def rule_ratios(mean, std, want):
    """(|mean - exact|, |std - exact|) / (2^-34 std_exact) for one channel; std_exact == 0 demands equality (0 or inf); a channel
    without values demands NaN"""
    if want["n"] == 0:
        return (0.0 if math.isnan(mean) else math.inf), (0.0 if math.isnan(std) else math.inf)
    if not (math.isfinite(mean) and math.isfinite(std)):
        return math.inf, math.inf
    em = abs((float(mean) - want["mean_hi"]) - want["mean_lo"])  # the first difference is exact: the two are neighbours
    es = abs(float(std) - want["std"])
    bound = RULE * want["std"]
    if bound == 0.0:
        return (0.0 if em == 0.0 else math.inf), (0.0 if es == 0.0 else math.inf)
    return em / bound, es / bound


def worst_ratio(means, stds, wants):
    """the largest ratio to the rule's bound over the channels (<= 1 passes)"""
    return max(max(rule_ratios(float(m), float(s), w)) for m, s, w in zip(means, stds, wants))


def numpy_stats(x):
    """numpy's float64 nanmean / nanstd of the float64-promoted input, per channel (the condition on the inputs: this must meet the rule)"""
    x64 = np.asarray(x, dtype=np.float64)
    C = x64.shape[1]
    flat = np.moveaxis(x64, 1, 0).reshape(C, -1)
    with np.errstate(all="ignore"):
        import warnings

        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.nanmean(flat, axis=1), np.nanstd(flat, axis=1)


def unpivoted_stats(x):
    """the shortcut a streaming kernel must NOT take: float64 sum x / n and sqrt(sum x^2 / n - mean^2), per channel"""
    x64 = np.asarray(x, dtype=np.float64)
    C = x64.shape[1]
    flat = np.moveaxis(x64, 1, 0).reshape(C, -1)
    n = (~np.isnan(flat)).sum(axis=1)
    mean = np.nansum(flat, axis=1) / n
    var = np.nansum(flat * flat, axis=1) / n - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


# ---- seeded inputs of the GPU tests -----------------------------------------------------------------------------------------------
def _normal(rng, shape, mean=0.0, std=1.0):
    return (rng.standard_normal(shape, dtype=np.float32) * np.float32(std) + np.float32(mean)).astype(np.float32)


def _dense(shape, seed):
    rng = np.random.default_rng(seed)
    C = shape[1]
    x = _normal(rng, shape)
    for c in range(C):
        x[:, c] = x[:, c] * np.float32(0.5 + c) + np.float32(3.0 * c - 2.0)
    return x


def _nan_mix(seed=40):
    """(3, 5, 16, 24): channel 0 all NaN; 1 about 30 % NaN in land-like blocks, with whole rows and a whole batch element; 2 a single
    valid value; 3 constant; 4 plain"""
    rng = np.random.default_rng(seed)
    x = _normal(rng, (3, 5, 16, 24), mean=285.0, std=12.0)
    x[:, 0] = np.nan
    land = np.zeros((16, 24), dtype=bool)
    land[2:6, 3:11] = True
    land[9:13, 14:22] = True
    land[7] = True  # a whole row
    land[15] = True
    x[:, 1][:, land] = np.nan
    x[2, 1] = np.nan  # a whole batch element
    keep = x[1, 2, 5, 7]
    x[:, 2] = np.nan
    x[1, 2, 5, 7] = keep
    x[:, 3] = np.float32(0.1) * np.float32(3.0)
    return x


def _teeth(seed=41):
    """(2, 2, 33, 64): mean 2e5 with std 3, mean 1e5 with std 3e3 - an unpivoted sum of squares loses the variance here"""
    rng = np.random.default_rng(seed)
    x = np.empty((2, 2, 33, 64), dtype=np.float32)
    x[:, 0] = _normal(rng, (2, 33, 64), 2.0e5, 3.0)
    x[:, 1] = _normal(rng, (2, 33, 64), 1.0e5, 3.0e3)
    return x


def _stream(seed=42):
    """(6, 3, 15, 30): six latent-grid frames, NaN blocks in channel 1, one frame of it all NaN"""
    x = _dense((6, 3, 15, 30), seed)
    x[:, 1, 4:9, 10:20] = np.nan
    x[3, 1] = np.nan
    return x


def _physical(seed=43):
    """(2, 84, 121, 240) raw frames; the SST channel (82) is NaN over land-like blocks; the tests view it with the south pole cropped"""
    rng = np.random.default_rng(seed)
    x = _normal(rng, (2, 84, 121, 240))
    for c in range(84):
        x[:, c] = x[:, c] * np.float32(1 + c % 5) + np.float32(50.0 * (c % 7 - 3))
    x[:, 82] = x[:, 82] * np.float32(0.1) + np.float32(288.0)
    land = np.zeros((121, 240), dtype=bool)
    land[20:70, 10:80] = True
    land[30:110, 120:200] = True
    land[:8] = True
    x[:, 82][:, land] = np.nan
    return x


# name -> (storage builder, index of the view the kernel is given).  The statistics are those of storage[view].
_ALL = (slice(None),) * 4
CASES = {
    "one": (lambda: _dense((1, 1, 1, 1), 1), _ALL),
    "scalar_tiny": (lambda: _dense((1, 3, 1, 5), 2), _ALL),
    "latent": (lambda: _dense((2, 4, 15, 30), 3), _ALL),  # scalar path, the latent grid
    "vec_small": (lambda: _dense((2, 5, 7, 8), 4), _ALL),  # vector path, a plane smaller than one chunk
    "chunks_issue": (lambda: _dense((3, 2, 33, 64), 5), _ALL),
    "chunks": (lambda: _dense((2, 2, 150, 64), 6), _ALL),  # 64 rows per 4096-value chunk: 64 + 64 + 22 rows
    "chunks_scalar": (lambda: _dense((2, 2, 150, 30), 7), _ALL),  # 136 rows per chunk: 136 + 14
    "wide_vec": (lambda: _dense((1, 2, 2, 8200), 8), _ALL),  # a row longer than a chunk: pieces of 4096, 4096, 8
    "wide_scalar": (lambda: _dense((1, 1, 2, 4099), 9), _ALL),  # pieces of 4096 and 3
    "crop_vec": (lambda: _dense((2, 4, 9, 8), 10), (slice(None), slice(0, 3), slice(1, None), slice(None))),  # first row cropped, last channel dropped
    "crop_scalar": (lambda: _dense((2, 4, 16, 30), 11), (slice(None), slice(0, 3), slice(1, None), slice(None))),
    "cols_vec": (lambda: _dense((2, 2, 6, 12), 12), (slice(None), slice(None), slice(None), slice(4, 12))),  # row stride > W, aligned
    "cols_unaligned": (lambda: _dense((2, 2, 6, 12), 13), (slice(None), slice(None), slice(None), slice(2, 10))),  # W % 4 == 0 but the base is not 16-byte aligned
    "nan_mix": (_nan_mix, _ALL),
    "teeth": (_teeth, _ALL),
    "stream": (_stream, _ALL),
    "physical": (_physical, (slice(None), slice(None), slice(1, None), slice(None))),
}
STREAM_SPLIT = (1, 3, 2)

_CACHE = {}


def case(name):
    """-> (storage fp32 array, view index, exact moments of storage[view]); computed once, shared, not to be modified"""
    if name not in _CACHE:
        build, view = CASES[name]
        x = build()
        x.setflags(write=False)
        _CACHE[name] = (x, view, exact_moments(x[view]))
    return _CACHE[name]
