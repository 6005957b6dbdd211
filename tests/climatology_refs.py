"""Float64 reference, exact rational arithmetic, accuracy rule and seeded inputs for the day-of-year climatology
(ladcast_amd.preprocess.climatology, C ABI ldc_climatology_accumulate / ldc_climatology_smooth).  A helper module, not a test; it
restates the definition in numpy and shares no code with the package.

Definition.  Frame at time t -> slot (dayofyear(t) - 1) * 4 + (0, 6, 12, 18).index(t.hour).  Per slot and point: n = the non-NaN
samples, s = their float64 sum.  Window w odd, r = (w - 1) / 2, g_k = exp(-k^2 / (2 sigma^2)), k = -r .. r (sigma <= 0: g_k = 1):
    clim[d, h] = (sum_k g_k s[(d + k) mod n_days, h]) / (sum_k g_k n[(d + k) mod n_days, h]),   NaN where the denominator is 0.

Accuracy rule (from the formats, not fitted).  With num = sum_k g_k s_k, den = sum_k g_k n_k, A = sum_k g_k sum |x| over the window's
samples and m the number of samples in the window:
    |out - exact| <= 2^-24 |exact| + (m + 2 w + 4) 2^-53 A / den
the one fp32 rounding, plus the fp64 accumulation of num (m - 1 additions inside s, w products and w additions), of den and the division.
Against the float64 numpy reference below instead of exact arithmetic the second term is doubled (the reference's own rounding).
"""
from datetime import datetime, timedelta
from fractions import Fraction

import numpy as np

HOURS = (0, 6, 12, 18)
U32, U64 = 2.0 ** -24, 2.0 ** -53


def ref_slot(t: datetime) -> int:
    return (int(t.strftime("%j")) - 1) * 4 + HOURS.index(t.hour)


def ref_weights(window: int, sigma: float) -> np.ndarray:
    r = (window - 1) // 2
    return np.array([1.0 if sigma <= 0 else float(np.exp(-(k * k) / (2.0 * sigma * sigma))) for k in range(-r, r + 1)], dtype=np.float64)


def accumulate_ref(frames, slots, n_slots):
    """frames: float32 (B, ...) in time order -> (sum float64, count int64, sum of |x| float64), each (n_slots, ...); a slot outside
    [0, n_slots) skips its frame.  The sum adds in frame order, as the definition's raw state does: the kernel's bits."""
    shape = (n_slots,) + tuple(frames.shape[1:])
    s, n, a = np.zeros(shape, np.float64), np.zeros(shape, np.int64), np.zeros(shape, np.float64)
    for f, slot in zip(frames, slots):
        if not 0 <= slot < n_slots:
            continue
        ok = ~np.isnan(f)
        v = np.where(ok, f, np.float32(0)).astype(np.float64)
        s[slot] = np.where(ok, s[slot] + v, s[slot])
        a[slot] = np.where(ok, a[slot] + np.abs(v), a[slot])
        n[slot] += ok
    return s, n, a


def smooth_ref(s, n, a, g, n_days, n_hours):
    """(reference float64 (n_days, n_hours, ...), NaN where no sample lies in the window; the rule's second term; the empty mask)"""
    w = len(g)
    r = (w - 1) // 2
    tail = tuple(s.shape[1:])
    s, n, a = (v.reshape((n_days, n_hours) + tail) for v in (s, n.astype(np.float64), a))
    num, den, A, m = (np.zeros_like(s) for _ in range(4))
    for k in range(-r, r + 1):
        num += g[k + r] * np.roll(s, -k, axis=0)  # index d holds s[(d + k) mod n_days]
        den += g[k + r] * np.roll(n, -k, axis=0)
        A += g[k + r] * np.roll(a, -k, axis=0)
        m += np.roll(n, -k, axis=0)
    empty = den == 0
    with np.errstate(all="ignore"):
        ref = np.where(empty, np.nan, num / den)
        term2 = np.where(empty, 0.0, (m + 2 * w + 4) * U64 * A / den)
    return ref, term2, empty


def worst_ratio(out, ref, term2, factor=2.0):
    """largest |out - ref| / (2^-24 |ref| + factor * term2) over the finite entries (0 where both sides are exactly equal); the NaN
    pattern must match exactly (AssertionError otherwise)"""
    out = np.asarray(out, dtype=np.float64).reshape(ref.shape)
    assert np.array_equal(np.isnan(out), np.isnan(ref)), "NaN entries differ from the reference's"
    ok = ~np.isnan(ref)
    err = np.abs(out[ok] - ref[ok])
    bound = U32 * np.abs(ref[ok]) + factor * term2[ok]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max()) if ratio.size else 0.0


def exact_point(samples_by_day, g, d):
    """exact rational (num / den, A / den, m) of day d of ONE point and hour: samples_by_day = per day the list of its float32 samples
    (NaN already left out); None when the window holds no sample"""
    n_days, w = len(samples_by_day), len(g)
    r = (w - 1) // 2
    num = den = A = Fraction(0)
    m = 0
    for k in range(-r, r + 1):
        gk = Fraction(float(g[k + r]))
        for x in samples_by_day[(d + k) % n_days]:
            num += gk * Fraction(float(x))
            A += gk * abs(Fraction(float(x)))
            den += gk
            m += 1
    if den == 0:
        return None
    return num / den, A / den, m


# ---- seeded inputs --------------------------------------------------------------------------------------------------------
def dataset(seed, n_days, n_hours, tail, kind="offset", max_per_slot=3, empty_day=None, empty_points=(), nan_frac=0.1):
    """(frames float32 (N,) + tail, slots) in time order: every slot gets 0 .. max_per_slot frames (a slot of `empty_day` none), spread
    over `max_per_slot` passes through the year.  kind: 'plain' N(0, 1); 'offset' about 280; 'cancel' values of both signs around 1e3
    whose sum nearly cancels.  nan_frac of the values are NaN; `empty_points` (index tuples into tail) are NaN in every frame."""
    rng = np.random.default_rng(seed)
    frames, slots = [], []
    for _ in range(max_per_slot):
        for slot in range(n_days * n_hours):
            if slot // n_hours == empty_day or rng.random() < 0.25:
                continue
            x = rng.standard_normal(tail)
            if kind == "offset":
                x = x * 3 + 280
            elif kind == "cancel":
                x = x + 1.0e3 * rng.choice([-1.0, 1.0], size=tail)
            x = x.astype(np.float32)
            x[rng.random(tail) < nan_frac] = np.nan
            for p in empty_points:
                x[p] = np.nan
            frames.append(x)
            slots.append(slot)
    return np.stack(frames), slots


def year_frames(year_start: datetime, n: int, fn, step_hours=6):
    """n frames `step_hours` apart from year_start: fn(time) -> float32 frame"""
    return np.stack([fn(year_start + timedelta(hours=k * step_hours)) for k in range(n)])
