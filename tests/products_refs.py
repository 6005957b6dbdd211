"""float64 oracle, COUNTED bounds, an fp32 restatement (with planted defects) and the case tables of the ensemble-products kernel
(csrc/products.hip: ldc_rollout_products).  tests/test_gpu_products.py runs the kernel; tests/test_products_cpu.py proves on the CPU
that every bound admits a correct fp32 implementation in the kernel's order and that every planted defect is caught.

Definitions, per grid point with the fp32 members x_i the kernel sees (after `inv_norm_f32` where the inverse
normalisation is fused):
    mean = sum_i x_i / M,  std = sqrt(sum_i (x_i - mean)^2 / (M - 1))  (M == 1: NaN),  min,  max
    quantile q = numpy.quantile(x, q, method="linear"): pos = q (M - 1), lo = min(floor(pos), M - 1), hi = min(lo + 1, M - 1),
        t = pos - lo;  x_(lo) when t == 0, else x_(lo) + (x_(hi) - x_(lo)) t
    exceed (thr, +1) = #{x_i > thr} / M,  (thr, -1) = #{x_i < thr} / M;  a NaN threshold: NaN
    a point with a NaN member is NaN in every product; +-inf are ordinary ordered values.
The oracle is float64 arithmetic (numpy.quantile, mean, std(ddof=1)) on the fp32 values; min, max, the order statistics and the counts
are properties of the fp32 values themselves, so they are compared exactly, BY VALUE (-0 == +0).

Bounds, counted from the kernel's arithmetic with U = 2**-24, nothing fitted; every bound is multiplied by (1 + 8 U) for the second-order
terms and, where a value is formed from quantities that carry a bound themselves, the bounds enter the formulas (b_e below):
  mean      M - 1 additions of the sequential sum (each at most U times the partial sum, <= U sum |x_i|), then one division:
            b_mean = (M - 1) U sum |x_i| / M + U |mean|
  std       M subtractions e_i = x_i - mean: b_e = b_mean + U |e_i|
            M squares: e_i^2 carries 2 |e_i| b_e + b_e^2 + U (|e_i| + b_e)^2
            M - 1 additions of the squares: (M - 1) U T with T = sum_i (|e_i| + b_e)^2          -> b_ss
            1 division by M - 1: b_var = (b_ss + U (ss + b_ss)) / (M - 1)
            1 square root (monotone, correctly rounded): the larger deviation of sqrt at var +- b_var, plus U sqrt(var + b_var)
            in all M + M + (M - 1) + 1 + 1 = 3 M + 1 roundings behind those of the mean
  quantile  t == 0: exact.  Otherwise 4 roundings: t to fp32 (|b - a| t U), b - a (|b - a| t U), the product (|b - a| t U), the sum
            (U |a + (b - a) t| <= U max(|a|, |b|)):  b_q = U (3 |b - a| t + max(|a|, |b|))
  min, max, exceed   exact (exceed: the one division float(count) / float(M) is correctly rounded; the float64 quotient of two
            integers <= 1024 rounds to the same fp32)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests.redzone import U
from tests.score_edge_refs import _seed, gen, inv_norm_f32, same_value_bits  # noqa: F401  (shared, not copied)

TPB = 256
MAX_Q, MAX_P, MAX_M, MAX_SORT_M = 16, 8, 1024, 64
STAT_NAMES = ("mean", "std", "min", "max")
SECOND = 1.0 + 8 * U  # second-order terms of every counted bound
SHAPES = ((3, 70), (3, 86))  # one partial workgroup; two workgroups with a ragged tail
C, L, L_OFF, L_TOTAL = 3, 2, 1, 4
QUANTILES = (0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0)
REGISTER_M = (1, 2, 3, 4, 5, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64)  # both ends of every register arm
STREAM_M = (65, 100, 1024)


def quantile_pos(q, M):
    """-> (lo, t as the fp32 value the kernel multiplies by), in float64 as the host forms them"""
    pos = float(q) * (M - 1)
    lo = min(int(math.floor(pos)), M - 1)
    return lo, float(np.float32(pos - lo))


# ---- float64 oracle with bounds ----------------------------------------------------------------------------------------------------
def products_ref(x, quantiles=(), thr=None, dirs=()):
    """x (M, C, ...) the fp32 values the kernel sees, thr (P, C) fp32 | None, dirs P values +-1 -> dict:
    mean, std: (float64 value, bound) (C, ...);  min, max: fp32 (C, ...);  quantiles: [(float64 value, bound, exact)] per q, `exact`
    True where t == 0 (then the value is an order statistic);  exceed: fp32 (P, C, ...).  NaN members poison their point."""
    xf = x.float()
    M = xf.shape[0]
    x64 = xf.double()
    poison = torch.isnan(xf).any(0)
    nan64 = torch.full(x64.shape[1:], float("nan"), dtype=torch.float64)
    mean = x64.sum(0) / M
    b_mean = ((M - 1) * U * x64.abs().sum(0) / M + U * mean.abs()) * SECOND
    e = x64 - mean.unsqueeze(0)
    b_e = b_mean.unsqueeze(0) + U * e.abs()
    ss = (e * e).sum(0)
    b_sq = 2 * e.abs() * b_e + b_e * b_e + U * (e.abs() + b_e) ** 2
    T = ((e.abs() + b_e) ** 2).sum(0)
    b_ss = b_sq.sum(0) + (M - 1) * U * T
    if M >= 2:
        var, b_var = ss / (M - 1), (b_ss + U * (ss + b_ss)) / (M - 1)
        std = torch.from_numpy(np.std(x64.numpy(), axis=0, ddof=1)) if not poison.any() and bool(torch.isfinite(x64).all()) else torch.sqrt(var)
        hi, lo = torch.sqrt(var + b_var), torch.sqrt((var - b_var).clamp_min(0.0))
        b_std = (torch.maximum(hi - torch.sqrt(var), torch.sqrt(var) - lo) + U * hi) * SECOND
    else:
        std, b_std = nan64.clone(), nan64.clone()
    out = dict(mean=(torch.where(poison, nan64, mean), b_mean), std=(torch.where(poison, nan64, std), b_std))
    nan32 = torch.full(xf.shape[1:], float("nan"))
    out["min"], out["max"] = torch.where(poison, nan32, xf.min(0).values), torch.where(poison, nan32, xf.max(0).values)
    qs = []
    clean = torch.where(poison.unsqueeze(0), torch.zeros_like(x64), x64)  # numpy.quantile on the points without NaN; poisoned afterwards
    srt = clean.sort(0).values
    for q in quantiles:
        lo_i, t = quantile_pos(q, M)
        a, b = srt[lo_i], srt[min(lo_i + 1, M - 1)]
        if bool(torch.isfinite(clean).all()):
            v = torch.from_numpy(np.quantile(clean.numpy(), float(q), axis=0, method="linear"))
        else:  # +-inf members: IEEE arithmetic on the two order statistics (inf - inf = NaN), which numpy follows too
            v = a if t == 0 else a + (b - a) * (float(q) * (M - 1) - lo_i)
        if t == 0:
            v = a  # the order statistic itself, by definition exact
        bound = U * (3 * (b - a).abs() * t + torch.maximum(a.abs(), b.abs())) * SECOND
        qs.append((torch.where(poison, nan64, v), torch.zeros_like(bound) if t == 0 else bound, t == 0))
    out["quantiles"] = qs
    if thr is not None and len(dirs):
        ex = []
        Mf = torch.tensor(float(M))
        for k, d in enumerate(dirs):
            tk = thr[k].float().view((-1,) + (1,) * (xf.dim() - 2))
            cnt = ((xf > tk) if d > 0 else (xf < tk)).sum(0)
            v = cnt.float() / Mf
            ex.append(torch.where(poison | torch.isnan(tk).expand_as(v), nan32, v))
        out["exceed"] = torch.stack(ex)
    return out


def ratio(got, want, bound):
    """worst |got - want| / bound over the finite oracle values; inf when the NaN / inf pattern differs or a zero bound is missed"""
    got, want, bound = torch.as_tensor(got).detach().cpu().double(), want.double(), bound.double()
    if got.shape != want.shape or not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    inf = torch.isinf(want)
    if not torch.equal(got[inf], want[inf]):
        return float("inf")
    fin = torch.isfinite(want)
    err = (got[fin] - want[fin]).abs()
    b = bound[fin]
    r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def equal_by_value(got, want):
    """the same NaN pattern and equal values elsewhere (-0 == +0, inf == inf)"""
    got, want = torch.as_tensor(got).detach().cpu().float(), torch.as_tensor(want).float()
    if got.shape != want.shape or not torch.equal(torch.isnan(got), torch.isnan(want)):
        return False
    ok = ~torch.isnan(want)
    return bool((got[ok] == want[ok]).all())


def check(got, ref, what=""):
    """got {mean, std, min, max (C, ...); quantiles (Q, C, ...); exceed (P, C, ...)} (keys may be absent where ref has none) against
    products_ref's dict: min / max / t == 0 quantiles / exceed equal by value, the rest within its bound.  Returns the worst err / bound."""
    worst = 0.0
    for k in ("mean", "std"):
        if k in got:
            r = ratio(got[k], *ref[k])
            assert r <= 1.0, f"{what}: {k} misses its bound: err / bound {r:.3g}"
            worst = max(worst, r)
    for k in ("min", "max"):
        if k in got:
            assert equal_by_value(got[k], ref[k]), f"{what}: {k} differs"
    if ref["quantiles"]:
        gq = torch.as_tensor(got["quantiles"]).detach().cpu()
        assert gq.shape[0] == len(ref["quantiles"]), f"{what}: {gq.shape[0]} quantile planes for {len(ref['quantiles'])}"
        for i, (v, b, exact) in enumerate(ref["quantiles"]):
            if exact:
                assert equal_by_value(gq[i], v.float()), f"{what}: quantile {i} (t == 0) is not the order statistic"
            else:
                r = ratio(gq[i], v, b)
                assert r <= 1.0, f"{what}: quantile {i} misses its bound: err / bound {r:.3g}"
                worst = max(worst, r)
    if "exceed" in ref:
        assert equal_by_value(got["exceed"], ref["exceed"]), f"{what}: exceed differs"
    return worst


# ---- the kernel's arithmetic in fp32 torch, with planted defects ------------------------------------------------------------------------
DEFECTS = ("lo_off", "pos_qM", "ddof0", "ge", "descending", "nan_ignored")


def kernel_f32(x, quantiles=(), thr=None, dirs=(), *, defect=None):
    """products_kernel restated in fp32 torch: the sequential sum in member order, the two-pass squared deviations, an ascending sort, the
    compare-and-select of x_(lo) / x_(hi), a + (b - a) * t in three fp32 operations, counts / M.  -> the keys of a `rollout_products` result
    for one lead time.  Planted defects:
      lo_off: lo + 1 in place of lo;  pos_qM: pos = q M in place of q (M - 1);  ddof0: M in place of M - 1;  ge: x >= thr counted in
      place of x > thr;  descending: the members sorted downwards;  nan_ignored: a NaN member skipped instead of poisoning the point"""
    assert defect in (None,) + DEFECTS
    x = x.float()
    M = x.shape[0]
    Mf = torch.tensor(float(M))
    poison = torch.isnan(x).any(0)
    nanv = torch.full(x.shape[1:], float("nan"))
    if defect == "nan_ignored":  # what fminf / fmaxf / a false comparison do with a NaN when nothing poisons the point
        xs = torch.where(torch.isnan(x), torch.zeros_like(x), x)
        mn = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x).min(0).values
        mx = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x).max(0).values
        poison = torch.zeros_like(poison)
    else:
        xs, mn, mx = x, x.min(0).values, x.max(0).values
    s = torch.zeros(x.shape[1:])
    for i in range(M):
        s = s + xs[i]
    mean = s / Mf
    ss = torch.zeros(x.shape[1:])
    for i in range(M):
        e = xs[i] - mean
        ss = ss + e * e
    std = torch.sqrt(ss / (Mf if defect == "ddof0" else Mf - 1.0))
    out = dict(mean=torch.where(poison, nanv, mean), std=torch.where(poison, nanv, std), min=torch.where(poison, nanv, mn),
               max=torch.where(poison, nanv, mx))
    if len(quantiles):
        srt = torch.where(poison.unsqueeze(0), torch.zeros_like(xs), xs).sort(0, descending=defect == "descending").values
        planes = []
        for q in quantiles:
            if defect == "pos_qM":
                pos = float(q) * M
                lo = min(int(math.floor(pos)), M - 1)
                t = float(np.float32(pos - lo))
            else:
                lo, t = quantile_pos(q, M)
            if defect == "lo_off":
                lo = min(lo + 1, M - 1)
            a, b = srt[lo], srt[min(lo + 1, M - 1)]
            r = a if t == 0 else a + (b - a) * torch.tensor(t, dtype=torch.float32)
            planes.append(torch.where(poison, nanv, r))
        out["quantiles"] = torch.stack(planes)
    if thr is not None and len(dirs):
        planes = []
        for k, d in enumerate(dirs):
            tk = thr[k].float().view((-1,) + (1,) * (x.dim() - 2))
            if d > 0:
                cnt = (x >= tk).sum(0) if defect == "ge" else (x > tk).sum(0)
            else:
                cnt = (x < tk).sum(0)
            planes.append(torch.where(poison | torch.isnan(tk).expand_as(nanv), nanv, cnt.float() / Mf))
        out["exceed"] = torch.stack(planes)
    return out


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# a / b. small integers: every sum is exact, so the mean is the float64 value rounded once; many ties among the members and with the
#        thresholds, which are integers from the same range
INT_DIRS = (1, -1, 1)


@functools.lru_cache(maxsize=None)
def integer_case(M, H, W):
    """x (M, C, L, H, W) integers in -12 .. 12; thr (3, C) integers"""
    g = gen(_seed(M, H, W, 5))
    x = torch.randint(-12, 13, (M, C, L, H, W), generator=g).float()
    thr = torch.tensor([[0.0, 3.0, -2.0], [1.0, -4.0, 5.0], [-12.0, 12.0, 0.0]])
    return dict(x=x, thr=thr, dirs=INT_DIRS)


# c. order and ties: duplicates, -0 / +0, +-inf members
@functools.lru_cache(maxsize=None)
def ties_case(M, H, W, with_inf):
    """x (M, C, L, H, W): values from a set of 5 (so most members are duplicated), +0 and -0 among them; with_inf: the first member of
    every third point is -inf and the last member of every fifth point +inf.  thr (4, C): a value of the set above and below, -inf, +inf"""
    g = gen(_seed(M, H, W, 11 + int(with_inf)))
    vals = torch.tensor([-1.5, -0.0, 0.0, 0.25, 2.0])
    x = vals[torch.randint(0, 5, (M, C, L, H, W), generator=g)]
    if with_inf:
        p = torch.arange(H * W).reshape(H, W)
        x[0][..., p % 3 == 0] = float("-inf")
        x[M - 1][..., p % 5 == 0] = float("inf")
    thr = torch.tensor([[0.25, 0.0, 2.0], [0.25, 0.0, 2.0], [float("-inf")] * 3, [float("inf")] * 3])
    return dict(x=x, thr=thr, dirs=(1, -1, 1, 1))


# d. physical scale: normalised values and the statistics of 2 m temperature, mean sea level pressure and 500 hPa geopotential
PHYS_MEAN = torch.tensor([278.5, 100950.0, 54100.0])
PHYS_STD = torch.tensor([21.3, 1330.0, 3350.0])
PHYS_THR = ((303.15, 1), (98000.0, -1))  # on channels 0 and 1
PHYS_M = (10, 50)


@functools.lru_cache(maxsize=None)
def physical_case(M, H, W):
    """v (M, C, L, H, W) normalised, a smooth field plus member noise"""
    g = gen(_seed(M, H, W, 23))
    base = torch.randn(1, C, L, H, W, generator=g) * 1.2
    return dict(v=base + 0.3 * torch.randn(M, C, L, H, W, generator=g), mean=PHYS_MEAN, std=PHYS_STD)


def phys_thresholds(channels):
    """(2, len(channels)) table: each threshold on its own channel, NaN elsewhere; directions"""
    thr = torch.full((2, len(channels)), float("nan"))
    for k, ((v, _), c) in enumerate(zip(PHYS_THR, (0, 1))):
        if c in channels:
            thr[k, list(channels).index(c)] = v
    return thr, tuple(d for _, d in PHYS_THR)


# e. the NaN table: one NaN member at one point of every (channel, lead time); a NaN threshold in one (plane, channel)
NAN_M = 9


@functools.lru_cache(maxsize=None)
def nan_case(H, W):
    """the integer case with member 4 of point (1, W - 3) NaN; threshold 1 of channel 2 NaN"""
    c = integer_case(NAN_M, H, W)
    x, thr = c["x"].clone(), c["thr"].clone()
    x[4, :, :, 1, W - 3] = float("nan")
    thr[1, 2] = float("nan")
    return dict(x=x, thr=thr, dirs=c["dirs"], point=(1, W - 3), nan_thr=(1, 2))


def ref_of(x, l, quantiles, thr, dirs, channels=None):
    """products_ref of lead time l of x (M, C, L, H, W), for the selected channels"""
    xs = x[:, :, l] if channels is None else x[:, list(channels), l]
    return products_ref(xs, quantiles, thr, dirs)


def column(d, l):
    """lead time l of a rollout_products result as the dict `check` takes"""
    out = {k: d[k][:, l] for k in STAT_NAMES if k in d}
    for k in ("quantiles", "exceed"):
        if k in d:
            out[k] = d[k][:, :, l]
    return out
