"""float64 oracle, COUNTED bounds, an fp32 restatement (with planted defects) and the case tables of the ensemble-reliability kernel
(csrc/reliability.hip: ldc_rollout_reliability).  tests/test_gpu_reliability.py runs the kernel; tests/test_reliability_cpu.py proves on
the CPU that every bound admits a correct fp32 implementation in the kernel's order (with and without contraction) and that every
planted defect is caught.  Shared helpers and cases come from tests/score_edge_refs.py.

Definitions, per grid point with the fp32 members x_i the kernel scores (after `inv_norm_f32` where the inverse
normalisation is fused), truth t, latitude weight w:
    mean = sum_i x_i / M,  se = (mean - t)^2,  var = sum_i (x_i - mean)^2 / (M - 1)  (M == 1: 0 / 0 = NaN)
    bin = #{x_i < t} + (#{x_i == t} >> 1)  in 0 .. M;  the point is valid when no member and not the truth is NaN (inf is ordered)
    ens_mse = <w se>, ens_var = <w var>: mean (one NaN point -> NaN), the nan_channel by nanmean;  ssr = sqrt((M + 1) / M) sqrt(ens_var / ens_mse)
The histograms are computed on the fp32 values themselves, so the bins are exact: hist_count and n_invalid must be equal bit for bit.

Bounds, first order in U = 2**-24 (redzone.elementwise_bound), counted from the kernel's arithmetic, nothing fitted:
  mean   M - 1 additions, one division                                   b_mean = M U sum |x_i| / M
  se     d = mean - t: b_d = b_mean + U |d|;  d d: 2 |d| b_d + b_d^2 + U (|d| + b_d)^2
  var    e_i = x_i - mean: b_e = b_mean + U |e_i|;  e_i^2 as d d;  M - 1 additions of the squares: (M - 1) U T, T = sum (|e_i| + b_e)^2;
         the division by M - 1: U (ss + b_ss) / (M - 1)
  every point value is multiplied by w: b w + U |q w|
  grid mean over P points, `tpw` tiles of 256 per workgroup, nrec = ceil(ceil(P / 256) / tpw) records: on sum |q w|
         tpw (a thread's tiles) + 6 (butterfly) + 2 (4 wave totals pairwise) + ceil(nrec / 64) (records per lane) + 6 (butterfly) + 1 (division)
  ssr    r = var / mse lies in [(var - b_v) / (mse + b_m), (var + b_v) / (mse - b_m)] (no claim where mse <= b_m); the square root is monotone,
         so the deviation of sqrt(r) is the larger of the two ends'; plus 5 U: (M + 1) / M and its root (2), the division, the root, the product
  hist_weight[b]  a sequential sum of the weights of the n_b points of the bin, then nrec records: (n_b + nrec) U sum w
"""
from __future__ import annotations

import functools

import torch

from tests import score_edge_refs as R
from tests.redzone import U
from tests.score_edge_refs import PHYS, cos_weights, gen, guard_case, integer_rows, inv_norm_f32  # noqa: F401  (shared, not copied)

TPB = R.TPB
MAX_M = 1024
NAMES = ("ens_mse", "ens_var", "ssr")
GUARD_CASES, GUARD_SLOTS, N_TRUTH = R.GUARD_CASES, R.GUARD_SLOTS, R.N_TRUTH


def tiles_per_wg(M):
    """reliability.hip: the record grows with M, so a workgroup covers more 256-point tiles"""
    return 1 if M <= 64 else -(-M // 64)


def n_records(P, M):
    return -(-(-(-P // TPB)) // tiles_per_wg(M))


def n_reduce(P, M):
    return tiles_per_wg(M) + 6 + 2 + -(-n_records(P, M) // 64) + 6 + 1


# ---- float64 oracle with bounds ----------------------------------------------------------------------------------------------------
def bins_of(x, t):
    """x (M, ...) fp32, t (...) fp32 -> (bin int64 (...), valid bool (...)), compared as fp32 values"""
    x, t = x.float(), t.float()
    lt, eq = (x < t.unsqueeze(0)).sum(0), (x == t.unsqueeze(0)).sum(0)
    valid = ~torch.isnan(x).any(0) & ~torch.isnan(t)
    return lt + eq // 2, valid


def _square(a, b_a):
    return a * a, 2 * a.abs() * b_a + b_a * b_a + U * (a.abs() + b_a) ** 2


def point_ref(x, t):
    """-> {se, var: (float64 value, bound)} per point; NaN / inf follow the elementwise rules"""
    x, t = x.double(), t.double()
    M = x.shape[0]
    mean = x.sum(0) / M
    b_mean = M * U * x.abs().sum(0) / M
    d = mean - t
    se = _square(d, b_mean + U * d.abs())
    e = x - mean.unsqueeze(0)
    b_e = b_mean.unsqueeze(0) + U * e.abs()
    sq, b_sq = _square(e, b_e)
    ss, T = sq.sum(0), ((e.abs() + b_e) ** 2).sum(0)
    b_ss = b_sq.sum(0) + (M - 1) * U * T
    if M >= 2:
        var = (ss / (M - 1), (b_ss + U * (ss + b_ss)) / (M - 1))
    else:
        var = (torch.full_like(ss, float("nan")),) * 2
    return dict(se=se, var=var)


def grid_mean(q, bq, nanmean, M):
    """q, bq (C, P) weighted point values and bounds, nanmean (C,) bool -> (value, bound) (C,)"""
    C, P = q.shape
    valid = ~torch.isnan(q)
    cnt = valid.sum(-1).double()
    qz = torch.where(valid, q, torch.zeros_like(q))
    s, sabs, sb = qz.sum(-1), qz.abs().sum(-1), torch.where(valid, bq, torch.zeros_like(bq)).sum(-1)
    nan = torch.full_like(s, float("nan"))
    ok = torch.where(nanmean, cnt > 0, cnt == P)
    den = cnt.clamp_min(1.0)
    return torch.where(ok, s / den, nan), torch.where(ok, (sb + n_reduce(P, M) * U * sabs) / den, nan)


def ssr_from(var, b_v, mse, b_m, M):
    c = ((M + 1) / M) ** 0.5
    ssr = c * torch.sqrt(var / mse)
    ok = (mse - b_m > 0) & torch.isfinite(ssr)
    one = torch.ones_like(mse)
    hi = torch.sqrt((var + b_v) / torch.where(ok, mse - b_m, one))
    lo = torch.sqrt(((var - b_v) / (mse + b_m)).clamp_min(0.0))
    mid = torch.sqrt(var / mse)
    dev = torch.maximum(hi - mid, mid - lo)
    return ssr, torch.where(ok, c * dev + 5 * U * c * hi, torch.full_like(hi, float("inf")))


def reliability_ref(x, t, w, nan_channel=-1):
    """x (M, C, H, W) the fp32 values the kernel scores, t (C, H, W), w (H,) -> dict: ens_mse, ens_var, ssr (value, bound) (C,);
    hist (C, M + 1) int64; hist_w (value, bound) (C, M + 1) float64; n_invalid (C,) int64"""
    M, C, H, W = x.shape
    P = H * W
    pt = point_ref(x, t)
    wp = w.double().view(1, H, 1).expand(C, H, W)
    nm = torch.zeros(C, dtype=torch.bool)
    if nan_channel >= 0:
        nm[nan_channel] = True

    def weighted(name):
        v, b = pt[name]
        return (v * wp).reshape(C, P), (b * wp + U * (v * wp).abs()).reshape(C, P)

    mse, var = grid_mean(*weighted("se"), nm, M), grid_mean(*weighted("var"), nm, M)
    b, valid = bins_of(x, t)
    b, valid, wf = b.reshape(C, P), valid.reshape(C, P), wp.reshape(C, P)
    hist, hist_w = torch.zeros(C, M + 1, dtype=torch.int64), torch.zeros(C, M + 1, dtype=torch.float64)
    for c in range(C):
        hist[c] = torch.bincount(b[c][valid[c]], minlength=M + 1)
        hist_w[c] = torch.bincount(b[c][valid[c]], weights=wf[c][valid[c]], minlength=M + 1)
    b_hw = (hist + n_records(P, M)).double() * U * hist_w
    return dict(ens_mse=mse, ens_var=var, ssr=ssr_from(*var, *mse, M), hist=hist, hist_w=(hist_w, b_hw), n_invalid=(~valid).sum(-1))


def brute_force(x, t, w, nan_channel=-1):
    """the definitions as a Python loop over points (float64 on the fp32 values; tiny cases only) -> values as reliability_ref, no bounds"""
    import math

    M, C, H, W = x.shape
    out = dict(ens_mse=[], ens_var=[], ssr=[], hist=torch.zeros(C, M + 1, dtype=torch.int64), hist_w=torch.zeros(C, M + 1, dtype=torch.float64),
               n_invalid=torch.zeros(C, dtype=torch.int64))
    nan = float("nan")
    for c in range(C):
        ses, vars_ = [], []
        for h in range(H):
            for k in range(W):
                xs, tt, ww = [float(v) for v in x[:, c, h, k]], float(t[c, h, k]), float(w[h])
                mean = sum(xs) / M
                ses.append((mean - tt) ** 2 * ww)
                vars_.append(sum((v - mean) ** 2 for v in xs) / (M - 1) * ww if M > 1 else nan)
                if any(math.isnan(v) for v in xs) or math.isnan(tt):
                    out["n_invalid"][c] += 1
                    continue
                lt, eq = sum(v < tt for v in xs), sum(v == tt for v in xs)
                out["hist"][c, lt + eq // 2] += 1
                out["hist_w"][c, lt + eq // 2] += ww
        for key, vals in (("ens_mse", ses), ("ens_var", vars_)):
            good = [v for v in vals if not math.isnan(v)]
            if c == nan_channel:
                out[key].append(sum(good) / len(good) if good else nan)
            else:
                out[key].append(sum(good) / len(vals) if len(good) == len(vals) else nan)
        mse, var = out["ens_mse"][-1], out["ens_var"][-1]
        out["ssr"].append(math.sqrt((M + 1) / M) * math.sqrt(var / mse) if mse > 0 and var >= 0 else nan)
    for k in NAMES:
        out[k] = torch.tensor(out[k], dtype=torch.float64)
    return out


judge, ratio_of, same_bits, same_value_bits = R.judge, R.ratio_of, R.same_bits, R.same_value_bits


def check(got, ref, what=""):
    """got {ens_mse, ens_var, ssr (C,), hist, hist_w (C, M + 1), n_invalid (C,)} against reliability_ref's dict: the integers equal, every
    float within its bound; returns the worst err / bound ratio.  Raises AssertionError."""
    gh, gn = torch.as_tensor(got["hist"]).cpu().long(), torch.as_tensor(got["n_invalid"]).cpu().long()
    assert torch.equal(gh, ref["hist"]), f"{what}: hist_count differs at {(gh != ref['hist']).nonzero()[:4].tolist()}"
    assert torch.equal(gn, ref["n_invalid"]), f"{what}: n_invalid {gn.tolist()} != {ref['n_invalid'].tolist()}"
    worst = judge(got["hist_w"], ref["hist_w"], f"{what} hist_weight")
    for k in NAMES:
        worst = max(worst, judge(got[k], ref[k], f"{what} {k}"))
    return worst


# ---- the kernel's arithmetic in fp32 torch, with planted defects ------------------------------------------------------------------------
DEFECTS = ("le", "no_tie", "ddof0", "var_first", "record_twice", "point_W")


def kernel_f32(x, t, w, nan_channel=-1, *, fma=False, defect=None):
    """reliability_kernel + reliability_finish_kernel restated in fp32 torch: member-order sums, the two-pass variance, a thread's tiles in
    order, butterfly per wave, the 4 wave totals pairwise, the finish (records r, r + 64, ... per lane, butterfly, the count rules); the
    histogram as one sequential sum per workgroup and bin in point order, then the records in order.  `fma`: ss += e e fused (what a build
    with contraction would do) or not.  -> the values of reliability_ref (fp32 / int64).  Planted defects:
      le: x_i <= t counted in place of x_i < t;  no_tie: the tie offset eq >> 1 dropped;  ddof0: M in place of M - 1;  var_first: the variance
      about the first member instead of the mean;  record_twice: workgroup record 1 (0 if there is one) added twice to the histogram;
      point_W: the members read W points further on (wrapping inside the plane)"""
    assert defect in (None,) + DEFECTS
    x, t, w = x.float(), t.float(), w.float()
    M, C, H, W = x.shape
    P = H * W
    x, t = x.reshape(M, C, P), t.reshape(C, P)
    if defect == "point_W":
        x = x.roll(-W, dims=-1)
    wp = w.view(1, H, 1).expand(C, H, W).reshape(C, P)
    Mf = torch.tensor(float(M))
    s = torch.zeros(C, P)
    for i in range(M):
        s = s + x[i]
    mean = s / Mf
    centre = x[0] if defect == "var_first" else mean
    ss = torch.zeros(C, P)
    for i in range(M):
        e = x[i] - centre
        ss = (e.double() * e.double() + ss.double()).float() if fma else e * e + ss
    var = ss / (Mf if defect == "ddof0" else Mf - 1.0)
    d = mean - t
    se = d * d
    lt = (x <= t.unsqueeze(0)).sum(0) if defect == "le" else (x < t.unsqueeze(0)).sum(0)
    eq = (x == t.unsqueeze(0)).sum(0)
    b = (lt if defect == "no_tie" else lt + eq // 2).clamp_max(M)
    valid = ~torch.isnan(x).any(0) & ~torch.isnan(t)
    tpw, nrec = tiles_per_wg(M), n_records(P, M)
    Pp = nrec * tpw * TPB

    def pad(v, fill=0):
        out = torch.full((C, Pp), fill, dtype=v.dtype)
        out[:, :P] = v
        return out

    def reduce(v):
        th = pad(v).reshape(C, nrec, tpw, 4, 64)
        acc = torch.zeros(C, nrec, 4, 64)
        for k in range(tpw):
            acc = acc + th[:, :, k]
        waves = R._butterfly(acc)
        rec = (waves[..., 0] + waves[..., 1]) + (waves[..., 2] + waves[..., 3])
        rp = torch.zeros(C, -(-nrec // 64) * 64)
        rp[:, :nrec] = rec
        lanes = torch.zeros(C, 64)
        for k in range(rp.shape[1] // 64):
            lanes = lanes + rp[:, k * 64:(k + 1) * 64]
        return R._butterfly(lanes)

    def avg(q):
        ok = ~torch.isnan(q)
        tot, cnt = reduce(torch.where(ok, q * wp, torch.zeros_like(q))), ok.sum(-1)
        out = torch.full((C,), float("nan"))
        for c in range(C):
            if (c == nan_channel and cnt[c] > 0) or (c != nan_channel and cnt[c] == P):
                out[c] = tot[c] / cnt[c].float()
        return out

    mse, v = avg(se), avg(var)
    ssr = torch.sqrt((Mf + 1.0) / Mf) * torch.sqrt(v / mse)
    # histogram records: a sequential sum over each workgroup's points
    per = tpw * TPB
    bb, ww = pad(torch.where(valid, b, torch.full_like(b, -1)), -1).reshape(C * nrec, per), pad(wp).reshape(C * nrec, per)
    hc, hw = torch.zeros(C * nrec, M + 1, dtype=torch.int64), torch.zeros(C * nrec, M + 1)
    rows = torch.arange(C * nrec)
    for p in range(min(per, P)):
        m = bb[:, p] >= 0
        hc[rows[m], bb[m, p]] += 1
        hw[rows[m], bb[m, p]] += ww[m, p]
    hc, hw = hc.reshape(C, nrec, M + 1), hw.reshape(C, nrec, M + 1)
    hist, hist_w = torch.zeros(C, M + 1, dtype=torch.int64), torch.zeros(C, M + 1)
    twice = (1 if nrec > 1 else 0) if defect == "record_twice" else -1
    for r in range(nrec):
        for _ in range(2 if r == twice else 1):
            hist, hist_w = hist + hc[:, r], hist_w + hw[:, r]
    return dict(ens_mse=mse, ens_var=v, ssr=ssr, hist=hist, hist_w=hist_w, n_invalid=(~valid).sum(-1))


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# a. integers on which EVERY fp32 operation up to the last division is exact, so ens_mse and ens_var are the float64 value rounded once:
#    x_i = c + a e_i with a = max(M - 1, 1), e_i in {-1, 0, 1}, sum e_i = 0 -> the mean is c, var = a sum e_i^2 (an integer), and the
#    weights are multiples of 1/4; few enough e_i are non-zero for every partial sum of 4 w var to stay below 2**24.
INT_SHAPE = R.INT_SHAPE  # C, H, W = 2, 5, 103: 515 points = 3 tiles, the last with 3 valid threads
INT_M = (1, 2, 3, 8, 24, 50, 64, 65, 100, 129, 1024)
INT_W = (0.5, 1.0, 1.5, 1.25, 0.75)


@functools.lru_cache(maxsize=None)
def integer_case(M):
    C, H, W = INT_SHAPE
    P = H * W
    g = gen(R._seed(M, 71))
    a = max(M - 1, 1)
    K = min(M // 2, max(1, 2700 // a))  # non-zero e_i: at most 2 K per point
    e = torch.zeros(C, P, M, dtype=torch.int64)
    for c in range(C):
        r = integer_rows(M, P, R._seed(M, 72 + c))
        anti = (r - r.flip(1)).clamp(-1, 1)  # antisymmetric about the middle: the sum is zero
        keep = torch.zeros(M, dtype=torch.bool)
        keep[:K] = keep[M - K:] = True
        e[c] = torch.where(keep, anti, torch.zeros_like(anti))[:, torch.randperm(M, generator=g)]
    centre = torch.randint(-8, 9, (C, P), generator=g)
    x = centre.unsqueeze(-1) + a * e  # (C, P, M)
    delta = torch.tensor([0, 0, 1, -1, 2, -2])[torch.randint(0, 6, (C, P), generator=g)]
    if a <= 8:  # small spread: the truth also ties a displaced member or lies beyond them all
        big = torch.tensor([a, -a, 2 * a, -2 * a])[torch.randint(0, 4, (C, P), generator=g)]
        delta = torch.where(torch.rand(C, P, generator=g) < 0.4, big, delta)
    t = centre + delta
    return dict(x=x.permute(2, 0, 1).reshape(M, C, H, W).float(), t=t.reshape(C, H, W).float(), w=torch.tensor(INT_W))


# b. ties and ends: five points whose rank bins are written out by hand
def ties_case(M):
    """(x (M, 1, 1, 5), t (1, 1, 5), the five bins): truth below all members, above all, equal to 1, to 2 and to all M members (M >= 4)"""
    up = torch.arange(1, M + 1).float()
    two = up.clone()
    two[2] = 2.0  # 1, 2, 2, 4, ...
    x = torch.stack([up, up, up, two, torch.full((M,), 7.0)], dim=1).reshape(M, 1, 1, 5)
    t = torch.tensor([0.0, M + 1.0, 3.0, 2.0, 7.0]).reshape(1, 1, 5)
    return x, t, [0, M, 2, 2, M // 2]


# c. physical scale (score_edge_refs.physical_case), d. the finish loop (finish_case), e. the NaN table (nan_table_case), f. guard bands
PHYS_M = (8, 50, 64, 100)
physical_case, finish_case, nan_table_case = R.physical_case, R.finish_case, R.nan_table_case
FINISH_SHAPES, FINISH_M, NAN_M = R.FINISH_SHAPES, R.FINISH_M, R.NAN_M


def finish_nan_case(H, W):
    """the finish case with one NaN member in the last thread of the last record"""
    c = dict(finish_case(H, W))
    c["x"] = c["x"].clone()
    c["x"][1, 0, H - 1, W - 1] = float("nan")
    return c
