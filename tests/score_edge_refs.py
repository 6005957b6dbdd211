"""float64 oracle, DERIVED per-point and grid-mean bounds, an fp32 restatement (with planted defects) and the shared case tables of the
scoring kernel edge tests (csrc/scoring.hip: ldc_ensemble_scores, ldc_rollout_scores, ldc_validation_scores).
tests/test_gpu_score_edges.py runs the kernels; tests/test_score_edge_bounds_cpu.py proves on the CPU that every bound admits a correct
fp32 implementation (the kernel's order and the reference's own torch order) and rejects the planted defects.

The oracle restates oracle/scoring.py (evaluate/utils.py, evaluate_ens_gpu.py:339-425) and tests/validation_oracle.py (train_AR.py:281-312)
in float64, per point and per (channel, lead time).  It starts from the fp32 bits the kernel sees: where the inverse normalisation is
fused into the load, `inv_norm_f32` applies (v / target_std) * std + mean in fp32, every operation rounded on its own, exactly as
ldc_chan_affine(inverse=1) does - the kernel promises those bits - and only then widens.

Every bound is `n * 2**-24 * S` (redzone.elementwise_bound; first order in 2**-24 as in tests/mfma_edge_refs.py), S the float64 sum of the
absolute terms, n counted from the arithmetic of score_point / finish_point.  Nothing is fitted to what a kernel returns.

Per point, M members x_i, truth t, climatology c (U = 2**-24, b_q = the bound of q):
  mean    sum / M: M - 1 additions, one division                         n = M      on sum |x_i| / M
  skill   M subtractions (one per term), M additions, one division       n = M + 2  on sum |t - x_i| / M
  spread  the sort only selects; M products (one per term), M additions, the scale 2 ws / (M (M - 1)): 2 ws and M (M - 1) are exact,
          one division                                                   n = M + 2  on 2 / (M (M - 1)) sum |x_(i)| |2 i - M - 1|
  se      d = mean - t: b_d = b_mean + U |d|;  d * d: 2 |d| b_d + b_d^2 + U (|d| + b_d)^2   (b_d^2 is kept: at physical scale b_d is
          not small against d)
  single  d_i = x_i - t (1, relative: 2 on d_i^2), the product (1), M additions, one division     n = M + 4  on sum d_i^2 / M
  crps    skill - spread / 2: b_skill + b_spread / 2 + U (|skill| + |spread| / 2).  The last term is U |crps| for the kernel, which
          subtracts first and weights afterwards; the reference weights skill and spread first (one rounding on each product) and
          subtracts then - the bound is written to admit either order.
  ACC     fa = mean - c: b_fa = b_mean + U |fa|;  ta = t - c: b_ta = U |ta|;  the products fa ta, fa^2, ta^2 as se above.
  Every reduced quantity is multiplied by the latitude weight first: b w + U |q w|.
Grid mean over P points in nblk = ceil(P / 256) workgroups: the weighted point bounds, plus on sum |q w|: 6 (butterfly within a wave)
  + 2 (the 4 wave totals, added pairwise) + ceil(nblk / 64) (records per lane in the finish) + 6 (one more butterfly) + 1 (the
  division by the count).
ACC = n4 / sqrt(n5 n6) from three such means: the interval (|n4| + b4) / sqrt((n5 - b5) (n6 - b6)) - |acc| (1 / sqrt is convex: the
  upper deviation is the larger one) plus 4 U for the product, the square root and the division; no claim (inf) where n5 <= b5 or n6 <= b6.
Values the reference makes NaN or inf carry no bound: their pattern (and the sign of an inf) must match.
"""
from __future__ import annotations

import functools

import torch

from oracle import scoring as S
from tests.redzone import U, elementwise_bound, worst_ratio

TPB = 256
KEYS = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
VKEYS = ("ens_mse", "single_mse", "crps")
FLT_MAX_BITS = 0x7F7FFFFF  # the largest finite fp32: the poison of guarded INPUTS (NaN is a legal input of these kernels)
ARMS = ((8, 8), (16, 16), (32, 24), (32, 32), (64, 40), (64, 48), (64, 56), (64, 64))  # ldc_dispatch_sort_arm (csrc/ensemble_common.h)


def sort_arm(M):
    """(NP, NUSE) that ldc_dispatch_sort_arm (csrc/ensemble_common.h) picks for M members"""
    return next(a for a in ARMS if M <= a[1])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _seed(*k):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31)


def cos_weights(H):
    return S.get_normalized_lat_weights_based_on_cos(torch.linspace(-89.0, 89.0, H))


def inv_norm_f32(v, mean, std, target_std):
    """(v / target_std) * std[c] + mean[c] in fp32, each operation rounded on its own (ldc_chan_affine inverse=1); v (M, C, ...)"""
    shape = (1, -1) + (1,) * (v.dim() - 2)
    q = v.float() if float(target_std) == 1.0 else v.float() / torch.tensor(float(target_std), dtype=torch.float32)
    return q * std.float().view(shape) + mean.float().view(shape)


# ---- float64 oracle with bounds ----------------------------------------------------------------------------------------------------
def point_ref(x, t, cl=None):
    """x (M, ...) the fp32 values the kernel scores, t (...), cl (...) | None -> {name: (float64 value, bound)} per point, for
    mean, skill, spread, crps, se, single and (with cl) fta, ffa, tta; NaN / inf follow the reference's elementwise rules"""
    x, t = x.double(), t.double()
    M = x.shape[0]
    out = {}
    mean = x.sum(0) / M
    b_mean = elementwise_bound(x.abs().sum(0) / M, M)
    out["mean"] = (mean, b_mean)
    skill = (t.unsqueeze(0) - x).abs().sum(0) / M
    b_skill = elementwise_bound(skill, M + 2)
    out["skill"] = (skill, b_skill)
    if M >= 2:
        xs = torch.sort(x, dim=0).values  # NaN sorts last and makes the weighted sum NaN, as in the reference
        wt = (2.0 * torch.arange(1, M + 1, dtype=torch.float64) - M - 1).view((-1,) + (1,) * (x.dim() - 1))
        spread = 2.0 * (xs * wt).sum(0) / (M * (M - 1))
        b_spread = elementwise_bound(2.0 * (xs.abs() * wt.abs()).sum(0) / (M * (M - 1)), M + 2)
    else:  # the reference returns zeros for one member, NaN or not
        spread, b_spread = torch.zeros_like(t), torch.zeros_like(t)
    out["spread"] = (spread, b_spread)
    out["crps"] = (skill - 0.5 * spread, b_skill + 0.5 * b_spread + U * (skill.abs() + 0.5 * spread.abs()))

    def square(a, b_a, c=None, b_c=None):
        c, b_c = (a, b_a) if c is None else (c, b_c)
        return a * c, c.abs() * b_a + a.abs() * b_c + b_a * b_c + U * (a.abs() + b_a) * (c.abs() + b_c)

    d = mean - t
    out["se"] = square(d, b_mean + U * d.abs())
    single = ((x - t.unsqueeze(0)) ** 2).sum(0) / M
    out["single"] = (single, elementwise_bound(single, M + 4))
    if cl is not None:
        cl = cl.double()
        fa, ta = mean - cl, t - cl
        b_fa, b_ta = b_mean + U * fa.abs(), U * ta.abs()
        out["fta"], out["ffa"], out["tta"] = square(fa, b_fa, ta, b_ta), square(fa, b_fa), square(ta, b_ta)
    return out


def n_reduce(P):
    """roundings of one grid mean over P points on top of the weighted point values (module docstring)"""
    nblk = -(-P // TPB)
    return 6 + 2 + -(-nblk // 64) + 6 + 1


def grid_mean(q, bq, nanmean):
    """q, bq (C, P) weighted point values and bounds, nanmean (C,) bool -> (value, bound) (C,): the reference's mean (one NaN point ->
    NaN) or nanmean (over the points that are not NaN; none -> NaN)"""
    C, P = q.shape
    valid = ~torch.isnan(q)
    cnt = valid.sum(-1).double()
    qz = torch.where(valid, q, torch.zeros_like(q))
    s, sabs, sb = qz.sum(-1), qz.abs().sum(-1), torch.where(valid, bq, torch.zeros_like(bq)).sum(-1)
    nan = torch.full_like(s, float("nan"))
    ok = torch.where(nanmean, cnt > 0, cnt == P)
    den = cnt.clamp_min(1.0)
    return torch.where(ok, s / den, nan), torch.where(ok, (sb + n_reduce(P) * U * sabs) / den, nan)


def acc_from(n4, b4, n5, b5, n6, b6):
    acc = n4 / torch.sqrt(n5 * n6)
    lo5, lo6 = n5 - b5, n6 - b6
    ok = (lo5 > 0) & (lo6 > 0)
    hi = (n4.abs() + b4) / torch.sqrt(torch.where(ok, lo5 * lo6, torch.ones_like(lo5)))
    return acc, torch.where(ok, (hi - acc.abs()) + 4 * U * hi, torch.full_like(hi, float("inf")))


def scores_ref(x, t, cl, w, nan_channel=-1):
    """x (M, C, H, W) the fp32 values the kernel scores, t / cl (C, H, W) (cl None: no ACC), w (H,) -> dict
      maps:       skill, spread -> (value, bound) (C, H, W)
      scores:     KEYS -> (value, bound) (C,), channel `nan_channel` by nanmean, ACC always by three independent nanmeans
      validation: VKEYS -> (value, bound) (C,), plain means"""
    pt = point_ref(x, t, cl)
    C, H, W = t.shape
    P = H * W
    wp = w.double().view(1, H, 1).expand(C, H, W)
    nm = torch.zeros(C, dtype=torch.bool)
    if nan_channel >= 0:
        nm[nan_channel] = True
    plain, every = torch.zeros(C, dtype=torch.bool), torch.ones(C, dtype=torch.bool)

    def weighted(name):
        v, b = pt[name]
        return (v * wp).reshape(C, P), (b * wp + U * (v * wp).abs()).reshape(C, P)

    names = {"ens_mse": "se", "crps_spread": "spread", "crps_skill": "skill", "crps": "crps", "single_mse": "single"}
    scores = {k: grid_mean(*weighted(names[k]), nm) for k in KEYS[1:]}
    if cl is not None:
        scores["ens_acc"] = acc_from(*grid_mean(*weighted("fta"), every), *grid_mean(*weighted("ffa"), every), *grid_mean(*weighted("tta"), every))
    else:
        scores["ens_acc"] = (torch.full((C,), float("nan"), dtype=torch.float64),) * 2
    validation = {k: grid_mean(*weighted(names[k]), plain) for k in VKEYS}
    return dict(maps={k: pt[k] for k in ("skill", "spread")}, scores=scores, validation=validation)


def ratio_of(got, want, bound):
    """worst |got - want| / bound over the elements whose oracle value is finite; inf when the NaN / inf pattern differs"""
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(want.shape).reshape(-1)
    got, want = torch.as_tensor(got).detach().cpu().double().reshape(-1), want.double().reshape(-1)
    if got.shape != want.shape or not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float("inf")
    inf = torch.isinf(want)
    if not torch.equal(got[inf], want[inf]):
        return float("inf")
    fin = torch.isfinite(want)
    if not bool(fin.any()):
        return 0.0
    return worst_ratio(got[fin], want[fin], bound[fin])[0]


def judge(got, ref, what=""):
    """got against ref = (float64 value, bound): the NaN / inf pattern equal, every finite value within its bound; returns the worst ratio"""
    want, bound = ref
    got = torch.as_tensor(got).detach().cpu().double().reshape(want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{what}: NaN pattern differs: got {got.reshape(-1)[:8].tolist()}, want {want.reshape(-1)[:8].tolist()}"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: inf pattern differs: got {got[inf][:8].tolist()}, want {want[inf][:8].tolist()}"
    r = ratio_of(got, want, bound)
    if not r <= 1.0:
        fin = torch.isfinite(want)
        rr = torch.where(fin, (got - want).abs() / bound.clamp_min(1e-300), torch.zeros_like(want)).reshape(-1)
        i = int(torch.nan_to_num(rr, nan=float("inf")).argmax())
        raise AssertionError(f"{what}: element {i}: got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r}, "
                             f"bound {float(bound.reshape(-1)[i]):.3e}, ratio {r:.3g}")
    return r


def same_bits(a, b):
    a, b = torch.as_tensor(a).detach().cpu().float().contiguous(), torch.as_tensor(b).detach().cpu().float().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def same_value_bits(a, b):
    """equal bits, any NaN equal to any NaN (the kernels write one NaN pattern, torch another)"""
    a, b = torch.as_tensor(a).detach().cpu().float(), torch.as_tensor(b).detach().cpu().float()
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and same_bits(torch.nan_to_num(a), torch.nan_to_num(b))


# ---- the reference's own torch arithmetic in fp32 -----------------------------------------------------------------------------------
def oracle_f32(x, t, cl, w, nan_channel=-1):
    """oracle/scoring.py and tests/validation_oracle.py run in fp32 on the same values -> maps / scores / validation as scores_ref, values only"""
    from tests import validation_oracle as VO

    x, t, w = x.float(), t.float(), w.float()
    C = t.shape[0]
    clf = torch.zeros_like(t) if cl is None else cl.float()
    if nan_channel >= 0:
        sc = S.ensemble_scores(x, t, clf, w, sst_channel=nan_channel)
    else:  # no nanmean channel: the reference's nanmean goes to a copy of channel 0 appended behind the others
        sc = S.ensemble_scores(torch.cat([x, x[:, :1]], 1), torch.cat([t, t[:1]]), torch.cat([clf, clf[:1]]), w, sst_channel=C)
        sc = {k: v[:C] for k, v in sc.items()}
    if cl is None:
        sc["ens_acc"] = torch.full((C,), float("nan"))
    va = VO.validation_scores(x.unsqueeze(2), t.unsqueeze(1), w)
    return dict(maps=dict(skill=S.pointwise_crps_skill(x, t.unsqueeze(0), 0), spread=S.pointwise_crps_spread(x, 0)), scores=sc,
                validation={k: va[k][:, 0] for k in VKEYS})


# ---- the kernel's arithmetic in fp32 torch, with planted defects ------------------------------------------------------------------------
DEFECTS = ("swap", "short", "MM", "weight", "record_twice", "point_HW")


def _butterfly(v):
    """__shfl_xor butterfly over the last axis (64 lanes): every lane ends with the same total"""
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def kernel_f32(x, t, cl, w, nan_channel=-1, *, fma=True, defect=None):
    """score_point + finish_point restated in fp32 torch: member-order sums, sorted weighted sum, 256-point workgroups (butterfly per
    wave, the 4 wave totals pairwise), the finish (records b, b + 64, ... per lane, butterfly, the count rules).  `fma`: the multiply-adds
    that the compiler may contract (ws += x w, single += d d) are fused (product exact, one rounding) or not.  -> maps / scores / validation
    as scores_ref, fp32 values only.  Planted defects:
      swap: one adjacent pair of sorted members exchanged at every point p % 64 == 5;  short: the last group of 8 registers is left out of
      the sort (NUSE one group short);  MM: M * M in place of M * (M - 1);  weight: 2 (i + 1) - M - 1 in place of 2 i - M - 1;
      record_twice: workgroup record 1 (0 if there is one) added twice in the finish;  point_HW: the point one past the plane (the next
      channel's first) included."""
    assert defect in (None,) + DEFECTS
    x, t, w = x.float(), t.float(), w.float()
    M, C, H, W = x.shape
    P = H * W
    x, t = x.reshape(M, C, P), t.reshape(C, P)
    c_ = None if cl is None else cl.float().reshape(C, P)
    wp = w.view(1, H, 1).expand(C, H, W).reshape(C, P)
    if defect == "point_HW":
        nxt = [(c + 1) % C for c in range(C)]
        x, t, wp = torch.cat([x, x[:, nxt, :1]], -1), torch.cat([t, t[nxt, :1]], -1), torch.cat([wp, wp[:, -1:]], -1)
        c_ = None if c_ is None else torch.cat([c_, c_[nxt, :1]], -1)
    Pk = x.shape[-1]
    Mf = torch.tensor(float(M))

    def mad(a, b, acc):
        return (a.double() * b.double() + acc.double()).float() if fma else a * b + acc

    s, skill, single = torch.zeros(C, Pk), torch.zeros(C, Pk), torch.zeros(C, Pk)
    for i in range(M):
        s = s + x[i]
        skill = skill + (t - x[i]).abs()
        d = x[i] - t
        single = mad(d, d, single)
    skill, single = skill / Mf, single / Mf
    nan_m = torch.isnan(x).any(0)
    spread = torch.zeros(C, Pk)
    if M >= 2:
        NP, NUSE = sort_arm(M)
        reg = torch.full((NP, C, Pk), float("inf"))
        reg[:M] = torch.nan_to_num(x, nan=float("inf"))  # (fminf / fmaxf drop a NaN; such points are made NaN below)
        if defect == "short":
            reg[: NUSE - 8] = torch.sort(reg[: NUSE - 8], dim=0).values
        else:
            reg = torch.sort(reg, dim=0).values
        if defect == "swap":
            j = M // 2 - 1
            hit = torch.arange(Pk) % 64 == 5
            a, b = reg[j].clone(), reg[j + 1].clone()
            reg[j], reg[j + 1] = torch.where(hit, b, a), torch.where(hit, a, b)
        ws = torch.zeros(C, Pk)
        for i in range(M):
            k = i + 2 if defect == "weight" else i + 1
            ws = mad(reg[i], torch.tensor(2.0 * k - M - 1.0), ws)
        spread = 2.0 * ws / (Mf * Mf if defect == "MM" else Mf * (Mf - 1.0))
        spread = torch.where(nan_m, torch.full_like(spread, float("nan")), spread)
    mean = s / Mf
    se = (mean - t) * (mean - t)
    crps = skill - 0.5 * spread
    q = {"crps_skill": skill, "crps_spread": spread, "crps": crps, "ens_mse": se, "single_mse": single}
    if c_ is not None:
        fa, ta = mean - c_, t - c_
        q.update(fta=fa * ta * wp, ffa=fa * fa * wp, tta=ta * ta * wp)
    nblk = -(-Pk // TPB)

    def reduce(v):
        """(C, Pk) -> (C,): workgroup records, then the finish"""
        pad = torch.zeros(C, nblk * TPB)
        pad[:, :Pk] = v
        waves = _butterfly(pad.reshape(C, nblk, 4, 64))
        rec = (waves[..., 0] + waves[..., 1]) + (waves[..., 2] + waves[..., 3])  # (C, nblk)
        lanes = torch.zeros(C, 64)
        rp = torch.zeros(C, -(-nblk // 64) * 64)
        rp[:, :nblk] = rec
        for k in range(rp.shape[1] // 64):
            lanes = lanes + rp[:, k * 64:(k + 1) * 64]
        if defect == "record_twice":
            r = 1 if nblk > 1 else 0
            lanes[:, r % 64] = lanes[:, r % 64] + rec[:, r]
        return _butterfly(lanes)

    total = float(Pk)
    nanv = float("nan")

    def avg(v, weighted, nanmean):
        """the count rules of finish_point for one reduced quantity"""
        val = v if weighted else v * wp
        valid = ~torch.isnan(v)
        tot, cnt = reduce(torch.where(valid, val, torch.zeros_like(val))), valid.sum(-1).float()
        out = torch.full((C,), nanv)
        for c in range(C):
            if (nanmean[c] and cnt[c] > 0) or (not nanmean[c] and cnt[c] == total):
                out[c] = tot[c] / cnt[c]
        return out

    nm = [c == nan_channel for c in range(C)]
    scores = {k: avg(q[k], False, nm) for k in KEYS[1:]}
    if c_ is not None:
        n4, n5, n6 = (avg(q[k], True, [True] * C) for k in ("fta", "ffa", "tta"))
        scores["ens_acc"] = n4 / torch.sqrt(n5 * n6)
    else:
        scores["ens_acc"] = torch.full((C,), nanv)
    validation = {k: avg(q[k], False, [False] * C) for k in VKEYS}
    return dict(maps=dict(skill=skill[:, :P].reshape(C, H, W), spread=spread[:, :P].reshape(C, H, W)), scores=scores, validation=validation)


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# a. every M, small integers: every sum of a point is exact, the maps are the float64 value rounded once
INT_SHAPE = (2, 5, 103)  # C, H, W: 515 points = 3 workgroups, the last with 3 valid threads
ALL_M = tuple(range(1, 65))
POW2_NORM = dict(mean=(8.0, -16.0), std=(4.0, 2.0), target_std=0.5)  # (v / 0.5) * std + mean: exact on small integers


def integer_rows(M, n, seed):
    """(n, M) int64 rows, shuffled: ascending, descending, every rotation, all equal, two-valued 0/1 (sorted, reversed, alternating, random),
    three-valued ties, seeded random permutations"""
    g = gen(seed)
    base = torch.arange(M) - M // 2
    rows = [base, base.flip(0)] + [base.roll(k) for k in range(1, M)] + [torch.full((M,), 3)]
    if M >= 2:
        for k in sorted({1, M // 2, M - 1}):
            r = (torch.arange(M) >= k).long()
            rows += [r, r.flip(0)]
        rows.append(torch.arange(M) % 2)
    three = torch.tensor([-2, 0, 5])
    while len(rows) < n:
        kind = len(rows) % 3
        if kind == 0:
            rows.append((torch.rand(M, generator=g) < 0.5).long())
        elif kind == 1:
            rows.append(three[torch.randint(0, 3, (M,), generator=g)])
        else:
            rows.append(base[torch.randperm(M, generator=g)])
    rows = torch.stack(rows[:n])
    return rows[torch.randperm(n, generator=g)]


@functools.lru_cache(maxsize=None)
def integer_case(M):
    """x (M, C, H, W), t, cl (C, H, W) fp32 holding small integers (|x| <= 103: sum |x| |2 i - M - 1| and 2 ws stay below 2**24), w (H,)"""
    C, H, W = INT_SHAPE
    P = H * W
    g = gen(_seed(M, 53))
    ch0 = integer_rows(M, P, _seed(M, 54))
    ch1 = integer_rows(M, P, _seed(M, 55)) * 3 - 7
    x = torch.stack([ch0.T, ch1.T], 1).reshape(M, C, H, W).float()
    t = torch.randint(-8, 9, (C, H, W), generator=g).float()
    cl = torch.randint(-3, 4, (C, H, W), generator=g).float()
    return dict(x=x, t=t, cl=cl, w=cos_weights(H))


# b. physical scale: (channel, centre, field std, ensemble std)
PHYS = (("z50", 2e5, 5e3, 1e2), ("z500", 5.4e4, 3e3, 60.0), ("mslp", 101325.0, 1200.0, 150.0), ("t2m", 280.0, 15.0, 1.0), ("q700", 2e-3, 1e-3, 3e-4),
        ("unit", 0.5, 1.0, 2.0))
PHYS_M = (8, 24, 50, 64)
PHYS_HW = (33, 17)
PHYS_TARGET_STD = 0.5


@functools.lru_cache(maxsize=None)
def physical_case(M, L=2):
    """members = field + ensemble noise, truth one more draw, climatology the field; stored normalised (v) and de-normalised in fp32 as
    the fused load does (x: the bits the kernels score).  v, x (M, C, L, H, W); t, cl (C, L, H, W)"""
    H, W = PHYS_HW
    C = len(PHYS)
    g = gen(_seed(M, 57))
    col = lambda i: torch.tensor([p[i] for p in PHYS], dtype=torch.float64).view(C, 1, 1, 1)  # noqa: E731
    centre, fstd, estd = col(1), col(2), col(3)
    field = centre + fstd * torch.randn(C, L, H, W, generator=g, dtype=torch.float64)
    members = field + estd * torch.randn(M, C, L, H, W, generator=g, dtype=torch.float64)
    truth = field + estd * torch.randn(C, L, H, W, generator=g, dtype=torch.float64)
    mean, std = centre.reshape(C).float(), fstd.reshape(C).float()
    v = ((members - centre) / fstd * PHYS_TARGET_STD).float()
    return dict(v=v, x=inv_norm_f32(v, mean, std, PHYS_TARGET_STD), t=truth.float(), cl=field.float(), w=cos_weights(H), mean=mean, std=std,
                target_std=PHYS_TARGET_STD)


# c. the finish loop: (H, W) -> workgroup records per plane
FINISH_SHAPES = ((129, 128), (129, 256))  # 65 and 129 records: 2 and 3 per lane in the finish
FINISH_M = 3


@functools.lru_cache(maxsize=None)
def finish_case(H, W):
    g = gen(_seed(H, W, 59))
    x = torch.randn(FINISH_M, 1, H, W, generator=g) * 2 + 0.5
    return dict(x=x, t=torch.randn(1, H, W, generator=g), cl=torch.randn(1, H, W, generator=g) * 0.3, w=cos_weights(H))


# d. guard bands: (M, C, L, H, W, nan_channel); slots into a 7-entry truth and a 4-entry climatology table (three lead times: neither
# identity nor monotone; two lead times can only be 'not increasing')
GUARD_CASES = ((5, 3, 3, 6, 8, 1), (9, 2, 2, 33, 17, 0))
GUARD_SLOTS = {3: ([5, 0, 5], [3, 3, 1]), 2: ([5, 0], [3, 1])}
N_TRUTH, N_CLIM = 7, 4


@functools.lru_cache(maxsize=None)
def guard_case(M, C, L, H, W, sst):
    """x (M, C, L, H, W), truth table (7, C, H, W), climatology table (4, C, H, W), 30 % land NaNs in channel `sst` (members and every truth entry)"""
    g = gen(_seed(M, C, L, H, W, 61))
    x = torch.randn(M, C, L, H, W, generator=g) * 2 + 0.5
    tt, ct = torch.randn(N_TRUTH, C, H, W, generator=g), torch.randn(N_CLIM, C, H, W, generator=g) * 0.3
    land = torch.rand(H, W, generator=g) < 0.3
    x[:, sst][:, :, land] = float("nan")
    tt[:, sst][:, land] = float("nan")
    ts, cs = GUARD_SLOTS[L]
    return dict(x=x, truth_table=tt, clim_table=ct, w=cos_weights(H), t_slots=ts, c_slots=cs)


# e. NaN / inf table: 64 points, M = 5.  Channel 0: the NaN patterns only (its nanmean scores stay finite); channel 1: all patterns;
# channel 2: NaN in every member of every point; channel 3: clean
NAN_M, NAN_HW = 5, (4, 16)
PATTERNS = ("clean", "NaN in one member", "NaN in all members", "NaN in truth", "NaN in climatology only", "+inf in one member",
            "-inf in one member", "+inf in truth")


@functools.lru_cache(maxsize=None)
def nan_table_case(M=NAN_M):
    H, W = NAN_HW
    C = 4
    g = gen(_seed(M, 63))
    x = torch.randn(M, C, H, W, generator=g) * 2 + 0.5
    t, cl = torch.randn(C, H, W, generator=g), torch.randn(C, H, W, generator=g) * 0.3
    nan, inf = float("nan"), float("inf")
    kind = torch.zeros(C, H * W, dtype=torch.long)
    kind[0], kind[1] = torch.arange(H * W) % 5, torch.arange(H * W) % 8
    xf, tf, cf = x.reshape(M, C, -1), t.reshape(C, -1), cl.reshape(C, -1)
    for c in (0, 1):
        for p in range(H * W):
            k, m = int(kind[c, p]), p % M
            if k == 1:
                xf[m, c, p] = nan
            elif k == 2:
                xf[:, c, p] = nan
            elif k == 3:
                tf[c, p] = nan
            elif k == 4:
                cf[c, p] = nan
            elif k == 5:
                xf[m, c, p] = inf
            elif k == 6:
                xf[m, c, p] = -inf
            elif k == 7:
                tf[c, p] = inf
    xf[:, 2] = nan
    return dict(x=x, t=t, cl=cl, w=cos_weights(H), kind=kind)


def relative_errors(got, want):
    """max |got - want| / |want| over the finite, non-zero oracle values (for the record, not a check)"""
    got, want = torch.as_tensor(got).detach().cpu().double().reshape(-1), want.double().reshape(-1)
    m = torch.isfinite(want) & (want != 0) & torch.isfinite(got)
    return float(((got[m] - want[m]).abs() / want[m].abs()).max()) if bool(m.any()) else 0.0

