"""float64 oracle, COUNTED bounds, a brute-force loop, an fp32 restatement (with planted defects) and the case tables of the regional
score kernel (csrc/regional.hip: ldc_rollout_regional).  tests/test_gpu_regional.py runs the kernel; tests/test_regional_cpu.py proves on
the CPU that every bound admits a correct fp32 implementation in the kernel's order and that every planted defect is caught.

Definitions, per point p of region r (bit r of mask[p]), members x_i in member order, truth t, weight w = the
latitude weight of p's row, climatology a; valid: no member and not t is NaN; ACC-valid: valid and a is not NaN:
    mean = sum_i x_i / M, e = mean - t, se = e^2, var = sum_i (x_i - mean)^2 / (M - 1) (0 at M == 1), skill = sum_i |t - x_i| / M,
    spread = 2 / (M (M - 1)) sum_i (2 i - M - 1) x_(i) (0 at M == 1), fa = mean - a, ta = t - a
    sums[r] = sum over valid points of w, w e, w se, w var, w skill, w spread; over ACC-valid points of w, w fa ta, w fa^2, w ta^2
    counts[r] = valid, invalid, ACC-valid points
Bounds, first order in U = 2**-24 (redzone.elementwise_bound), counted from the kernel's arithmetic, nothing fitted:
    mean, se, skill, fa ta, fa^2, ta^2   the counting of tests/score_edge_refs.py (point_ref): the same fp32 operations
    e = mean - t                          b_mean + U |e|
    var                                   the counting of tests/reliability_refs.py (point_ref)
    spread                                one bound per member count: M products and M - 1 additions (a term passes one product and at
                                          most M - 1 additions; fused or not), one division: (M + 1) U on 2 / (M (M - 1)) sum |x_(i)| |2 i - M - 1|
    every term of a sum is double(w) * double(v): exact.  A sum of n terms in a workgroup's records and nrec records is n + nrec fp64
    additions: (n + nrec) 2**-53 sum |w v| on top of sum w b_v.  sum w itself carries that part only.
counts are compared by value.  Values the definitions make NaN or inf carry no bound: their pattern (and the sign of an inf) must match."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import reliability_refs as REL
from tests import score_edge_refs as SE
from tests.redzone import U
from tests.score_edge_refs import cos_weights, gen, guard_case, inv_norm_f32  # noqa: F401  (shared, not copied)

TPB, TPW, MAX_R, MAX_M = 256, 8, 32, 64
NS, NC = 10, 3
U53 = 2.0 ** -53
REC_BYTES = MAX_R * (NS * 8 + 4 * 4)
GUARD_CASES, GUARD_SLOTS, N_TRUTH, N_CLIM = SE.GUARD_CASES, SE.GUARD_SLOTS, SE.N_TRUTH, SE.N_CLIM
FLT_MAX_BITS = SE.FLT_MAX_BITS


def n_records(P):
    return -(-(-(-P // TPB)) // TPW)


def workspace_bytes(C, L, P):
    return L * C * n_records(P) * REC_BYTES


def region_bits(mask, R):
    """mask (H, W) integer words -> bool (R, H * W)"""
    m = torch.as_tensor(np.asarray(mask).astype(np.int64) & 0xFFFFFFFF).reshape(-1)
    return torch.stack([((m >> r) & 1).bool() for r in range(R)])


# ---- float64 oracle with bounds ----------------------------------------------------------------------------------------------------
def point_values(x, t, cl=None):
    """x (M, C, H, W) the fp32 values the kernel scores, t (C, H, W), cl (C, H, W) | None -> ((C, P) float64 value, bound) for the nine
    point values behind sums 1 .. 5 and 7 .. 9, by name, and the validity masks"""
    M, C = x.shape[0], x.shape[1]
    flat = lambda a: a.reshape(*a.shape[:-2], -1)  # noqa: E731
    x, t = flat(x), flat(t)
    cl = None if cl is None else flat(cl)
    pt = SE.point_ref(x, t, cl)
    mean, b_mean = pt["mean"]
    e = mean - t.double()
    out = dict(e=(e, b_mean + U * e.abs()), se=pt["se"], skill=pt["skill"])
    if M >= 2:
        out["var"] = REL.point_ref(x, t)["var"]
        xs = torch.sort(x.double(), dim=0).values
        wt = (2.0 * torch.arange(1, M + 1, dtype=torch.float64) - M - 1).view(-1, 1, 1)
        scale = 2.0 / (M * (M - 1))
        out["spread"] = (scale * (xs * wt).sum(0), (M + 1) * U * scale * (xs.abs() * wt.abs()).sum(0))
    else:
        zero = torch.zeros(C, x.shape[-1], dtype=torch.float64)
        out["var"], out["spread"] = (zero, zero), (zero, zero)
    valid = ~torch.isnan(x).any(0) & ~torch.isnan(t)
    acc_valid = torch.zeros_like(valid)
    if cl is not None:
        out.update(fta=pt["fta"], ffa=pt["ffa"], tta=pt["tta"])
        acc_valid = valid & ~torch.isnan(cl)
    return out, valid, acc_valid


SUM_OF = ("one", "e", "se", "var", "skill", "spread", "one", "fta", "ffa", "tta")


def regional_ref(x, t, w, mask, R, cl=None):
    """-> dict: sums (value, bound) (R, C, 10) float64, counts (R, C, 3) int64"""
    M, C, H, W = x.shape
    P = H * W
    pv, valid, acc_valid = point_values(x, t, cl)
    wp = w.double().reshape(H, 1).expand(H, W).reshape(P)
    bits = region_bits(mask, R)
    nrec = n_records(P)
    sums, bnd = torch.zeros(R, C, NS, dtype=torch.float64), torch.zeros(R, C, NS, dtype=torch.float64)
    counts = torch.zeros(R, C, NC, dtype=torch.int64)
    one = (torch.ones(C, P, dtype=torch.float64), torch.zeros(C, P, dtype=torch.float64))
    for r in range(R):
        for c in range(C):
            sel_v, sel_a = bits[r] & valid[c], bits[r] & acc_valid[c]
            counts[r, c] = torch.tensor([int(sel_v.sum()), int((bits[r] & ~valid[c]).sum()), int(sel_a.sum())])
            for k, name in enumerate(SUM_OF):
                if k >= 6 and cl is None:
                    continue
                sel = sel_v if k < 6 else sel_a
                v, b = one if name == "one" else pv[name]
                terms = wp[sel] * v[c][sel]
                sums[r, c, k] = terms.sum()
                bnd[r, c, k] = (wp[sel] * b[c][sel]).sum() + (int(sel.sum()) + nrec) * U53 * terms.abs().sum()
    return dict(sums=(sums, bnd), counts=counts)


def brute_force(x, t, w, mask, R, cl=None):
    """the definitions as a Python loop over points (float64 on the fp32 values; tiny cases only) -> sums (R, C, 10), counts (R, C, 3)"""
    import math

    M, C, H, W = x.shape
    m = np.asarray(mask).astype(np.int64).reshape(-1) & 0xFFFFFFFF
    sums, counts = torch.zeros(R, C, NS, dtype=torch.float64), torch.zeros(R, C, NC, dtype=torch.int64)
    for c in range(C):
        for p in range(H * W):
            i, j = divmod(p, W)
            if not any((int(m[p]) >> r) & 1 for r in range(R)):
                continue
            xs = [float(x[k, c, i, j]) for k in range(M)]
            tt, ww = float(t[c, i, j]), float(w[i])
            a = None if cl is None else float(cl[c, i, j])
            valid = not any(math.isnan(v) for v in xs) and not math.isnan(tt)
            acc_valid = valid and a is not None and not math.isnan(a)
            vals = None
            if valid:
                mean = sum(xs) / M
                var = sum((v - mean) ** 2 for v in xs) / (M - 1) if M > 1 else 0.0
                skill = sum(abs(tt - v) for v in xs) / M
                srt = sorted(xs)
                spread = 2.0 / (M * (M - 1)) * sum((2 * (k + 1) - M - 1) * v for k, v in enumerate(srt)) if M > 1 else 0.0
                e = mean - tt
                vals = [1.0, e, e * e, var, skill, spread]
                if acc_valid:
                    fa, ta = mean - a, tt - a
                    vals += [1.0, fa * ta, fa * fa, ta * ta]
            for r in range(R):
                if not (int(m[p]) >> r) & 1:
                    continue
                counts[r, c, 0] += int(valid)
                counts[r, c, 1] += int(not valid)
                counts[r, c, 2] += int(acc_valid)
                if vals:
                    for k, v in enumerate(vals):
                        sums[r, c, k] += ww * v
    return dict(sums=sums, counts=counts)


def judge(got, ref, what=""):
    """got (..., ) float64 against (value, bound): NaN / inf patterns must match, finite values lie within the bound; -> worst err / bound"""
    want, bound = ref
    got = torch.as_tensor(got).detach().cpu().double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    fin = torch.isfinite(want)
    odd_ok = (torch.isnan(got) & torch.isnan(want)) | (got == want)
    if not bool(odd_ok[~fin].all()):
        i = int((~odd_ok & ~fin).reshape(-1).nonzero()[0])
        raise AssertionError(f"{what}: element {i}: got {float(got.reshape(-1)[i])}, the definitions give {float(want.reshape(-1)[i])}")
    if not bool(torch.isfinite(got[fin]).all()):
        raise AssertionError(f"{what}: a non-finite value where the definitions give a finite one")
    err = (got - want).abs()[fin]
    b = bound[fin]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: finite element {i}: err {float(err[i]):.3e}, bound {float(b[i]):.3e}, ratio {worst:.3g}")
    return worst


def check(got, ref, what=""):
    """got: dict(sums (R, C, 10) float64, counts (R, C, 3)) against regional_ref's; counts by value; -> the worst err / bound"""
    gc = torch.as_tensor(got["counts"]).detach().cpu().long()
    assert torch.equal(gc, ref["counts"]), f"{what}: counts differ at {(gc != ref['counts']).nonzero()[:4].tolist()}"
    return judge(got["sums"], ref["sums"], f"{what}: sums")


def passes(got, ref):
    try:
        check(got, ref)
        return True
    except AssertionError:
        return False


def exact(got, ref):
    """sums and counts equal the oracle's bit for bit (the integer cases)"""
    return torch.equal(torch.as_tensor(got["counts"]).cpu().long(), ref["counts"]) and \
        torch.equal(torch.as_tensor(got["sums"]).cpu().double(), ref["sums"][0])


# ---- the kernel's arithmetic restated in fp32 -----------------------------------------------------------------------------------------
DEFECTS = ("bit_ignored", "bit_r_plus_1", "invalid_counted_valid", "invalid_of_other_regions", "w_over_all_points", "acc_over_valid",
           "padding_counted", "e_sign", "var_div_M", "wrap_threshold", "weight_by_col", "inv_norm_truth")


def _seq_sum(terms, sel):
    """one workgroup's sequential fp64 sum over its points in index order, then the records in record order; terms, sel (P,)"""
    v = np.where(sel, terms, 0.0)
    total = 0.0
    for b in range(0, v.size, TPB * TPW):
        chunk = v[b : b + TPB * TPW]
        total = total + (float(np.add.accumulate(chunk)[-1]) if chunk.size else 0.0)
    return total


def kernel_f32(v, t, w, mask, R, cl=None, norm=None, *, defect=None):
    """regional.hip restated: the fused inverse normalisation, the fp32 point values in the kernel's operation order (sequential member
    sums, two-pass variance, fused multiply-adds in the spread), fp64 sums of exact products in point order per workgroup and record order.
    v (M, C, H, W) as stored, norm = (mean, std, target_std) | None.  -> dict(sums (R, C, 10) float64, counts (R, C, 3) int64)"""
    M, C, H, W = v.shape
    P = H * W
    x = (v.float() if norm is None else inv_norm_f32(v, *norm)).reshape(M, C, P)
    t = t.float()
    if defect == "inv_norm_truth" and norm is not None:
        t = inv_norm_f32(t.unsqueeze(0), *norm)[0]
    t = t.reshape(C, P)
    a = None if cl is None else cl.float().reshape(C, P)
    Mf = torch.tensor(float(M), dtype=torch.float32)
    s, skill = torch.zeros(C, P), torch.zeros(C, P)
    nan_m = torch.zeros(C, P, dtype=torch.bool)
    for i in range(M):
        s = s + x[i]
        nan_m |= torch.isnan(x[i])
        skill = skill + (t - x[i]).abs()
    skill = skill / Mf
    mean = s / Mf
    ss = torch.zeros(C, P)
    for i in range(M):
        d = x[i] - mean
        ss = ss + d * d
    var, spread = torch.zeros(C, P), torch.zeros(C, P)
    if M >= 2:
        var = ss / (Mf if defect == "var_div_M" else Mf - 1.0)
        xs = torch.sort(torch.nan_to_num(x, nan=float("inf")), dim=0).values  # fminf / fmaxf drop a NaN; such points are not valid
        ws = torch.zeros(C, P)
        for i in range(M):
            coef = 2.0 * torch.tensor(float(i + 1)) - Mf - 1.0
            ws = (xs[i].double() * coef.double() + ws.double()).float()  # fmaf: the product exact, one rounding
        spread = 2.0 * ws / (Mf * (Mf - 1.0))
    e = t - mean if defect == "e_sign" else mean - t
    se = e * e
    valid = ~nan_m & ~torch.isnan(t)
    vals = [None, e, se, var, skill, spread]
    acc_valid = torch.zeros_like(valid)
    if a is not None:
        fa, ta = mean - a, t - a
        vals += [None, fa * ta, fa * fa, ta * ta]
        acc_valid = valid if defect == "acc_over_valid" else valid & ~torch.isnan(a)
    if defect == "invalid_counted_valid":
        valid = torch.ones_like(valid)
        acc_valid = valid if a is None else ~torch.isnan(a)
    rows = torch.arange(P) // W
    if defect == "weight_by_col":
        rows = (torch.arange(P) % W) % H
    wp = w.float()[rows].double().numpy()
    bits = region_bits(mask, MAX_R)
    sums, counts = torch.zeros(R, C, NS, dtype=torch.float64), torch.zeros(R, C, NC, dtype=torch.int64)
    pad = (-P) % TPB if defect == "padding_counted" else 0  # the padding threads of the last tile re-read point 0
    for r in range(R):
        b = bits[(r + 1) % MAX_R] if defect == "bit_r_plus_1" else bits[r]
        if defect == "bit_ignored":
            b = torch.ones(P, dtype=torch.bool)
        any_region = bits[:R].any(0)
        for c in range(C):
            sel_v, sel_a = (b & valid[c]).numpy(), (b & acc_valid[c]).numpy()
            inv = (any_region if defect == "invalid_of_other_regions" else b) & ~valid[c]
            counts[r, c] = torch.tensor([int(sel_v.sum()), int(inv.sum()), int(sel_a.sum())])
            if pad and bool(b[0]):
                counts[r, c] += pad * torch.tensor([int(sel_v[0]), int(inv[0]), int(sel_a[0])])
            for k in range(len(vals)):
                sel = sel_v if k < 6 else sel_a
                if k == 0 and defect == "w_over_all_points":
                    sel = b.numpy()
                val = np.ones(P) if vals[k] is None else vals[k][c].double().numpy()
                with np.errstate(invalid="ignore", over="ignore"):
                    terms = wp * val
                    total = _seq_sum(terms, sel)
                    if pad and bool(b[0]) and sel[0]:
                        for _ in range(pad):
                            total = total + terms[0]
                sums[r, c, k] = total
    return dict(sums=sums, counts=counts)


# ---- regions -----------------------------------------------------------------------------------------------------------------------------
def named_mask(H, W, names=None, defect=None):
    """the product's region_mask of the named regions on an H x W grid (rows as evaluate_ens_gpu.row_latitudes, longitudes 0, 360 / W, ...);
    defect "wrap_threshold": a box across the 0 degree meridian keeps its eastern part only (`europe` loses its western columns)"""
    from ladcast_amd.evaluate import NAMED_REGIONS, region_mask
    from ladcast_amd.evaluate.evaluate_ens_gpu import row_latitudes

    regions = [NAMED_REGIONS[n] for n in (names or NAMED_REGIONS)]
    lat, lon = row_latitudes(H), np.arange(W) * (360.0 / W)
    mask = region_mask(regions, lat, lon)
    if defect == "wrap_threshold":
        for r, reg in enumerate(regions):
            if reg.lon_min % 360.0 > reg.lon_max % 360.0 and reg.lon_max - reg.lon_min < 360.0:
                west = (lon >= reg.lon_min % 360.0)[None, :] & (((mask >> np.uint32(r)) & np.uint32(1)) == 1)
                mask = np.where(west, mask & ~np.uint32(1 << r), mask).astype(np.uint32)
    return mask


def case_mask(H, W, R, seed):
    """(H, W) int64 words.  R == 1: a random half.  R == 3: everything / nothing / the last point alone.  R == 32: overlapping random
    regions (30 % each), region 5 empty, region 7 the last point alone, bit 31 on half the points, a tenth of the points in no region.
    Bits >= R hold garbage the kernel must ignore."""
    g = gen(seed)
    P = H * W
    m = torch.zeros(P, dtype=torch.int64)
    if R == 1:
        m |= (torch.rand(P, generator=g) < 0.5).long()
        m[0] |= 1
    elif R == 3:
        m |= 1
        m[P - 1] |= 4
    else:
        for r in range(R):
            p = 0.5 if r == R - 1 else 0.3
            m |= (torch.rand(P, generator=g) < p).long() << r
        m &= ~((1 << 5) | (1 << 7)) if R > 7 else ~0
        m[torch.rand(P, generator=g) < 0.1] = 0
        m[0] |= 1
        if R > 7:
            m[P - 1] |= 1 << 7
    if R < 32:
        m |= torch.randint(0, 1 << (32 - R), (P,), generator=g) << R
    return m.reshape(H, W)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
INT_M = (1, 2, 8, 9, 24, 25, 50, 64)  # every arm of the sort ladder and both sides of its edges
INT_GRIDS = ((3, 50), (5, 103), (1, 257))  # under one tile; three tiles, the last ragged; a tile boundary inside a row
INT_R = (1, 3, 32)
INT_EXTRA = ((9, 9, 257, 32),)  # M, H, W, R: ten tiles = two workgroup records
INT_CASES = tuple((M, H, W, R) for M in INT_M for H, W in INT_GRIDS for R in INT_R) + INT_EXTRA


@functools.lru_cache(maxsize=None)
def integer_case(M, H, W, R, C=2):
    """Every fp32 point value and every fp64 sum is exact.  With S = M (M - 1): member i = base + S k_i, k a permutation (per point) of
    (2, -2, 1, -1, 1, -1, 0, ...) (fewer pairs for small M), base a small integer, truth = base + M j, climatology an integer, weights
    k / 4.  Then mean = base, x_i - mean = S k_i (squares S^2 k^2 and their sums have <= 24 significant bits), sum |t - x_i| and the
    spread's weighted sum are multiples of M and of S."""
    g = gen(SE._seed(M, H, W, R, 71))
    S = max(M * (M - 1), 1)
    k = [2, -2, 1, -1, 1, -1] if M >= 6 else [1, -1] if M >= 2 else []
    k = torch.tensor(k + [0] * (M - len(k)), dtype=torch.int64)
    perm = torch.rand(C, H, W, M, generator=g).argsort(-1)
    ks = k[perm].permute(3, 0, 1, 2)  # (M, C, H, W)
    base = torch.randint(-20, 21, (C, H, W), generator=g)
    x = (base.unsqueeze(0) + S * ks).float()
    t = (base + M * torch.randint(-2, 3, (C, H, W), generator=g)).float()
    cl = (base + torch.randint(-3, 4, (C, H, W), generator=g)).float()
    w = (1 + torch.arange(H) % 4).float() / 4
    return dict(v=x, x=x, t=t, cl=cl, w=w, norm=None, mask=case_mask(H, W, R, SE._seed(M, H, W, R, 73)), R=R)


PHYS = (("z50", 2e5, 3e3, 1e2), ("t2m", 280.0, 15.0, 1.0))
PHYS_M = (8, 24, 50, 64)
PHYS_HW = (5, 103)
PHYS_TARGET_STD = 0.5


@functools.lru_cache(maxsize=None)
def physical_case(M, R=32):
    """channel 0: mean 2e5, std 3e3 through the fused inverse normalisation; channel 1: a 280 +- 15 field; members = field + ensemble
    noise, truth one more draw, climatology the field; cos weights; the overlapping 32-region mask"""
    H, W = PHYS_HW
    C = len(PHYS)
    g = gen(SE._seed(M, 79))
    col = lambda i: torch.tensor([p[i] for p in PHYS], dtype=torch.float64).view(C, 1, 1)  # noqa: E731
    centre, fstd, estd = col(1), col(2), col(3)
    field = centre + fstd * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    members = field + estd * torch.randn(M, C, H, W, generator=g, dtype=torch.float64)
    truth = field + estd * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    norm = (centre.reshape(C).float(), fstd.reshape(C).float(), PHYS_TARGET_STD)
    v = ((members - centre) / fstd * PHYS_TARGET_STD).float()
    return dict(v=v, x=inv_norm_f32(v, *norm), t=truth.float(), cl=field.float(), w=cos_weights(H), norm=norm,
                mask=case_mask(H, W, R, SE._seed(M, 83)), R=R)


NAN_M, NAN_HW, NAN_R = 5, (4, 300), 3  # 1200 points = 5 tiles; tile 2 (points 512 .. 767) lies outside every region
PATTERNS = ("clean", "NaN in one member", "NaN in truth", "NaN in climatology only", "+inf in one member")


@functools.lru_cache(maxsize=None)
def nan_table_case(poison=True):
    """point p of a region carries pattern p % 5; three overlapping regions (thirds of the points, halves, the last 100 points); the points
    of no region - all of tile 2 among them - hold NaN and inf in members, truth and climatology when `poison`"""
    H, W = NAN_HW
    P, C, M = H * W, 2, NAN_M
    g = gen(89)
    x = torch.randn(M, C, P, generator=g) * 2 + 1
    t, cl = torch.randn(C, P, generator=g), torch.randn(C, P, generator=g) * 0.5
    kind = torch.arange(P) % len(PATTERNS)
    x[2][:, kind == 1] = float("nan")
    t[:, kind == 2] = float("nan")
    cl[:, kind == 3] = float("nan")
    x[M - 1][:, kind == 4] = float("inf")
    idx = torch.arange(P)
    m = ((idx % 3 == 0).long()) | ((idx % 2 == 0).long() << 1) | ((idx >= P - 100).long() << 2)
    outside = (idx >= 2 * TPB) & (idx < 3 * TPB) | (idx % 7 == 3)
    m[outside] = 0
    if poison:
        x[:, :, outside] = float("nan")
        x[1][:, outside & (idx % 2 == 0)] = float("-inf")
        t[:, outside] = float("inf")
        cl[:, outside & (idx % 2 == 1)] = float("nan")
    m |= 0x7FFFFFF8  # garbage above bit R - 1 on every point, the points of no region among them
    x = x.reshape(M, C, H, W)
    return dict(v=x, x=x, t=t.reshape(C, H, W), cl=cl.reshape(C, H, W), w=cos_weights(H), norm=None, mask=m.reshape(H, W), R=NAN_R, kind=kind,
                outside=outside)


NAMED_HW = (24, 48)  # 7.5 degree boxes: every named region holds points, europe on both sides of the 0 degree meridian


@functools.lru_cache(maxsize=None)
def named_case(M=3, defect=None):
    """the 13 named regions on a coarse grid, random fields; `defect` goes to named_mask"""
    H, W = NAMED_HW
    g = gen(97)
    x = torch.randn(M, 1, H, W, generator=g) + torch.linspace(0, 3, W).view(1, 1, 1, W)  # a zonal gradient: the columns of a box matter
    t, cl = torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g) * 0.3
    mask = torch.from_numpy(named_mask(H, W, defect=defect).astype(np.int64))
    return dict(v=x, x=x, t=t, cl=cl, w=cos_weights(H), norm=None, mask=mask, R=13)


def cpu_cases():
    """(name, case) of every table above, at the sizes the CPU judge can afford"""
    for M, H, W, R in ((1, 3, 50, 1), (2, 5, 103, 3), (9, 1, 257, 32), (25, 3, 50, 32), (64, 5, 103, 3)) + INT_EXTRA:
        yield f"integer M={M} {H}x{W} R={R}", integer_case(M, H, W, R)
    for M in (8, 50):
        yield f"physical M={M}", physical_case(M)
    yield "nan table", nan_table_case()
    yield "named regions", named_case()
