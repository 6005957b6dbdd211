"""float64 oracle, COUNTED bounds, an fp32 restatement and the case tables of the energy score kernel (csrc/energy.hip:
ldc_rollout_energy).  tests/test_gpu_energy.py runs the kernel; tests/test_energy_cpu.py proves on the CPU that every bound admits a
correct fp32 implementation that adds in another order, and checks the identities of the score in float64.

Definitions, per (channel, lead time): vectors y_0 .. y_{M-1} the members (fp32, after the inverse normalisation),
y_M the truth, N = M + 1; a point p is valid when no member and not the truth is NaN; w_p the latitude weight of p's row:
    D2[a][b] = sum over valid p of w_p (y_a[p] - y_b[p])^2 (diagonal: 0),  Wv = sum over valid p of w_p,  norm(a, b) = sqrt(D2[a][b] / Wv)
    skill = sum_i norm(i, M) / M,  spread = sum_{i != j} norm(i, j) / M^2,  spread_fair = the same sum / (M (M - 1)) (0 at M == 1)
    es = skill - spread / 2,  es_fair = skill - spread_fair / 2;  the four are NaN when Wv == 0
    group g: D2_g = sum over c in g, ascending, of D2_c * inv_scale2[c],  Wv_g = sum over c in g of Wv_c, then the same
The oracle works in float64 on the fp32 point values (the difference of two fp32 values is exact in float64) and sums the norms
sequentially in (i, j) order, the diagonal adding +0.0, as the kernel does: where every value is exact (the integer cases) the IEEE
divisions and square roots then give the kernel's bits.

Bounds, first order in U = 2**-24 and U53 = 2**-53, counted from the kernel's arithmetic, nothing fitted; n = the valid points:
    a term of D2   the fp32 subtraction and the fp32 product: (1 + U)^3 - 1 <= 3 U (1 + U) relative; the product by w is exact
    D2             every term is >= 0: 3 U (1 + U) D2, plus the fp64 additions.  Adding +0.0 is exact, so only additions of two non-zero
                   values round, and in any summation tree over n non-zero leaves a leaf passes at most n - 1 of them: n U53 D2
    Wv             n U53 Wv
    norm           sqrt halves the relative error of D2 / Wv; the division and the square root round once each:
                   r_norm = (r_D2 + r_Wv) / 2 * (1 + r_D2 + r_Wv) + 2 U53   (the factor covers the second order of the square root)
    skill          sum_i b_norm(i, M) / M + (M + 2) U53 skill: M additions, the division, and the rounding of the final subtraction of es
    spread         sum b_norm(i, j) / M^2 + (M^2 + 2) U53 spread: the additions, the division (M * M is exact), the product by 0.5 is exact
    spread_fair    the same with M (M - 1) (the product of the divisor rounds: one more U53)
    es, es_fair    b_skill + b_spread / 2, absolute: the two terms cancel, there is no relative bound
    group          D2_g: sum_c b_D2_c inv_scale2[c] + 2 n_c U53 D2_g (a product and an addition per channel of the group);
                   Wv_g: sum_c b_Wv_c + n_c U53 Wv_g; then as above
n_invalid is compared by value.  Values the definitions make NaN or inf carry no bound: their pattern (and the sign of an inf) must match."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import score_edge_refs as SE
from tests.redzone import U
from tests.regional_refs import judge  # noqa: F401  (shared, not copied)
from tests.score_edge_refs import cos_weights, gen, guard_case, inv_norm_f32  # noqa: F401  (shared, not copied)

# the constants of csrc/energy.hip
TPB, PT, CHUNK_TILES, BLK = 256, 32, 128, 16
CHUNK = PT * CHUNK_TILES  # 4096 points per workgroup
MAX_M, MAX_G = 256, 32
U53 = 2.0 ** -53
GUARD_CASES, GUARD_SLOTS, N_TRUTH = SE.GUARD_CASES, SE.GUARD_SLOTS, SE.N_TRUTH
FLT_MAX_BITS = SE.FLT_MAX_BITS
SCORES = ("es", "es_fair", "skill", "spread")  # planes 0 .. 3 of the kernel's `energy`; plane 4 is Wv


def geometry(M):
    """csrc/energy.hip make_geo: N, blocks per side, blocks of the upper triangle, blocks per workgroup, point slices, block groups"""
    N = M + 1
    NB = (N + 3) // 4
    NBP = NB * (NB + 1) // 2
    BPG = min(NBP, TPB)
    SL = 1
    while SL * 2 * BPG <= TPB and SL * 2 <= PT:
        SL *= 2
    return dict(N=N, NB=NB, NBP=NBP, BPG=BPG, SL=SL, NGRP=-(-NBP // TPB))


def workspace_bytes(M, C, L, P):
    """ldc_rollout_energy_workspace_bytes: per (channel, lead time) one record of NBP blocks per chunk and one for the total, the weight
    of every chunk and the total weight in fp64, and the invalid count of every chunk in int32"""
    nchunk = -(-(-(-P // PT)) // CHUNK_TILES)
    rec = geometry(M)["NBP"] * BLK * 8
    b = C * L * ((nchunk + 1) * rec + nchunk * 8 + 8 + nchunk * 4)
    return (b + 7) & ~7


# ---- float64 oracle with bounds ----------------------------------------------------------------------------------------------------
def _seq_sum(a):
    """the sequential fp64 sum of a flat array, from +0.0"""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        return float(np.add.accumulate(a)[-1]) if a.size else 0.0


def scores_of(D2, bD2, Wv, bWv, M, extra_adds=0):
    """the five quantities of one (M + 1, M + 1) matrix with their bounds -> {name: (value, bound)}, floats"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        norm = np.sqrt(D2 / Wv)
        np.fill_diagonal(norm, 0.0)
        r = np.where(D2 > 0, bD2 / np.where(D2 > 0, D2, 1.0), 0.0) + (bWv / Wv if Wv > 0 else 0.0)
        bn = norm * (0.5 * r * (1.0 + r) + 2 * U53)
        k_sum, s_sum = _seq_sum(norm[:M, M]), _seq_sum(norm[:M, :M])
        skill, spread = k_sum / float(M), s_sum / (float(M) * float(M))
        fair = s_sum / (float(M) * (float(M) - 1.0)) if M > 1 else 0.0
        b_skill = bn[:M, M].sum() / M + (M + 2) * U53 * abs(skill)
        b_spread = bn[:M, :M].sum() / (M * M) + (M * M + 2) * U53 * abs(spread)
        b_fair = (bn[:M, :M].sum() / (M * (M - 1)) + (M * M + 3) * U53 * abs(fair)) if M > 1 else 0.0
        if not Wv != 0.0:
            skill = spread = fair = float("nan")
        return dict(es=(skill - 0.5 * spread, b_skill + 0.5 * b_spread), es_fair=(skill - 0.5 * fair, b_skill + 0.5 * b_fair),
                    skill=(skill, b_skill), spread=(spread, b_spread))


def dist2_ref(x, t, w, block=512):
    """x (M, C, H, W) fp32, t (C, H, W), w (H,) -> D2 (C, N, N), its bound, Wv (C,), its bound, n_invalid (C,) - numpy float64"""
    M, C, H, W = x.shape
    P, N = H * W, M + 1
    y = np.concatenate([x.reshape(M, C, P).numpy(), t.reshape(1, C, P).numpy()]).astype(np.float64)
    wp = np.repeat(w.double().numpy(), W)
    D2, Wv, ninv = np.zeros((C, N, N)), np.zeros(C), np.zeros(C, dtype=np.int64)
    for c in range(C):
        valid = ~np.isnan(y[:, c]).any(0)
        ninv[c] = P - int(valid.sum())
        yv, wv = y[:, c][:, valid], wp[valid]
        Wv[c] = wv.sum()
        with np.errstate(invalid="ignore", over="ignore"):
            for b0 in range(0, yv.shape[1], block):
                d = yv[:, None, b0 : b0 + block] - yv[None, :, b0 : b0 + block]
                D2[c] += (wv[b0 : b0 + block] * (d * d)).sum(-1)
        np.fill_diagonal(D2[c], 0.0)
    n = (P - ninv).astype(np.float64)
    with np.errstate(invalid="ignore"):
        bD2 = D2 * (3 * U * (1 + U) + n[:, None, None] * U53)
    return D2, bD2, Wv, n * U53 * Wv, ninv


def energy_ref(x, t, w, groups=(), scales=None):
    """-> dict: dist2 (value, bound) (C, N, N); energy (value, bound) (5, C): es, es_fair, skill, spread, Wv; n_invalid (C,) int64;
    with groups energy_group (value, bound) (5, G).  torch float64 tensors.  groups: sequences of channel indices; scales (C,)"""
    M, C = x.shape[0], x.shape[1]
    D2, bD2, Wv, bWv, ninv = dist2_ref(x, t, w)

    def table(mats):
        val, bnd = np.zeros((5, len(mats))), np.zeros((5, len(mats)))
        for k, (d, bd, wv, bwv) in enumerate(mats):
            sc = scores_of(d, bd, wv, bwv, M)
            for i, name in enumerate(SCORES):
                val[i, k], bnd[i, k] = sc[name]
            val[4, k], bnd[4, k] = wv, bwv
        return torch.from_numpy(val), torch.from_numpy(np.nan_to_num(bnd, nan=0.0, posinf=0.0))

    out = dict(dist2=(torch.from_numpy(D2), torch.from_numpy(np.nan_to_num(bD2, nan=0.0, posinf=0.0))), n_invalid=torch.from_numpy(ninv),
               energy=table([(D2[c], bD2[c], Wv[c], bWv[c]) for c in range(C)]))
    if groups:
        inv = inv_scale2(scales).numpy()
        mats = []
        for chans in groups:
            d, bd, wv, bwv = np.zeros_like(D2[0]), np.zeros_like(D2[0]), 0.0, 0.0
            with np.errstate(invalid="ignore", over="ignore"):
                for c in sorted(int(v) for v in chans):
                    d = d + D2[c] * inv[c]
                    bd = bd + bD2[c] * inv[c]
                    wv, bwv = wv + Wv[c], bwv + bWv[c]
                bd = bd + 2 * len(chans) * U53 * d
            mats.append((d, bd, wv, bwv + len(chans) * U53 * wv))
        out["energy_group"] = table(mats)
    return out


def inv_scale2(scales):
    """1 / (s * s) in float64, as ladcast_amd.evaluate.energy.inverse_scale2 forms it"""
    s = torch.as_tensor(scales).double().reshape(-1)
    return 1.0 / (s * s)


def check(got, ref, what=""):
    """got: dict(energy (5, C) float64, n_invalid (C,), [dist2 (C, N, N)], [energy_group (5, G)]) against energy_ref's; n_invalid by
    value; -> the worst err / bound"""
    gn = torch.as_tensor(got["n_invalid"]).detach().cpu().long()
    assert torch.equal(gn, ref["n_invalid"]), f"{what}: n_invalid {gn.tolist()}, expected {ref['n_invalid'].tolist()}"
    worst = judge(got["energy"], ref["energy"], f"{what}: energy")
    for k in ("dist2", "energy_group"):
        if k in ref and got.get(k) is not None:
            worst = max(worst, judge(got[k], ref[k], f"{what}: {k}"))
    return worst


def passes(got, ref):
    try:
        check(got, ref)
        return True
    except AssertionError:
        return False


def same_bits(a, b):
    a, b = torch.as_tensor(a).detach().cpu().contiguous(), torch.as_tensor(b).detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int64), b.view(torch.int64)) if a.dtype == torch.float64 else torch.equal(a, b)


def exact(got, ref):
    """every output equals the oracle's bit for bit, NaN where it is NaN (the integer cases)"""
    eq = lambda a, b: torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))  # noqa: E731
    ok = torch.equal(torch.as_tensor(got["n_invalid"]).cpu().long(), ref["n_invalid"]) and eq(torch.as_tensor(got["energy"]).cpu().double(), ref["energy"][0])
    for k in ("dist2", "energy_group"):
        if k in ref and got.get(k) is not None:
            ok = ok and eq(torch.as_tensor(got[k]).cpu().double(), ref[k][0])
    return ok


# ---- the kernel's arithmetic restated in fp32, added in ANOTHER order ---------------------------------------------------------------
DEFECTS = ("weight_by_col", "invalid_times_zero", "inv_norm_truth", "spread_over_M_M1", "skill_over_N", "group_scale_not_squared")


def kernel_f32(v, t, w, norm=None, groups=(), scales=None, *, defect=None):
    """fp32 subtraction, fp32 square, exact product by the weight, fp64 additions from the LAST point to the first (the kernel adds slice
    by slice from the first), the norms added by numpy's pairwise sum (the kernel adds them one by one).  v (M, C, H, W) as stored, norm
    = (mean, std, target_std) | None.  -> dict(energy (5, C), n_invalid (C,), dist2 (C, N, N), [energy_group (5, G)])"""
    M, C, H, W = v.shape
    P, N = H * W, M + 1
    x = (v.float() if norm is None else inv_norm_f32(v, *norm)).reshape(M, C, P)
    t = t.float()
    if defect == "inv_norm_truth" and norm is not None:
        t = inv_norm_f32(t.unsqueeze(0), *norm)[0]
    y = torch.cat([x, t.reshape(1, C, P)]).numpy()
    rows = np.arange(P) // W
    if defect == "weight_by_col":
        rows = (np.arange(P) % W) % H
    wp = w.float().numpy()[rows].astype(np.float64)
    D2, Wv, ninv = np.zeros((C, N, N)), np.zeros(C), np.zeros(C, dtype=np.int64)
    for c in range(C):
        valid = ~np.isnan(y[:, c]).any(0)
        ninv[c] = P - int(valid.sum())
        if defect == "invalid_times_zero":
            yv, wv = y[:, c], np.where(valid, wp, 0.0)
        else:
            yv, wv = y[:, c][:, valid], wp[valid]
        with np.errstate(invalid="ignore", over="ignore"):
            d = yv[:, None, ::-1] - yv[None, :, ::-1]  # float32
            sq = d * d  # float32
            terms = wv[::-1] * sq.astype(np.float64)
            D2[c] = np.add.accumulate(terms, axis=-1)[..., -1] if terms.shape[-1] else 0.0
            Wv[c] = np.add.accumulate(wv[::-1])[-1] if wv.size else 0.0
        np.fill_diagonal(D2[c], 0.0)

    def five(d, wv):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            nm = np.sqrt(d / wv)
            np.fill_diagonal(nm, 0.0)
            skill = nm[:M, M].sum() / (N if defect == "skill_over_N" else M)
            s = nm[:M, :M].sum()
            spread = s / (M * (M - 1) if defect == "spread_over_M_M1" and M > 1 else M * M)
            fair = s / (M * (M - 1)) if M > 1 else 0.0
            if not wv != 0.0:
                skill = spread = fair = float("nan")
            return [skill - 0.5 * spread, skill - 0.5 * fair, skill, spread, wv]

    out = dict(energy=torch.tensor([five(D2[c], Wv[c]) for c in range(C)], dtype=torch.float64).T.contiguous(), n_invalid=torch.from_numpy(ninv),
               dist2=torch.from_numpy(D2))
    if groups:
        s = torch.as_tensor(scales).double().reshape(-1)
        inv = (1.0 / s if defect == "group_scale_not_squared" else 1.0 / (s * s)).numpy()
        rows5 = []
        for chans in groups:
            with np.errstate(invalid="ignore", over="ignore"):
                d = sum(D2[c] * inv[c] for c in sorted(chans, reverse=True))  # descending: another order
                rows5.append(five(d, sum(Wv[c] for c in sorted(chans, reverse=True))))
        out["energy_group"] = torch.tensor(rows5, dtype=torch.float64).T.contiguous()
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# every M the issue names; 87 / 88: the last ensemble size one workgroup's 256 blocks serve and the first that needs two block groups
INT_M = (1, 2, 3, 17, 64, 65, 87, 88, 256)
INT_SMALL_GRIDS = ((1, 1), (3, 5), (1, PT - 1), (4, PT // 4), (3, (PT + 1) // 3))  # 1, 15, and 31 / 32 / 33 points; 3 x 11: W odd
INT_CHUNK_GRIDS = ((63, 65), (64, 64), (17, 241))  # CHUNK - 1, CHUNK, CHUNK + 1 points
INT_CASES = tuple((M, H, W) for M in INT_M for H, W in INT_SMALL_GRIDS) + ((256, 13, 23),) \
    + tuple((M, H, W) for M in (1, 3, 17) for H, W in INT_CHUNK_GRIDS) + ((65, 17, 241), (88, 17, 241))
assert [H * W for H, W in INT_SMALL_GRIDS[2:]] == [PT - 1, PT, PT + 1] and [H * W for H, W in INT_CHUNK_GRIDS] == [CHUNK - 1, CHUNK, CHUNK + 1]


@functools.lru_cache(maxsize=None)
def integer_case(M, H, W, C=2):
    """members and truth small integers, weights k / 4: every fp32 difference and square and every fp64 sum is exact"""
    g = gen(SE._seed(M, H, W, 131))
    x = torch.randint(-8, 9, (M, C, H, W), generator=g).float()
    t = torch.randint(-8, 9, (C, H, W), generator=g).float()
    w = (1 + torch.arange(H) % 4).float() / 4
    return dict(v=x, x=x, t=t, w=w, norm=None)


PHYS = (("z500", 5e4, 3e3, 50.0), ("t2m", 280.0, 15.0, 1.0))  # name, mean, std of the field, ensemble spread
PHYS_M = (2, 20, 50)
PHYS_HW = (5, 103)
PHYS_TARGET_STD = 0.5
PHYS_GROUPS = ((0, 1), (1,))


@functools.lru_cache(maxsize=None)
def physical_case(M):
    """channel 0: geopotential-like, mean 5e4 and ensemble spread 50, through the fused inverse normalisation; channel 1: a 280 +- 15
    field; members = field + ensemble noise, truth one more draw; cos weights"""
    H, W = PHYS_HW
    C = len(PHYS)
    g = gen(SE._seed(M, 137))
    col = lambda i: torch.tensor([p[i] for p in PHYS], dtype=torch.float64).view(C, 1, 1)  # noqa: E731
    centre, fstd, estd = col(1), col(2), col(3)
    field = centre + fstd * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    members = field + estd * torch.randn(M, C, H, W, generator=g, dtype=torch.float64)
    truth = field + estd * torch.randn(C, H, W, generator=g, dtype=torch.float64)
    norm = (centre.reshape(C).float(), fstd.reshape(C).float(), PHYS_TARGET_STD)
    v = ((members - centre) / fstd * PHYS_TARGET_STD).float()
    return dict(v=v, x=inv_norm_f32(v, *norm), t=truth.float(), w=cos_weights(H), norm=norm, scales=fstd.reshape(C).float())


NAN_M, NAN_HW = 5, (4, 20)
NAN_CHANNELS = ("clean", "NaN in one member", "NaN in truth", "NaN in all", "+inf in one member", "+inf in two members at one point")
NAN_POINTS = (3, 40, 41, 79)  # where channels 1 and 2 are poisoned; channels 4 and 5 at point 40


@functools.lru_cache(maxsize=None)
def nan_table_case(poison=True):
    """one channel per pattern of NAN_CHANNELS, the same random field in every channel; `poison=False`: the clean field six times"""
    H, W = NAN_HW
    M, C, P = NAN_M, len(NAN_CHANNELS), H * W
    g = gen(139)
    x = (torch.randn(M, 1, P, generator=g) * 2 + 1).repeat(1, C, 1)
    t = torch.randn(1, P, generator=g).repeat(C, 1)
    if poison:
        pts = torch.tensor(NAN_POINTS)
        x[2, 1, pts] = float("nan")
        t[2, pts] = float("nan")
        x[:, 3], t[3] = float("nan"), float("nan")
        x[1, 4, 40] = float("inf")
        x[1, 5, 40], x[3, 5, 40] = float("inf"), float("inf")
    x = x.reshape(M, C, H, W)
    return dict(v=x, x=x, t=t.reshape(C, H, W), w=cos_weights(H), norm=None)


GROUP_C, GROUP_SST = 5, 3
GROUPS = ((0, 1), (1, 3, 4), (3,), (0, 1, 3, 4))  # overlapping; channel 2 in no group; groups 1 .. 3 span the SST-like channel


@functools.lru_cache(maxsize=None)
def group_case(M=6, H=7, W=19):
    """five channels of different scale, channel GROUP_SST with NaN over 30 % of the points (members and truth alike)"""
    g = gen(149)
    scales = torch.tensor([300.0, 2.5, 1.0, 0.75, 40.0])
    x = torch.randn(M, GROUP_C, H, W, generator=g) * scales.view(1, -1, 1, 1)
    t = torch.randn(GROUP_C, H, W, generator=g) * scales.view(-1, 1, 1)
    land = torch.rand(H, W, generator=g) < 0.3
    x[:, GROUP_SST][:, land] = float("nan")
    t[GROUP_SST][land] = float("nan")
    return dict(v=x, x=x, t=t, w=cos_weights(H), norm=None, scales=scales, groups=GROUPS, land=land)


def cpu_cases():
    """(name, case, groups, scales) of every table above, at the sizes the CPU judge can afford"""
    for M, H, W in ((1, 1, 1), (2, 3, 5), (3, 1, 31), (17, 4, 8), (65, 3, 11), (3, 17, 241)):
        yield f"integer M={M} {H}x{W}", integer_case(M, H, W), (), None
    for M in PHYS_M:
        c = physical_case(M)
        yield f"physical M={M}", c, PHYS_GROUPS, c["scales"]
    yield "nan table", nan_table_case(), (), None
    c = group_case()
    yield "groups", c, c["groups"], c["scales"]
