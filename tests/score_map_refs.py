"""float64 oracle, COUNTED bound, an fp32 restatement (with planted defects) and the case tables of the score-map kernel
(csrc/score_maps.hip: ldc_rollout_score_maps).  tests/test_gpu_score_maps.py runs the kernel; tests/test_score_maps_cpu.py proves on the
CPU that the bound admits a correct implementation in the kernel's order and that every planted defect is caught.

The point values, their bounds and the validity masks are `point_values` of tests/regional_refs.py (the regional kernel forms the same
eight fp32 values); the integer, physical-scale and NaN / inf cases are that file's, the guard cases those of tests/score_edge_refs.py:
imported, not copied.  A CALL here is dict(v (M, C, L, H, W) as stored, norm (mean, std, target_std) | None, x the fp32 values scored,
t (L, C, H, W), cl (L, C, H, W) | None); a TABLE is dict(calls, channel_idx, plane_of_lead, P, init | None).

Definition: entry (ci, pl, k, p) of `sums` = init + the sum over the calls in order, over the leads l of a call in ascending order with
plane_of_lead[l] == pl, of the fp32 point value k of channel channel_idx[ci] at point p where the point is valid (k < 5) or ACC-valid
(k >= 5); `counts` = valid, invalid, ACC-valid samples.  Without a climatology terms 5 .. 7 and count 2 keep their init.
Bound, nothing fitted: after N contributions v_1 .. v_N with point bounds b_i, |got - sum v_i| <= sum b_i + N 2^-53 sum |v_i| (each of
the N fp64 additions rounds once, relative to a partial sum that sum |v_i| bounds; double(v) is exact).  A non-zero init counts as v_0
with bound 0.  Values the definitions make NaN or inf carry no bound: their pattern (and the sign of an inf) must match."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import regional_refs as R
from tests.regional_refs import integer_case, nan_table_case, physical_case, point_values  # noqa: F401  (shared, not copied)
from tests.score_edge_refs import GUARD_CASES, guard_case, inv_norm_f32  # noqa: F401

NT, NC, TPB, MAX_M = 8, 3, 256, 64
U53 = 2.0 ** -53
TERMS = ("e", "se", "var", "skill", "spread", "fta", "ffa", "tta")
SENTINEL, SENTINEL_N = 12345.0, 77  # finite init of the entries a call must not touch (the CPU tables; the device tests use NaN patterns)


def make_call(leads):
    """leads: dicts of tests/regional_refs.py's single-lead cases (v, x (M, C, H, W), t, cl (C, H, W) | None, norm) -> a CALL"""
    cl = None if leads[0]["cl"] is None else torch.stack([c["cl"] for c in leads])
    return dict(v=torch.stack([c["v"] for c in leads], 2), x=torch.stack([c["x"] for c in leads], 2), t=torch.stack([c["t"] for c in leads]),
                cl=cl, norm=leads[0]["norm"])


def rolled(c, k):
    """the single-lead case c with every field rolled by k points along a row: other data at every point, nothing new drawn"""
    roll = lambda a: None if a is None else torch.roll(a, k, -1)  # noqa: E731
    return dict(c, v=roll(c["v"]), x=roll(c["x"]), t=roll(c["t"]), cl=roll(c["cl"]))


# ---- float64 oracle with the counted bound ------------------------------------------------------------------------------------------
def maps_ref(tab):
    """-> dict: sums (value, bound) (Cm, P, 8, HW) float64, counts (Cm, P, 3, HW) int64"""
    chan, pol, P = tab["channel_idx"], tab["plane_of_lead"], tab["P"]
    M, C, L, H, W = tab["calls"][0]["x"].shape
    HW, Cm = H * W, len(chan)
    if tab.get("init") is None:
        val, cnt = torch.zeros(Cm, P, NT, HW, dtype=torch.float64), torch.zeros(Cm, P, NC, HW, dtype=torch.int64)
    else:
        val, cnt = tab["init"][0].double().reshape(Cm, P, NT, HW).clone(), tab["init"][1].long().reshape(Cm, P, NC, HW).clone()
    mag, pb, n_add = val.abs(), torch.zeros_like(val), torch.zeros(Cm, P, NT, HW, dtype=torch.float64)
    for call in tab["calls"]:
        assert len(pol) >= call["x"].shape[2]
        for l in range(call["x"].shape[2]):
            pl = pol[l]
            if pl < 0:
                continue
            pv, valid, acc_valid = point_values(call["x"][:, :, l], call["t"][l], None if call["cl"] is None else call["cl"][l])
            for ci, c in enumerate(chan):
                cnt[ci, pl, 0] += valid[c]
                cnt[ci, pl, 1] += ~valid[c]
                cnt[ci, pl, 2] += acc_valid[c]
                for k, name in enumerate(TERMS):
                    if name not in pv:
                        continue
                    sel = valid[c] if k < 5 else acc_valid[c]
                    v, b = pv[name]
                    val[ci, pl, k] = torch.where(sel, val[ci, pl, k] + v[c], val[ci, pl, k])
                    mag[ci, pl, k] += torch.where(sel, v[c].abs(), torch.zeros(HW, dtype=torch.float64))
                    pb[ci, pl, k] += torch.where(sel, b[c], torch.zeros(HW, dtype=torch.float64))
                    n_add[ci, pl, k] += sel
    return dict(sums=(val, pb + n_add * U53 * mag), counts=cnt)


def check(got, ref, what=""):
    """got: dict(sums (Cm, P, 8, HW) float64, counts (Cm, P, 3, HW)) against maps_ref's; counts by value; -> the worst err / bound"""
    gc = torch.as_tensor(got["counts"]).detach().cpu().long().reshape(ref["counts"].shape)
    assert torch.equal(gc, ref["counts"]), f"{what}: counts differ at {(gc != ref['counts']).nonzero()[:4].tolist()}"
    return R.judge(torch.as_tensor(got["sums"]).reshape(ref["sums"][0].shape), ref["sums"], f"{what}: sums")


def passes(got, ref):
    try:
        check(got, ref)
        return True
    except AssertionError:
        return False


def exact(got, ref):
    """sums and counts equal the oracle's bit for bit (the integer cases)"""
    return torch.equal(torch.as_tensor(got["counts"]).cpu().long().reshape(ref["counts"].shape), ref["counts"]) and \
        torch.equal(torch.as_tensor(got["sums"]).cpu().double().reshape(ref["sums"][0].shape), ref["sums"][0])


# ---- the kernel's arithmetic restated in fp32 -----------------------------------------------------------------------------------------
DEFECTS = ("invalid_added", "invalid_not_counted", "acc_over_valid", "descending_leads", "skipped_lead_added", "channel_idx_ignored",
           "plane_overwritten", "acc_touched_without_clim")


def point_f32(x, t, a):
    """ensemble_point_values (csrc/ensemble_common.h) restated: x (M, C, P) fp32 after the inverse normalisation, t (C, P), a (C, P) | None
    -> the eight fp32 values (None where there is no climatology), valid, acc_valid"""
    M = x.shape[0]
    Mf = torch.tensor(float(M), dtype=torch.float32)
    s, skill = torch.zeros_like(t), torch.zeros_like(t)
    nan_m = torch.zeros_like(t, dtype=torch.bool)
    for i in range(M):
        s = s + x[i]
        nan_m |= torch.isnan(x[i])
    for i in range(M):
        skill = skill + (t - x[i]).abs()
    skill, mean = skill / Mf, s / Mf
    ss = torch.zeros_like(t)
    for i in range(M):
        d = x[i] - mean
        ss = ss + d * d
    var, spread = torch.zeros_like(t), torch.zeros_like(t)
    if M >= 2:
        var = ss / (Mf - 1.0)
        xs = torch.sort(torch.nan_to_num(x, nan=float("inf"), posinf=float("inf"), neginf=float("-inf")), dim=0).values  # fminf / fmaxf drop a NaN
        ws = torch.zeros_like(t)
        for i in range(M):
            coef = 2.0 * torch.tensor(float(i + 1)) - Mf - 1.0
            ws = (xs[i].double() * coef.double() + ws.double()).float()  # fmaf: the product exact, one rounding
        spread = 2.0 * ws / (Mf * (Mf - 1.0))
    e = mean - t
    valid = ~nan_m & ~torch.isnan(t)
    vals = [e, e * e, var, skill, spread, None, None, None]
    acc_valid = torch.zeros_like(valid)
    if a is not None:
        fa, ta = mean - a, t - a
        vals[5:] = [fa * ta, fa * fa, ta * ta]
        acc_valid = valid & ~torch.isnan(a)
    return vals, valid, acc_valid


def kernel_f32(tab, *, defect=None):
    """score_maps.hip restated: the fused inverse normalisation, the fp32 point values in the kernel's operation order, and per (channel,
    plane, point) one accumulator that starts from the stored value and takes the leads of a call that share the plane in ascending order,
    fp64.  -> dict(sums (Cm, P, 8, HW) float64, counts (Cm, P, 3, HW) int64)"""
    chan, pol, P = tab["channel_idx"], list(tab["plane_of_lead"]), tab["P"]
    M, C, L, H, W = tab["calls"][0]["x"].shape
    HW, Cm = H * W, len(chan)
    if tab.get("init") is None:
        sums, counts = np.zeros((Cm, P, NT, HW)), np.zeros((Cm, P, NC, HW), dtype=np.int64)
    else:
        sums, counts = tab["init"][0].double().reshape(Cm, P, NT, HW).numpy().copy(), tab["init"][1].long().reshape(Cm, P, NC, HW).numpy().copy()
    if defect == "skipped_lead_added":
        pol = [max(p, 0) for p in pol]
    for call in tab["calls"]:
        Lc = call["v"].shape[2]
        x = (call["v"].float() if call["norm"] is None else inv_norm_f32(call["v"], *call["norm"])).reshape(M, C, Lc, HW)
        has_clim = call["cl"] is not None
        pts = {}
        for ci in range(Cm):
            c = ci if defect == "channel_idx_ignored" else chan[ci]
            for pl in range(P):
                leads = [l for l in range(Lc) if pol[l] == pl]
                if not leads:
                    continue
                if defect == "descending_leads":
                    leads = leads[::-1]
                acc = np.zeros((NT, HW)) if defect == "plane_overwritten" else sums[ci, pl].copy()
                n = np.zeros((NC, HW), dtype=np.int64) if defect == "plane_overwritten" else counts[ci, pl].copy()
                if defect == "acc_touched_without_clim" and not has_clim:
                    acc[5:], n[2] = 0.0, 0
                for l in leads:
                    if l not in pts:
                        pts[l] = point_f32(x[:, :, l], call["t"][l].float().reshape(C, HW), call["cl"][l].float().reshape(C, HW) if has_clim else None)
                    vals, valid, acc_valid = pts[l]
                    v_ok, a_ok = valid[c].numpy(), acc_valid[c].numpy()
                    if defect == "acc_over_valid" and has_clim:
                        a_ok = v_ok
                    add_ok = np.ones_like(v_ok) if defect == "invalid_added" else v_ok
                    with np.errstate(invalid="ignore", over="ignore"):
                        for k in range(NT):
                            if vals[k] is None:
                                continue
                            sel = add_ok if k < 5 else a_ok
                            acc[k] = np.where(sel, acc[k] + vals[k][c].double().numpy(), acc[k])
                    n[0] += v_ok
                    if defect != "invalid_not_counted":
                        n[1] += ~v_ok
                    n[2] += a_ok
                sums[ci, pl], counts[ci, pl] = acc, n
    return dict(sums=torch.from_numpy(sums), counts=torch.from_numpy(counts))


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
INT_M, INT_GRIDS = R.INT_M, R.INT_GRIDS
INT_CHANNELS, INT_PLANES, INT_P = [1, 0], [1, -1, 0, 1], 2
INT_SEEDS = (1, 3, 32)  # tests/regional_refs.py seeds its integer case by its region count: three calls, three data sets


@functools.lru_cache(maxsize=None)
def integer_table(M, H, W):
    """three calls of four leads and two channels each: call k is `integer_case(M, H, W, INT_SEEDS[k], C=8)`, whose eight channels are
    read as (lead, channel).  Every fp32 point value is a small integer (that file's docstring), so every fp64 sum is exact."""
    calls = []
    for seed in INT_SEEDS:
        c = integer_case(M, H, W, seed, 8)
        split = lambda a, c0: a[..., c0 : c0 + 2, :, :]  # noqa: E731
        calls.append(make_call([dict(v=split(c["v"], 2 * l), x=split(c["x"], 2 * l), t=split(c["t"], 2 * l), cl=split(c["cl"], 2 * l), norm=None)
                                for l in range(4)]))
    return dict(calls=calls, channel_idx=INT_CHANNELS, plane_of_lead=INT_PLANES, P=INT_P, init=None)


PHYS_M = R.PHYS_M


@functools.lru_cache(maxsize=None)
def physical_table(M, shared_plane=False):
    """`physical_case(M)` (channel 0 through the fused inverse normalisation at 2e5 +- 3e3, channel 1 at 280 +- 15) as three calls of two
    leads, every lead the case rolled by another number of points; one lead per plane, or (`shared_plane`) all in one"""
    c = physical_case(M)
    calls = [make_call([rolled(c, 7 * k + 3 * l) for l in range(2)]) for k in range(3)]
    return dict(calls=calls, channel_idx=[0, 1], plane_of_lead=[0, 0] if shared_plane else [0, 1], P=1 if shared_plane else 2, init=None)


@functools.lru_cache(maxsize=None)
def nan_table():
    """`nan_table_case()`: point p carries pattern p % 5 (clean, NaN in one member, NaN in truth, NaN in the climatology only, +inf in one
    member), and NaN / inf fill the points outside its regions; two calls of two leads (the second lead rolled by one point, so that
    a point meets two patterns) into one plane"""
    c = nan_table_case()
    calls = [make_call([c, rolled(c, 1)]) for _ in range(2)]
    return dict(calls=calls, channel_idx=[1, 0], plane_of_lead=[0, 0], P=1, init=None)


def sentinel_init(Cm, P, HW):
    s, n = torch.zeros(Cm, P, NT, HW, dtype=torch.float64), torch.zeros(Cm, P, NC, HW, dtype=torch.int64)
    s[:, :, 5:], n[:, :, 2] = SENTINEL, SENTINEL_N
    return s, n


@functools.lru_cache(maxsize=None)
def no_clim_table():
    """the nan table without its climatology, into buffers whose terms 5 .. 7 and count 2 hold a sentinel: they keep it"""
    t = nan_table()
    calls = [dict(c, cl=None) for c in t["calls"]]
    return dict(t, calls=calls, init=sentinel_init(2, 1, calls[0]["x"].shape[-1] * calls[0]["x"].shape[-2]))


ORDER_LEADS = (2.0 ** 60, -(2.0 ** 60), 1.0)


@functools.lru_cache(maxsize=None)
def order_table():
    """one member, truth 0, three leads x = 2^60, -2^60, 1 in one plane: e = x exactly, and the fp64 sum in ascending lead order is
    (2^60 - 2^60) + 1 = 1, in descending order (1 - 2^60) + 2^60 = 0.  Term 0 tells the order; nothing else is looked at."""
    H, W = 1, 3
    x = torch.tensor(ORDER_LEADS, dtype=torch.float32).view(1, 1, 3, 1, 1).expand(1, 1, 3, H, W).contiguous()
    t = torch.zeros(3, 1, H, W)
    return dict(calls=[dict(v=x, x=x, t=t, cl=None, norm=None)], channel_idx=[0], plane_of_lead=[0, 0, 0], P=1, init=None)


def order_ok(got):
    return bool((torch.as_tensor(got["sums"]).reshape(1, 1, NT, -1)[0, 0, 0] == 1.0).all())


def cpu_tables():
    """(name, table, exact) of every table above, at the sizes the CPU judge can afford"""
    for M, H, W in ((1, 3, 50), (2, 5, 103), (9, 1, 257), (25, 3, 50), (64, 5, 103)):
        yield f"integer M={M} {H}x{W}", integer_table(M, H, W), True
    for M in (8, 50):
        yield f"physical M={M}", physical_table(M), False
    yield "physical M=24 shared plane", physical_table(24, True), False
    yield "nan table", nan_table(), False
    yield "no climatology", no_clim_table(), False
