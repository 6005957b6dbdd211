"""Integer / float64 oracle, the COUNTED bound, an fp32 restatement (with planted defects) and the case tables of the threshold-event
kernel (csrc/events.hip: ldc_rollout_events).  tests/test_gpu_events.py runs the kernel; tests/test_events_cpu.py proves on the CPU that
the bound admits a correct fp32 implementation in the kernel's order and that every planted defect is caught by the case tables.  Shared
helpers and cases come from tests/score_edge_refs.py.

Definitions, per grid point of event e = (channel, dir, thr, anomaly) with the fp32 members x_i the kernel scores
(after `inv_norm_f32` where the inverse normalisation is fused), truth t, climatology a, latitude weight w:
    u_i = x_i, v = t;  with anomaly u_i = x_i - a, v = t - a, ONE fp32 subtraction each (reproduced here with torch fp32)
    n = #{u_i > thr} in 0 .. M, o = (v > thr)  (dir == -1: <);  thr is the fp32 value the descriptor holds
    the point is valid when no member, not the truth and (anomaly) not the climatology is NaN; inf is an ordinary ordered value
Bins are formed from the fp32 values themselves, so hist_count and n_invalid must be equal bit for bit.

Bound, first order in U = 2**-24, counted from the kernel's order, nothing fitted:
  hist_weight[n, o]  a sequential sum of the weights of the n_b points of the bin inside each workgroup record, then the nrec records in
                     order: at most n_b + nrec additions on partial sums that never exceed the bin's sum w:  (n_b + nrec) U sum w
"""
from __future__ import annotations

import functools

import torch

from tests import score_edge_refs as R
from tests.redzone import U
from tests.score_edge_refs import FINISH_SHAPES, GUARD_CASES, cos_weights, gen, guard_case, inv_norm_f32  # noqa: F401  (shared, not copied)

TPB = R.TPB
MAX_M, MAX_E = 1024, 32
HEAD = 4
GUARD_SLOTS, N_TRUTH, N_CLIM = R.GUARD_SLOTS, R.N_TRUTH, R.N_CLIM
judge, same_bits = R.judge, R.same_bits


def tiles_per_wg(M):
    """events.hip: the record holds 4 (M + 1) words, so a workgroup covers more 256-point tiles as M grows"""
    return 1 if M <= 32 else -(-M // 32)


def n_records(P, M):
    return -(-(-(-P // TPB)) // tiles_per_wg(M))


def rec_words(M):
    return HEAD + 4 * (M + 1)


def workspace_bytes(M, E, L, P):
    return 4 * L * E * n_records(P, M) * rec_words(M)


def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _cmp(a, thr, d, ge=False):
    if d > 0:
        return a >= thr if ge else a > thr
    return a <= thr if ge else a < thr


# ---- integer / float64 oracle ----------------------------------------------------------------------------------------------------------
def keys_of(x, t, cl, event):
    """x (M, C, ...) fp32, t / cl (C, ...) -> (n int64 (...), o int64 (...), valid bool (...)) of one event, compared as fp32 values"""
    c, d, thr, anom = event
    xc, tc = x[:, c].float(), t[c].float()
    valid = ~torch.isnan(xc).any(0) & ~torch.isnan(tc)
    if anom:
        a = cl[c].float()
        xc, tc = xc - a.unsqueeze(0), tc - a  # one fp32 subtraction each
        valid = valid & ~torch.isnan(a)
    thr = f32(thr)
    return _cmp(xc, thr, d).sum(0), _cmp(tc, thr, d).long(), valid


def events_ref(x, t, w, events, cl=None):
    """x (M, C, H, W) the fp32 values the kernel scores, t / cl (C, H, W), w (H,), events [(channel, dir, thr, anomaly)] -> dict:
    hist (E, M + 1, 2) int64; hist_w (value, bound) (E, M + 1, 2) float64; n_invalid (E,) int64"""
    M, C, H, W = x.shape
    P, E = H * W, len(events)
    wp = w.double().view(H, 1).expand(H, W).reshape(P)
    hist, hist_w = torch.zeros(E, 2 * (M + 1), dtype=torch.int64), torch.zeros(E, 2 * (M + 1), dtype=torch.float64)
    n_invalid = torch.zeros(E, dtype=torch.int64)
    for e, ev in enumerate(events):
        n, o, valid = (v.reshape(P) for v in keys_of(x, t, cl, ev))
        key = (2 * n + o)[valid]
        hist[e] = torch.bincount(key, minlength=2 * (M + 1))
        hist_w[e] = torch.bincount(key, weights=wp[valid], minlength=2 * (M + 1))
        n_invalid[e] = (~valid).sum()
    b_hw = (hist + n_records(P, M)).double() * U * hist_w
    shape = (E, M + 1, 2)
    return dict(hist=hist.reshape(shape), hist_w=(hist_w.reshape(shape), b_hw.reshape(shape)), n_invalid=n_invalid)


def brute_force(x, t, w, events, cl=None):
    """the definitions as a Python loop over points (tiny cases only) -> hist, hist_w (float64), n_invalid"""
    import math
    import struct

    def r32(v):
        return struct.unpack("f", struct.pack("f", v))[0]

    M, C, H, W = x.shape
    E = len(events)
    hist, hist_w = torch.zeros(E, M + 1, 2, dtype=torch.int64), torch.zeros(E, M + 1, 2, dtype=torch.float64)
    n_invalid = torch.zeros(E, dtype=torch.int64)
    for e, (c, d, thr, anom) in enumerate(events):
        thr = r32(thr)
        for h in range(H):
            for k in range(W):
                xs, tt = [float(v) for v in x[:, c, h, k]], float(t[c, h, k])
                a = float(cl[c, h, k]) if anom else 0.0
                if any(math.isnan(v) for v in xs) or math.isnan(tt) or math.isnan(a):
                    n_invalid[e] += 1
                    continue
                if anom:  # the difference of two fp32 values rounded to fp32 once (float64 holds it exactly before the rounding)
                    xs, tt = [r32(v - a) if math.isfinite(v - a) else v - a for v in xs], r32(tt - a) if math.isfinite(tt - a) else tt - a
                hitf = (lambda v: v > thr) if d > 0 else (lambda v: v < thr)
                n, o = sum(hitf(v) for v in xs), int(hitf(tt))
                hist[e, n, o] += 1
                hist_w[e, n, o] += float(w[h])
    return dict(hist=hist, hist_w=hist_w, n_invalid=n_invalid)


def check(got, ref, what=""):
    """got {hist, hist_w (E, M + 1, 2), n_invalid (E,)} against events_ref's dict: the integers equal, every weight within its bound;
    returns the worst err / bound ratio.  Raises AssertionError."""
    gh, gn = torch.as_tensor(got["hist"]).cpu().long(), torch.as_tensor(got["n_invalid"]).cpu().long()
    assert gh.shape == ref["hist"].shape, f"{what}: hist_count is {tuple(gh.shape)}, expected {tuple(ref['hist'].shape)}"
    assert torch.equal(gh, ref["hist"]), f"{what}: hist_count differs at {(gh != ref['hist']).nonzero()[:4].tolist()}"
    assert torch.equal(gn, ref["n_invalid"]), f"{what}: n_invalid {gn.tolist()} != {ref['n_invalid'].tolist()}"
    return judge(got["hist_w"], ref["hist_w"], f"{what} hist_weight")


def passes(got, ref):
    try:
        check(got, ref)
        return True
    except AssertionError:
        return False


# ---- the kernel's arithmetic in fp32 torch, with planted defects ------------------------------------------------------------------------
DEFECTS = ("ge", "dir", "anom_truth", "invalid_bin0", "swap_o", "pad", "thr_before_norm", "channel_e", "drop_M")


def kernel_f32(v, t, w, events, cl=None, norm=None, *, defect=None):
    """events_kernel + events_finish_kernel restated in fp32 torch.  v (M, C, H, W): the forecast as stored; norm = (mean, std, target_std)
    or None: the fused inverse normalisation (`inv_norm_f32`).  Per workgroup record (tpw tiles of 256 points) one sequential sum per bin
    in point order, then the records in order.  -> hist (E, M + 1, 2) int64, hist_w (E, M + 1, 2) fp32, n_invalid (E,).  Planted defects:
      ge: >= for > (<= for <);  dir: dir == -1 treated as +1;  anom_truth: the climatology subtracted from the members, not from the truth;
      invalid_bin0: an invalid point counted in bin (0, 0) instead of n_invalid;  swap_o: the o columns swapped;  pad: the padding threads of
      the last partial tile counted (they read point 0);  thr_before_norm: the threshold compared before the inverse normalisation;
      channel_e: event e reads channel e (mod C) instead of channel[e];  drop_M: bin n = M dropped"""
    assert defect in (None,) + DEFECTS
    v, t, w = v.float(), t.float(), w.float()
    M, C, H, W = v.shape
    P, E = H * W, len(events)
    x = v if norm is None or defect == "thr_before_norm" else inv_norm_f32(v, *norm)
    x, t = x.reshape(M, C, P), t.reshape(C, P)
    a_ = None if cl is None else cl.float().reshape(C, P)
    wp = w.view(H, 1).expand(H, W).reshape(P)
    tpw, nrec, NB = tiles_per_wg(M), n_records(P, M), 2 * (M + 1)
    per = tpw * TPB
    Pp = nrec * per
    hist, hist_w = torch.zeros(E, NB, dtype=torch.int64), torch.zeros(E, NB)
    n_invalid = torch.zeros(E, dtype=torch.int64)
    rows = torch.arange(nrec)
    for e, (c, d, thr, anom) in enumerate(events):
        if defect == "channel_e":
            c = e % C
        if defect == "dir":
            d = 1
        thr = f32(thr)
        xc, tc = x[:, c], t[c]
        valid = ~torch.isnan(xc).any(0) & ~torch.isnan(tc)
        if anom:
            a = a_[c]
            xc = xc - a.unsqueeze(0)
            tc = tc if defect == "anom_truth" else tc - a
            valid = valid & ~torch.isnan(a)
        n, o = _cmp(xc, thr, d, defect == "ge").sum(0), _cmp(tc, thr, d, defect == "ge").long()
        key = torch.where(valid, 2 * n + (1 - o if defect == "swap_o" else o), torch.full_like(n, -1))
        n_invalid[e] = (~valid).sum()
        if defect == "invalid_bin0":
            key, n_invalid[e] = key.clamp_min(0), 0
        if defect == "drop_M":
            key = torch.where(key >= 2 * M, torch.full_like(key, -1), key)
        kp, wpad = torch.full((Pp,), -1, dtype=torch.int64), torch.zeros(Pp)
        kp[:P], wpad[:P] = key, wp
        if defect == "pad":  # the threads past the plane read point 0; tiles past the last one are never run
            last = -(-P // TPB) * TPB
            kp[P:last], wpad[P:last] = key[0], wp[0]
        kp, wpad = kp.reshape(nrec, per), wpad.reshape(nrec, per)
        hc, hw = torch.zeros(nrec, NB, dtype=torch.int64), torch.zeros(nrec, NB)
        for p in range(min(per, -(-P // TPB) * TPB)):
            m = kp[:, p] >= 0
            hc[rows[m], kp[m, p]] += 1
            hw[rows[m], kp[m, p]] += wpad[m, p]
        for r in range(nrec):
            hist[e], hist_w[e] = hist[e] + hc[r], hist_w[e] + hw[r]
    return dict(hist=hist.reshape(E, M + 1, 2), hist_w=hist_w.reshape(E, M + 1, 2), n_invalid=n_invalid)


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# Every case is a dict: v (M, C, H, W) the forecast as stored, x the fp32 values the kernel scores (v, or inv_norm_f32(v)), t, cl (C, H, W),
# w (H,), events, norm (mean, std, target_std) | None.
#
# a. integer-valued members, truths, climatologies and thresholds: ties with the threshold are certain, so > against >= shows.  Per point
#    and channel a count k drawn uniformly from 0 .. M: k members take a high value (2, 3), the others a low one (-1, 0, 1), in a random
#    member order - every bin n = 0 .. M is reachable, bin M among them, whatever M is.
INT_M = (1, 2, 8, 9, 16, 17, 64, 65, 127, 128, 1024)  # every register arm and its boundary; streaming; 256 bins at 127; the second bin
#                                                       slot per thread at 128; the partial ninth slot at 1024
INT_GRIDS = ((3, 50), (16, 16), (1, 257))  # a partial tile; one exact tile; one point into a second tile
INT_EXTRA = ((65, 9, 100),)  # 900 points = 4 tiles at 3 tiles per workgroup: two records, the second one short
INT_CASES = tuple((M, H, W) for M in INT_M for H, W in INT_GRIDS) + INT_EXTRA
INT_C = 4
# two events on one channel with different directions, one on another channel with anomaly; no event e reads channel e
INT_EVENTS = ((2, 1, 1.0, 0), (2, -1, 0.0, 0), (0, 1, 1.0, 1))


def _integer_planes(M, C, P, g):
    k = torch.randint(0, M + 1, (C, P), generator=g)
    k[:, 0] = M  # every member above the threshold at point 0 ...
    if P > 1:
        k[:, 1] = 0  # ... and none at point 1, whatever the draw
    order = torch.rand(M, C, P, generator=g).argsort(0)  # a random member order per point
    high = order < k.unsqueeze(0)
    hi_v, lo_v = torch.randint(2, 4, (M, C, P), generator=g), torch.randint(-1, 2, (M, C, P), generator=g)
    return torch.where(high, hi_v, lo_v).float()


@functools.lru_cache(maxsize=None)
def integer_case(M, H, W):
    C, P = INT_C, H * W
    g = gen(R._seed(M, H, W, 81))
    x = _integer_planes(M, C, P, g).reshape(M, C, H, W)
    t = torch.randint(-1, 4, (C, H, W), generator=g).float()
    cl = torch.randint(-1, 2, (C, H, W), generator=g).float()
    return dict(v=x, x=x, t=t, cl=cl, w=cos_weights(H), events=INT_EVENTS, norm=None)


# b. the event mix over two lead times with truth / climatology slots that are not 0 .. L - 1: (M, C, L, H, W) = (9, 4, 2, 3, 50)
MIX_SHAPE = (9, 4, 2, 3, 50)
MIX_T_SLOTS, MIX_C_SLOTS = [5, 2], [3, 0]


@functools.lru_cache(maxsize=None)
def mix_case():
    M, C, L, H, W = MIX_SHAPE
    g = gen(R._seed(*MIX_SHAPE, 83))
    x = torch.stack([_integer_planes(M, C, H * W, g).reshape(M, C, H, W) for _ in range(L)], 2)
    tt = torch.randint(-1, 4, (N_TRUTH, C, H, W), generator=g).float()
    ct = torch.randint(-1, 2, (N_CLIM, C, H, W), generator=g).float()
    return dict(x=x, truth_table=tt, clim_table=ct, w=cos_weights(H), events=INT_EVENTS, t_slots=MIX_T_SLOTS, c_slots=MIX_C_SLOTS)


# c. physical scale through the fused inverse normalisation: thresholds placed on values that members take exactly after it
PHYS_M = (8, 50, 65)
PHYS_HW = (5, 67)  # 335 points: a partial second tile
PHYS_NORM = (torch.tensor([2e5, 5.4e4, 2e5, 280.0]), torch.tensor([3e3, 3e3, 3e3, 15.0]), 0.5)


@functools.lru_cache(maxsize=None)
def physical_case(M):
    H, W = PHYS_HW
    C = 4
    g = gen(R._seed(M, 85))
    field = torch.randn(C, H, W, generator=g)
    v = (0.5 * (field.unsqueeze(0) + 0.3 * torch.randn(M, C, H, W, generator=g))).float()
    x = inv_norm_f32(v, *PHYS_NORM)
    mean, std, _ = PHYS_NORM
    sh = (C, 1, 1)
    t = ((field + 0.3 * torch.randn(C, H, W, generator=g)) * std.view(sh) + mean.view(sh)).float()
    cl = (0.8 * field * std.view(sh) + mean.view(sh)).float()
    t[0, 2, 5] = x[0, 0, 1, 3]  # the truth on the threshold too
    anom_thr = float(x[M // 2, 2, 3, 11] - cl[2, 3, 11])  # an anomaly one member takes exactly (the fp32 difference)
    events = ((0, 1, float(x[0, 0, 1, 3]), 0), (0, -1, float(x[M - 1, 0, 4, 60]), 0), (2, 1, anom_thr, 1), (3, -1, float(x[0, 3, 0, 0]), 0))
    return dict(v=v, x=x, t=t, cl=cl, w=cos_weights(H), events=events, norm=PHYS_NORM)


# d. the finish loop (score_edge_refs.finish_case: 65 and 129 records of one tile, M = 3): a finish lane adds more than one record
FINISH_EVENTS = ((0, 1, 0.5, 0), (0, -1, 0.0, 1))


def finish_case(H, W):
    c = R.finish_case(H, W)
    return dict(v=c["x"], x=c["x"], t=c["t"], cl=c["cl"], w=c["w"], events=FINISH_EVENTS, norm=None)


# e. the NaN / inf table (score_edge_refs.nan_table_case, M = 5, 64 points).  Channel 0: clean / NaN in one member / in all members / in
#    the truth / in the climatology only; channel 1: those and +inf, -inf in one member, +inf in the truth; channel 2: NaN everywhere - no
#    event reads it; channel 3: clean
NAN_EVENTS = ((1, 1, 0.5, 0), (1, -1, 0.5, 0), (0, 1, 0.0, 1), (0, 1, 0.0, 0), (3, 1, 0.2, 1))


def nan_table_case():
    c = R.nan_table_case(R.NAN_M)
    return dict(v=c["x"], x=c["x"], t=c["t"], cl=c["cl"], w=c["w"], events=NAN_EVENTS, norm=None, kind=c["kind"])


def nan_table_invalid(kind):
    """n_invalid of NAN_EVENTS from the pattern table: NaN in a member or the truth (kinds 1 - 3) for every event, NaN in the climatology
    (kind 4) for the anomaly events only; inf is no NaN"""
    bad = lambda ch, hi: int(((kind[ch] >= 1) & (kind[ch] <= hi)).sum())  # noqa: E731
    return [bad(1, 3), bad(1, 3), bad(0, 4), bad(0, 3), 0]


# f. guard bands: score_edge_refs.GUARD_CASES (M, C, L, H, W, sst) with land NaNs in channel sst; events over the first and the last channel
def guard_events(C):
    return ((C - 1, 1, 0.5, 0), (C - 1, -1, 0.0, 0), (0, 1, 0.1, 1))


def cpu_cases():
    """the single-lead cases the CPU proofs run over: (name, case)"""
    for M, H, W in INT_CASES:
        yield f"integer M={M} {H}x{W}", integer_case(M, H, W)
    for M in PHYS_M:
        yield f"physical M={M}", physical_case(M)
    for H, W in FINISH_SHAPES:
        yield f"finish {H}x{W}", finish_case(H, W)
    yield "nan table", nan_table_case()
