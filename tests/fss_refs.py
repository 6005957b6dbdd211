"""Integer / float64 oracles, the COUNTED bound, a float64 restatement (with planted defects) and the case tables of the neighbourhood
verification kernel (csrc/fss.hip: ldc_rollout_fss).  tests/test_gpu_fss.py runs the kernel; tests/test_fss_cpu.py proves on the CPU that
the vectorised oracle equals the definitions written as loops, that the bound admits the kernel's reduction order and that every planted
defect is caught by the case tables.  The point classification and the shared helpers come from tests/events_refs.py.

Definitions.  Every grid point q of event e = (channel, dir, thr, anomaly) is classified as in section 8.4: n(q)
in 0 .. M, o(q) in {0, 1}, valid(q).  For a radius r the window of centre p = (i, j) is rows i - r .. i + r clipped to 0 .. H - 1 and
columns j - r .. j + r modulo W.  Over the valid points of the window N = #valid, Sn = sum n, So = sum o (exact integers).  A centre
contributes when it is valid itself.  Per contributing centre in float64, every operation rounded on its own, w = double(lat_weight[i]):
    Pf = Sn / (M * N),  Po = So / N,  a = w * Pf,  b = w * Po,  d = Pf - Po,   terms (w, a, b, a * Pf, b * Po, (w * d) * d)
sums[e, s] are the sums of the six terms over the contributing centres; n_invalid[e] counts the other centres.

Bound, counted from the kernel's order, nothing fitted.  The terms themselves are the same float64 operations in the same order on the
same integers, so they are equal bit for bit; only the additions differ.  All terms are >= 0, so no partial sum exceeds the sum s.  The
kernel adds the 64 lanes of a wave by butterfly (6 levels), the 4 waves pairwise (2 levels) - the results of one level add up to at most
s, so a level costs at most u s with u = 2**-53 - and then the nrec = ceil(H W / 256) workgroup records one after the other (nrec
additions).  The oracle's math.fsum rounds once.  Hence |got - ref| <= (8 + nrec + 1) u s.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import score_edge_refs as R
from tests.events_refs import _cmp, _integer_planes, f32  # noqa: F401  (shared, not copied)
from tests.score_edge_refs import cos_weights, gen, inv_norm_f32  # noqa: F401

TPB = 256
U64 = 2.0 ** -53
NT = 6
MAX_SCALES = 16


def n_records(P):
    return -(-P // TPB)


def workspace_bytes(E, S, L, H, W):
    """fss.hip layout_of: records (fp64), invalid counts, packed words, table entries of three uint32; every part rounded up to 8 bytes"""
    up8 = lambda v: (v + 7) // 8 * 8  # noqa: E731
    planes, P = L * E, H * W
    return planes * n_records(P) * S * NT * 8 + up8(planes * n_records(P) * 4) + up8(planes * P * 4) + up8(planes * (H + 1) * (W + 1) * 12)


# ---- the classification of a point (events_refs), as numpy integers -------------------------------------------------------------------
def classify(x, t, cl, event, *, ge=False):
    """x (M, C, H, W) fp32, t / cl (C, H, W) -> n (H, W) int64, o (H, W) int64, valid (H, W) bool, valid_f (H, W) bool (no NaN member)"""
    c, d, thr, anom = event
    xc, tc = x[:, c].float(), t[c].float()
    valid_f = ~torch.isnan(xc).any(0)
    valid = valid_f & ~torch.isnan(tc)
    if anom:
        a = cl[c].float()
        xc, tc = xc - a.unsqueeze(0), tc - a  # one fp32 subtraction each
        valid = valid & ~torch.isnan(a)
    thr = f32(thr)
    n, o = _cmp(xc, thr, d, ge).sum(0), _cmp(tc, thr, d, ge).long()
    return n.numpy().astype(np.int64), o.numpy().astype(np.int64), valid.numpy(), valid_f.numpy()


def terms_of(Sn, So, N, M, w):
    """the six float64 terms, each operation rounded on its own (numpy float64 arithmetic does exactly that); N >= 1"""
    Sn, So, N, w = (np.asarray(v, dtype=np.float64) for v in (Sn, So, N, w))
    Pf = Sn / (np.float64(M) * N)
    Po = So / N
    a, b, d = w * Pf, w * Po, Pf - Po
    return np.stack([w, a, b, a * Pf, b * Po, (w * d) * d], -1)


# ---- the definitions as loops (tiny grids only) ---------------------------------------------------------------------------------------
def fss_brute(x, t, w, events, radii, cl=None):
    """-> sums (E, S, 6) float64 (math.fsum), n_invalid (E,) int64"""
    M, C, H, W = x.shape
    E, S = len(events), len(radii)
    sums, n_invalid = np.zeros((E, S, NT)), np.zeros(E, dtype=np.int64)
    w64 = w.float().double().numpy()
    for e, ev in enumerate(events):
        n, o, valid, _ = classify(x, t, cl, ev)
        n_invalid[e] = int((~valid).sum())
        for s, r in enumerate(radii):
            rows_t = []
            for i in range(H):
                for j in range(W):
                    if not valid[i, j]:
                        continue
                    N = Sn = So = 0
                    q = np.arange(j - r, j + r + 1) % W  # the window's columns: longitude is periodic
                    for ii in range(i - r, i + r + 1):
                        if ii < 0 or ii > H - 1:
                            continue  # past a pole
                        ok = valid[ii, q]
                        N, Sn, So = N + int(ok.sum()), Sn + int(n[ii, q][ok].sum()), So + int(o[ii, q][ok].sum())
                    rows_t.append(terms_of(Sn, So, N, M, w64[i]))
            tt = np.array(rows_t).reshape(-1, NT)
            sums[e, s] = [math.fsum(tt[:, k]) for k in range(NT)]
    return dict(sums=sums, n_invalid=n_invalid)


# ---- vectorised oracle -----------------------------------------------------------------------------------------------------------------
def _window(a, r):
    """integer window sums of a (H, W): columns j - r .. j + r modulo W (2 r + 1 <= W), rows i - r .. i + r clipped"""
    H, W = a.shape
    ext = np.concatenate([a[:, W - r:], a, a[:, :r]], 1) if r else a
    c = np.concatenate([np.zeros((H, 1), dtype=np.int64), np.cumsum(ext, 1)], 1)
    cols = c[:, 2 * r + 1:] - c[:, :W]
    rr = np.concatenate([np.zeros((1, W), dtype=np.int64), np.cumsum(cols, 0)], 0)
    i = np.arange(H)
    return rr[np.minimum(i + r, H - 1) + 1] - rr[np.maximum(i - r, 0)]


def fss_ref(x, t, w, events, radii, cl=None):
    """x (M, C, H, W) the fp32 values the kernel scores, t / cl (C, H, W), w (H,), events [(channel, dir, thr, anomaly)], radii ->
    dict: sums (value, bound) (E, S, 6) float64; n_invalid (E,) int64; contributing, clipped, reduced (E, S) int64: the centres that
    contribute, those among them whose window loses rows at a pole, and those whose N is reduced by invalid neighbours"""
    M, C, H, W = x.shape
    E, S = len(events), len(radii)
    sums, n_invalid = np.zeros((E, S, NT)), np.zeros(E, dtype=np.int64)
    contributing, clipped, reduced = (np.zeros((E, S), dtype=np.int64) for _ in range(3))
    w64 = np.broadcast_to(w.float().double().numpy().reshape(H, 1), (H, W))
    ones = np.ones((H, W), dtype=np.int64)
    for e, ev in enumerate(events):
        n, o, valid, _ = classify(x, t, cl, ev)
        n_invalid[e] = int((~valid).sum())
        v = valid.astype(np.int64)
        for s, r in enumerate(radii):
            assert r >= 0 and 2 * r + 1 <= W
            N, Sn, So, full = _window(v, r), _window(n * v, r), _window(o * v, r), _window(ones, r)
            tt = terms_of(Sn[valid], So[valid], N[valid], M, w64[valid])
            sums[e, s] = [math.fsum(tt[:, k]) for k in range(NT)]
            contributing[e, s] = int(valid.sum())
            clipped[e, s] = int((full[valid] < (2 * r + 1) ** 2).sum())
            reduced[e, s] = int((N[valid] < full[valid]).sum())
    return dict(sums=(sums, bound(sums, H * W)), n_invalid=n_invalid, contributing=contributing, clipped=clipped, reduced=reduced)


def bound(sums, P):
    """(8 + nrec + 1) u s per sum (module docstring): 6 + 2 butterfly levels, nrec records in order, the oracle's one rounding"""
    return (8 + n_records(P) + 1) * U64 * np.abs(np.asarray(sums, dtype=np.float64))


def check(got, ref, what=""):
    """got {sums (E, S, 6), n_invalid (E,)} against fss_ref's dict: n_invalid equal, every sum within its bound (a bound of 0 demands
    equality); returns the worst err / bound ratio.  Raises AssertionError."""
    gs = np.asarray(torch.as_tensor(got["sums"]).cpu(), dtype=np.float64)
    gn = np.asarray(torch.as_tensor(got["n_invalid"]).cpu(), dtype=np.int64)
    want, bnd = ref["sums"]
    assert gs.shape == want.shape, f"{what}: fss_sums is {gs.shape}, expected {want.shape}"
    assert np.array_equal(gn, ref["n_invalid"]), f"{what}: n_invalid {gn.tolist()} != {ref['n_invalid'].tolist()}"
    assert np.isfinite(gs).all(), f"{what}: fss_sums holds a NaN or inf at {np.argwhere(~np.isfinite(gs))[:4].tolist()}"
    err = np.abs(gs - want)
    bad = err > bnd
    assert not bad.any(), (f"{what}: fss_sums outside its bound at {np.argwhere(bad)[:4].tolist()}: got {gs[bad][:4].tolist()}, want "
                           f"{want[bad][:4].tolist()}, bound {bnd[bad][:4].tolist()}")
    ratio = np.where(err == 0, 0.0, err / np.maximum(bnd, 1e-300))
    return float(ratio.max())


def passes(got, ref):
    try:
        check(got, ref)
        return True
    except AssertionError:
        return False


# ---- the kernel's arithmetic in float64 numpy, with planted defects --------------------------------------------------------------------
DEFECTS = ("no_wrap", "wrap_off_by_one", "window_2r", "clipped_rows_in_N", "invalid_as_non_event", "invalid_centre", "no_M", "weight_row",
           "ge", "po_forecast_validity")


def _kernel_reduce(terms):
    """(P, 6) terms in point order, zeros at the centres that do not contribute -> (6,): lanes by butterfly, 4 waves pairwise, the
    workgroup records in order - fss_window_kernel + fss_finish_kernel"""
    P = terms.shape[0]
    nrec = n_records(P)
    v = np.zeros((nrec * TPB, NT))
    v[:P] = terms
    v = v.reshape(nrec, 4, 64, NT)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    wv = v[:, :, 0]
    rec = (wv[:, 0] + wv[:, 1]) + (wv[:, 2] + wv[:, 3])
    acc = np.zeros(NT)
    for r in range(nrec):
        acc = acc + rec[r]
    return acc


def kernel_f64(v, t, w, events, radii, cl=None, norm=None, *, defect=None):
    """ldc_rollout_fss restated on the CPU: the window sums offset by offset (no table), the terms and the kernel's reduction order.
    v (M, C, H, W): the forecast as stored; norm = (mean, std, target_std) or None.  -> sums (E, S, 6), n_invalid (E,).  Planted defects:
      no_wrap: columns outside 0 .. W - 1 dropped instead of wrapped;  wrap_off_by_one: a wrapped column lands one column off;
      window_2r: the window is 2 r wide (its last row and column missing);  clipped_rows_in_N: rows past a pole counted in N as valid
      non-events;  invalid_as_non_event: invalid neighbours counted in N with n = o = 0;  invalid_centre: an invalid centre contributes
      (where N >= 1);  no_M: Pf = Sn / N;  weight_row: lat_weight[p % H] for lat_weight[p // W];  ge: >= for > (<= for <);
      po_forecast_validity: So and its N from the points without a NaN member, the truth's and the climatology's NaN ignored"""
    assert defect in (None,) + DEFECTS
    M, C, H, W = v.shape
    x = v.float() if norm is None else inv_norm_f32(v, *norm)
    E, S, P = len(events), len(radii), H * W
    sums, n_invalid = np.zeros((E, S, NT)), np.zeros(E, dtype=np.int64)
    w64 = w.float().double().numpy()
    p = np.arange(P)
    wp = w64[p % H] if defect == "weight_row" else w64[p // W]
    jj = np.arange(W)

    def window(a, r, outside_rows=0):
        hi = r - 1 if defect == "window_2r" else r
        cols = np.zeros_like(a)
        for dc in range(-r, hi + 1):
            q = jj + dc
            inside = (q >= 0) & (q < W)
            if defect == "no_wrap":
                cols += np.where(inside, a[:, np.clip(q, 0, W - 1)], 0)
            elif defect == "wrap_off_by_one":
                cols += a[:, np.where(inside, q, (q + (1 if dc < 0 else -1)) % W)]
            else:
                cols += a[:, q % W]
        out = np.zeros_like(a)
        width = hi + r + 1
        ii = np.arange(H)
        for dr in range(-r, hi + 1):
            inside = ((ii + dr >= 0) & (ii + dr < H)).reshape(H, 1)
            out += np.where(inside, cols[np.clip(ii + dr, 0, H - 1)], outside_rows * width)
        return out

    for e, ev in enumerate(events):
        n, o, valid, valid_f = classify(x, t, cl, ev, ge=defect == "ge")
        n_invalid[e] = int((~valid).sum())
        vv = valid.astype(np.int64)
        for s, r in enumerate(radii):
            if defect == "invalid_as_non_event":
                N = window(np.ones_like(vv), r)
            else:
                N = window(vv, r, outside_rows=1 if defect == "clipped_rows_in_N" else 0)
            Sn, So, No = window(n * vv, r), window(o * vv, r), N
            if defect == "po_forecast_validity":
                vf = valid_f.astype(np.int64)
                So, No = window(o * vf, r), window(vf, r)
            centre = (N > 0) if defect == "invalid_centre" else valid
            Nf, Nof = np.where(centre, N, 1).astype(np.float64), np.where(centre & (No > 0), No, 1).astype(np.float64)
            with np.errstate(invalid="ignore"):  # window_2r at r = 0: an empty window, 0 / 0
                Pf = Sn / Nf if defect == "no_M" else Sn / (np.float64(M) * Nf)
                Po = So / Nof
            wc = wp.reshape(H, W)
            a, b, d = wc * Pf, wc * Po, Pf - Po
            tt = np.stack([wc, a, b, a * Pf, b * Po, (wc * d) * d], -1)
            tt = np.where(centre[..., None], tt, 0.0)
            sums[e, s] = _kernel_reduce(tt.reshape(P, NT))
    return dict(sums=sums, n_invalid=n_invalid)


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# Every case is a dict: v (M, C, H, W) the forecast as stored, x the fp32 values the kernel scores, t, cl (C, H, W), w (H,), events, radii,
# norm (mean, std, target_std) | None.
#
# a. integer-valued members, truths, climatologies and thresholds (ties certain), events_refs' planes with features written over them:
#    channel 0  a truth feature on columns W - 1 | 0 with the forecast's displaced across the seam to columns 0 | 1; a truth feature in
#               row 0 and one in row H - 1 (the forecast's one column on)
#    channel 1  a block of NaN truth ("land") inside windows, a NaN member at one point
#    channel 2  the anomaly event
INT_M = (1, 8, 9, 64, 65, 130)  # every register arm and its boundary, the streaming arm
INT_GRIDS = ((5, 7), (16, 16), (17, 33), (3, 50))  # one partial tile; one exact tile; three tiles with an odd row length; 2 r + 1 > H
INT_CASES = tuple((M, H, W) for M in INT_M for H, W in INT_GRIDS)
INT_C = 3
INT_EVENTS = ((0, 1, 1.0, 0), (1, -1, 0.0, 0), (2, 1, 1.0, 1), (1, 1, 1.0, 0))


def radii_for(H, W):
    """0, 1, 2, the widest window that fits, and H itself (every row, twice over) where 2 H + 1 <= W"""
    rs = {0, 1, 2, (W - 1) // 2}
    if 2 * H + 1 <= W:
        rs.add(H)
    return tuple(sorted(r for r in rs if 2 * r + 1 <= W))


@functools.lru_cache(maxsize=None)
def integer_case(M, H, W):
    C, P = INT_C, H * W
    g = gen(R._seed(M, H, W, 97))
    x = _integer_planes(M, C, P, g).reshape(M, C, H, W)
    t = torch.randint(-1, 4, (C, H, W), generator=g).float()
    cl = torch.randint(-1, 2, (C, H, W), generator=g).float()
    mid = H // 2
    x[:, 0, mid - 1 : mid + 1] = 0.0  # a quiet band for the seam feature
    t[0, mid - 1 : mid + 1] = 0.0
    t[0, mid - 1 : mid + 1, W - 1] = t[0, mid - 1 : mid + 1, 0] = 3.0
    x[:, 0, mid - 1 : mid + 1, 0:2] = 3.0
    t[0, 0, 2:4], t[0, H - 1, 3:5] = 3.0, 3.0
    x[: (M + 1) // 2, 0, 0, 3:5], x[: (M + 1) // 2, 0, H - 1, 4:6] = 3.0, 3.0
    t[1, 1:3, 2:5] = float("nan")
    x[M - 1, 1, H - 1, W - 2] = float("nan")
    return dict(v=x, x=x, t=t, cl=cl, w=cos_weights(H), events=INT_EVENTS, radii=radii_for(H, W), norm=None)


# b. special fields on the smallest grid, M = 9: the perfect forecast (every member equals the truth, a land block included), a field
#    with the event everywhere and one with the event nowhere
SPECIAL_KINDS = ("perfect", "all_event", "no_event")
SPECIAL_SHAPE = (9, 5, 7)


@functools.lru_cache(maxsize=None)
def special_case(kind):
    M, H, W = SPECIAL_SHAPE
    c = integer_case(M, H, W)
    if kind == "perfect":
        t = c["t"].clone()
        x = t.unsqueeze(0).repeat(M, 1, 1, 1)
        return dict(c, v=x, x=x, t=t)
    thr = -10.0 if kind == "all_event" else 10.0
    return dict(c, events=((0, 1, thr, 0), (1, 1, thr, 0), (2, 1, thr, 1)))


# c. two lead times with truth / climatology slots that are not 0 .. L - 1: (M, C, L, H, W) = (9, 3, 2, 5, 7)
MIX_SHAPE = (9, 3, 2, 5, 7)
MIX_T_SLOTS, MIX_C_SLOTS = [5, 2], [3, 0]
N_TRUTH, N_CLIM = R.N_TRUTH, R.N_CLIM


@functools.lru_cache(maxsize=None)
def mix_case():
    M, C, L, H, W = MIX_SHAPE
    g = gen(R._seed(*MIX_SHAPE, 99))
    x = torch.stack([_integer_planes(M, C, H * W, g).reshape(M, C, H, W) for _ in range(L)], 2)
    tt = torch.randint(-1, 4, (N_TRUTH, C, H, W), generator=g).float()
    ct = torch.randint(-1, 2, (N_CLIM, C, H, W), generator=g).float()
    tt[:, 1, 1:3, 2:5] = float("nan")
    return dict(x=x, truth_table=tt, clim_table=ct, w=cos_weights(H), events=INT_EVENTS, radii=radii_for(H, W), t_slots=MIX_T_SLOTS,
                c_slots=MIX_C_SLOTS)


# d. physical scale through the fused inverse normalisation (events_refs.physical_case), M = 50
PHYS_M = 50
PHYS_RADII = (0, 1, 3)

# e. the one large case: (M, E, S, L, H, W) = (50, 2, 4, 2, 120, 240), an SST-like channel with land
BIG_SHAPE = (50, 2, 4, 2, 120, 240)
BIG_RADII = (0, 2, 10, 119)
BIG_C = 2


@functools.lru_cache(maxsize=None)
def big_case():
    M, E, S, L, H, W = BIG_SHAPE
    g = gen(R._seed(*BIG_SHAPE, 101))
    field = torch.nn.functional.avg_pool2d(torch.randn(L, BIG_C, H + 8, W + 8, generator=g), 9, stride=1) * 4.0  # smooth features
    x = (field.unsqueeze(0) + 0.5 * torch.randn(M, L, BIG_C, H, W, generator=g)).permute(0, 2, 1, 3, 4).contiguous().float()
    t = torch.roll(field, shifts=3, dims=-1).float() + 0.3 * torch.randn(L, BIG_C, H, W, generator=g)
    land = torch.nn.functional.avg_pool2d(torch.randn(1, 1, H + 8, W + 8, generator=g), 9, stride=1)[0, 0] > 0.05
    t[:, 1][:, land] = float("nan")
    x[:, 1][:, :, land] = float("nan")
    events = ((0, 1, 0.5, 0), (1, -1, -0.25, 0))
    return dict(x=x, truth_table=t.contiguous(), w=cos_weights(H), events=events, radii=BIG_RADII)


def cpu_cases():
    """the single-lead cases the CPU proofs run over: (name, case)"""
    for M, H, W in INT_CASES:
        yield f"integer M={M} {H}x{W}", integer_case(M, H, W)
    for kind in SPECIAL_KINDS:
        yield f"special {kind}", special_case(kind)
