"""float64 oracle, COUNTED bound, an fp32 restatement (with planted defects) and the case tables of the zonal-spectrum kernel
(csrc/spectrum.hip: ldc_rollout_spectrum).  tests/test_gpu_spectrum.py runs the kernel; tests/test_spectrum_cpu.py proves on the CPU that
the bound admits a correct fp32 implementation in the kernel's order and that every planted defect is caught.  numpy throughout.

Definitions, per row of W points with positive weight, for a real sequence y (a member x_i, the ensemble mean
m = fp32 member-order sum / M, the truth t; all fp32 values, after `inv_norm_f32` where the inverse normalisation is fused):
    Y_k = sum_j y_j exp(-2 pi i j k / W), k = 0 .. W / 2;  P_k(y) = s_k |Y_k|^2 / W^2, s_0 = s_{W/2} = 1, s_k = 2 otherwise
    spec_members = <(1 / M) sum_i P_k(x_i)>, spec_mean = <P_k(m)>, spec_truth = <P_k(t)>, <.> = sum_h w_h (.) / sum_h w_h over valid rows
    a row is valid when w_h > 0 and none of its (M + 1) W member and truth values is NaN; n_invalid counts the rows with w_h > 0 left out
The oracle is numpy.fft.rfft in float64 of those fp32 values; m is formed as the kernel forms it, so both transform the same sequence.

The bound, first order in U = 2**-24, counted from spectrum.hip's arithmetic, nothing fitted.  For one row and one sequence y with
exact mean mu and residual r_j = y_j - mu, V = mean_j r_j^2:
  mean    lane t adds its pairs y_p + y_{W-p} (1 addition) for p = t, t + 64, ... (KB + 1 additions, KB = ceil(W / 128)), a 6-step butterfly,
          one division: N_MU = KB + 9 roundings, |d_mu| <= N_MU U mean_j |y_j|.  P_0 = mu^2: |dP_0| <= 2 |mu| d_mu + d_mu^2.
  k >= 1  a constant shift of the pivot leaves Y_k (k >= 1) unchanged in exact arithmetic, but the kernel's roundings are relative to
          the residual about ITS pivot, so the scale is sqrt(V') = sqrt(V) + d_mu.  Per bin: 1 rounding in y_j - pivot, 1 in the fold
          (e = ra + rb, o = ra - rb), 1 in the fp32 twiddle, and n = W / 2 + 1 fused multiply-adds in index order: to first order
          |dRe_k| <= g sum_p |e_p c_pk|, |dIm_k| <= g sum_p |o_p s_pk| with g = (n + 3) U.  By Cauchy-Schwarz with sum_p c^2, sum_p s^2 <=
          W / 4 + 1 and sum_p (e_p^2 + o_p^2) <= 2 W V':  |dY_k| <= g W sqrt(V') sqrt(1 / 2 + 2 / W) <= g W sqrt(V') for W >= 4, i.e. for the
          amplitude a_k = Y_k / W:  |da_k| <= g sqrt(V'),  and  |dP_k| <= s_k (2 |a_k| g sqrt(V') + g^2 V').
          |Y_k|^2 is formed in fp64 from the fp32 Re / Im (exact products), sums over members and rows are fp64.
  average the weighted mean of the rows' (and members') bounds, plus 2 U |result|: the fp64 sums and quotient (~1e-16 relative, far
          below U) and the one rounding to fp32.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -24
RPW = 8  # spectrum.hip: rows per workgroup = rows per workspace record; H > 8 exercises the finish launch's merge
NAMES = ("spec_members", "spec_mean", "spec_truth")
MAX_M, MIN_W, MAX_W = 1024, 4, 512
f32, f64 = np.float32, np.float64


def kb_of(W):
    return -(-(W // 2) // 64)


def n_mu(W):
    return kb_of(W) + 9


def gamma(W):
    return (W // 2 + 1 + 3) * U


def workspace_bytes(M, C, L, H, W):
    return 4096 + 8 * L * C * (-(-H // RPW)) * (2 + 3 * (W // 2 + 1))


def s_k(W):
    s = np.full(W // 2 + 1, 2.0)
    s[0] = s[-1] = 1.0
    return s


def inv_norm_f32(v, mean, std, target_std):
    """(v / target_std) * std[c] + mean[c] on the channel axis 1, every operation rounded to fp32 (csrc/ensemble_common.h: inv_norm)"""
    shape = [1, -1] + [1] * (v.ndim - 2)
    q = v.astype(f32) if target_std == 1.0 else (v.astype(f32) / f32(target_std)).astype(f32)
    return ((q * std.astype(f32).reshape(shape)).astype(f32) + mean.astype(f32).reshape(shape)).astype(f32)


def ens_mean_f32(x):
    """x (M, ...) fp32 -> the fp32 member-order sum divided by M, as the kernel (and ldc_rollout_reliability) forms it"""
    s = np.zeros(x.shape[1:], f32)
    for i in range(x.shape[0]):
        s = (s + x[i]).astype(f32)
    return (s / f32(x.shape[0])).astype(f32)


def valid_rows(x, t, w):
    """-> (valid (C, L, H) bool, n_invalid (C, L) int64)"""
    pos = (w > 0)[None, None, :]
    nan = np.isnan(x).any(axis=(0, -1)) | np.isnan(t).any(axis=-1)
    return pos & ~nan, (pos & nan).sum(-1).astype(np.int64)


# ---- float64 oracle with the bound ----------------------------------------------------------------------------------------------------
def _seq_power_and_bound(y):
    """y (..., W) fp32 (NaN allowed: such rows are masked by the caller) -> (P, bound) (..., K) float64"""
    W = y.shape[-1]
    y = np.nan_to_num(y.astype(f64), nan=0.0)
    Y = np.fft.rfft(y, axis=-1)
    s = s_k(W)
    a = np.abs(Y) / W
    P = s * a * a
    mu = y.mean(-1, keepdims=True)
    d_mu = n_mu(W) * U * np.abs(y).mean(-1, keepdims=True)
    rv = np.sqrt(((y - mu) ** 2).mean(-1, keepdims=True)) + d_mu
    g = gamma(W)
    b = s * (2 * a * g * rv + g * g * rv * rv)
    b[..., :1] = 2 * np.abs(mu) * d_mu + d_mu * d_mu
    return P, b


def _average(P, b, w, valid):
    """P, b (C, L, H, K), w (H,), valid (C, L, H) -> (value, bound) (C, L, K); no valid row: NaN"""
    wv = w.astype(f64)[None, None, :] * valid
    den = wv.sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = (P * wv[..., None]).sum(-2) / den[..., None]
        bnd = (b * wv[..., None]).sum(-2) / den[..., None] + 2 * U * np.abs(val)
    none = ~valid.any(-1)
    val[none], bnd[none] = np.nan, np.nan
    return val, bnd


def spectrum_ref(x, t, w):
    """x (M, C, L, H, W) the fp32 values the kernel transforms, t (C, L, H, W), w (H,) -> dict: each of NAMES a (value, bound) pair of
    (C, L, K) float64; n_invalid (C, L) int64"""
    x, t, w = np.asarray(x, f32), np.asarray(t, f32), np.asarray(w, f32)
    valid, n_inv = valid_rows(x, t, w)
    Pm, bm = _seq_power_and_bound(x)
    out = dict(spec_members=_average(Pm.mean(0), bm.mean(0), w, valid), spec_mean=_average(*_seq_power_and_bound(ens_mean_f32(x)), w, valid),
               spec_truth=_average(*_seq_power_and_bound(t), w, valid), n_invalid=n_inv)
    return out


def mean_square_ref(x, t, w):
    """Parseval's other side in float64: the weighted mean over the valid rows of mean_j y_j^2 -> (3, C, L)"""
    x, t, w = np.asarray(x, f32), np.asarray(t, f32), np.asarray(w, f32)
    valid, _ = valid_rows(x, t, w)
    wv = w.astype(f64)[None, None, :] * valid

    def ms(y):
        return (np.nan_to_num(y.astype(f64)) ** 2).mean(-1)

    with np.errstate(invalid="ignore"):
        return np.stack([(q * wv).sum(-1) / wv.sum(-1) for q in (ms(x).mean(0), ms(ens_mean_f32(x)), ms(t))])


def ratio_of(got, ref):
    """worst |got - value| / bound over the elements (NaN must meet NaN; a non-finite `got` where the value is finite: inf)"""
    got, (val, bnd) = np.asarray(got, f64), ref
    assert got.shape == val.shape, (got.shape, val.shape)
    both_nan = np.isnan(got) & np.isnan(val)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - val) / np.maximum(bnd, 1e-300)
    r = np.where(got == val, 0.0, r)
    r = np.where(both_nan, 0.0, np.where(np.isfinite(r), r, np.inf))
    return float(r.max()) if r.size else 0.0


def check(got, ref, what=""):
    """got {spec_members, spec_mean, spec_truth (C, L, K), n_invalid (C, L)} against spectrum_ref's dict: the counts equal, every value
    within its bound; returns the worst err / bound ratio.  Raises AssertionError."""
    gn = np.asarray(got["n_invalid"]).astype(np.int64)
    assert np.array_equal(gn, ref["n_invalid"]), f"{what}: n_invalid {gn.tolist()} != {ref['n_invalid'].tolist()}"
    worst = 0.0
    for k in NAMES:
        r = ratio_of(got[k], ref[k])
        assert r <= 1.0, f"{what}: {k} misses its bound: worst err / bound {r:.4g}"
        worst = max(worst, r)
    return worst


# ---- the kernel's arithmetic in fp32 numpy, with planted defects ------------------------------------------------------------------------
DEFECTS = ("unpivoted", "nyquist_2", "s_1", "mean_of_spectra", "nan_row_kept", "zero_row_read", "fold_drops_half")


def twiddle_table(W):
    """(cos, sin)(2 pi i / W), i < W: float64 values (exact at the multiples of a quarter turn, as sincospi) rounded to fp32"""
    i = np.arange(W)
    c, s = np.cos(2 * np.pi * i / W), np.sin(2 * np.pi * i / W)
    for q, (cv, sv) in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1))):
        if (q * W) % 4 == 0:
            c[q * W // 4], s[q * W // 4] = cv, sv
    return c.astype(f32), s.astype(f32)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in float64"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _seq_sums_f32(y, defect):
    """y (..., W) fp32 -> |Y_k|^2 (..., K) float64 as spectrum_kernel forms it"""
    W = y.shape[-1]
    half, K = W // 2, W // 2 + 1
    lead = y.shape[:-1]
    # pair sums per lane in index order, butterfly over the 64 lanes, one division
    npair = -(-K // 64) * 64
    ya = np.zeros(lead + (npair,), f32)
    yb = np.zeros(lead + (npair,), f32)
    ya[..., :K] = y[..., :K]
    yb[..., 1:half] = y[..., :half:-1]
    part = np.zeros(lead + (64,), f32)
    for r in range(npair // 64):
        part = (part + (ya[..., 64 * r:64 * r + 64] + yb[..., 64 * r:64 * r + 64]).astype(f32)).astype(f32)
    o = 32
    while o:
        part = (part + part[..., np.arange(64) ^ o]).astype(f32)
        o >>= 1
    mu = (part[..., :1] / f32(W)).astype(f32)
    pivot = np.zeros_like(mu) if defect == "unpivoted" else mu
    ra, rb = (ya[..., :K] - pivot).astype(f32), (yb[..., :K] - pivot).astype(f32)
    paired = (np.arange(K) > 0) & (np.arange(K) < half)
    e = np.where(paired, (ra + rb).astype(f32), ra)
    od = np.where(paired, (ra - rb).astype(f32), f32(0))
    ct, st = twiddle_table(W)
    k = np.arange(K)
    re, im = np.zeros(lead + (K,), f32), np.zeros(lead + (K,), f32)
    for p in range(K):
        if defect == "fold_drops_half" and p == half:
            continue
        idx = (p * k) % W
        re = _fma(e[..., p:p + 1], ct[idx], re)
        im = _fma(od[..., p:p + 1], st[idx], im)
    p2 = re.astype(f64) ** 2 + im.astype(f64) ** 2
    p2[..., 0] = (mu[..., 0].astype(f64) * W) ** 2
    return p2


def kernel_f32(x, t, w, defect=None):
    """spectrum_kernel + spectrum_finish_kernel restated: the fp32 mean, residual, fold and fused multiply-adds in index order, fp64 power
    and sums (rows in order inside a record of RPW rows, then the records in order).  -> {NAMES: (C, L, K) fp32, n_invalid}.  Planted defects:
      unpivoted: the raw row is transformed;  nyquist_2: s_k = 2 at k = W / 2;  s_1: s_k = 1 everywhere;  mean_of_spectra: spec_mean is
      spec_members;  nan_row_kept: a row with a NaN enters the sums;  zero_row_read: a row of weight 0 enters the sums with its weight;
      fold_drops_half: the fold leaves out p = W / 2"""
    assert defect in (None,) + DEFECTS
    x, t, w = np.asarray(x, f32), np.asarray(t, f32), np.asarray(w, f32)
    M, C, L, H, W = x.shape
    K = W // 2 + 1
    valid, n_inv = valid_rows(x, t, w)
    if defect == "nan_row_kept":
        valid = np.broadcast_to((w > 0)[None, None, :], valid.shape)
    if defect == "zero_row_read":
        valid = valid | np.broadcast_to((w == 0)[None, None, :], valid.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        pm = np.zeros((C, L, H, K), f64)
        for i in range(M):
            pm = pm + _seq_sums_f32(x[i], defect)
        planes = [pm, _seq_sums_f32(ens_mean_f32(x), defect), _seq_sums_f32(t, defect)]
        if defect == "mean_of_spectra":
            planes[1] = pm / M
        s = np.ones(K) if defect == "s_1" else s_k(W)
        if defect == "nyquist_2":
            s[-1] = 2.0
        out = {}
        wd = w.astype(f64)
        for name, p2, div in zip(NAMES, planes, (float(M), 1.0, 1.0)):
            tot, wsum = np.zeros((C, L, K), f64), np.zeros((C, L), f64)
            for r0 in range(0, H, RPW):
                rt, rw = np.zeros((C, L, K), f64), np.zeros((C, L), f64)
                for h in range(r0, min(r0 + RPW, H)):
                    v = valid[:, :, h]
                    rt = rt + np.where(v[..., None], wd[h] * p2[:, :, h], 0.0)
                    rw = rw + np.where(v, wd[h], 0.0)
                tot, wsum = tot + rt, wsum + rw
            val = s * tot / (div * float(W) * float(W) * wsum[..., None])
            val[~valid.any(-1)] = np.nan
            out[name] = val.astype(f32)
    out["n_invalid"] = n_inv
    return out


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# (M, C, L, H, W): one row at the smallest W; W / 2 odd; a small general case; the workload's W; the largest W (four bins per lane);
# more members than a 64-member register arm would hold (the kernel walks blocks of 8 sequences: 72 = 9 blocks);
# 37 rows = 5 workspace records of RPW = 8 rows, the last with 5: the finish launch's merge
SHAPES = ((1, 1, 1, 1, 4), (2, 2, 1, 3, 6), (3, 2, 2, 3, 8), (3, 1, 1, 2, 240), (1, 1, 1, 1, 512), (70, 1, 1, 2, 8), (2, 1, 1, 37, 16))
OFFSETS = (0.0, 280.0, 5.0e4)  # channel means: none, a temperature, a geopotential
SCALES = (1.0, 12.0, 900.0)


def row_weights(H):
    """cos-like, positive, not normalised to anything convenient"""
    return (0.25 + np.cos(np.linspace(-1.2, 1.3, H))).astype(f32)


@functools.lru_cache(maxsize=None)
def case(shape, seed=0):
    """-> dict x (M, C, L, H, W), t (C, L, H, W), w (H,): members = truth + noise around a channel offset (read-only: shared by the tests)"""
    M, C, L, H, W = shape
    g = np.random.RandomState(1000 * seed + 17 * M + 5 * H + W)
    off = np.array([OFFSETS[c % 3] for c in range(C)]).reshape(C, 1, 1, 1)
    sc = np.array([SCALES[c % 3] for c in range(C)]).reshape(C, 1, 1, 1)
    t = (off + sc * g.standard_normal((C, L, H, W))).astype(f32)
    x = (t[None] + 0.5 * sc * g.standard_normal((M, C, L, H, W))).astype(f32)
    out = dict(x=x, t=t, w=row_weights(H))
    for v in out.values():
        v.setflags(write=False)
    return out


# defect (a): a large mean under a small amplitude near the Nyquist wavenumber.  The issue names mean 2e5 and amplitude 1e-2 at k0 = W / 2 - 1.
# The ulp of 2e5 is 1.6e-2, so the fp32 input already holds the tone only as a pattern of -1 / 0 / +1 ulp; the oracle transforms that fp32
# input, and its own P_k0 (7.6e-5 for the truth at W = 240, about 2900 x the pivoted bound of 2.6e-8; test_spectrum_cpu.py asserts the
# factor 100) is what the kernel must return.  The mean therefore stays at the issue's 2e5; nothing had to be lowered.
PIVOT_MEAN, PIVOT_AMP, PIVOT_W = 2.0e5, 1.0e-2, 240


@functools.lru_cache(maxsize=None)
def pivot_case():
    M, C, L, H, W = 2, 1, 1, 2, PIVOT_W
    j = np.arange(W)
    k0 = W // 2 - 1
    tone = PIVOT_AMP * np.cos(2 * np.pi * k0 * j / W)
    t = (PIVOT_MEAN + tone).astype(f32).reshape(1, 1, 1, W).repeat(H, axis=2)
    x = np.stack([t, (PIVOT_MEAN + 1.5 * tone).astype(f32).reshape(1, 1, 1, W).repeat(H, axis=2)])
    out = dict(x=x, t=t, w=np.ones(H, f32), k0=k0)
    for v in (out["x"], out["t"], out["w"]):
        v.setflags(write=False)
    return out


def nan_case(zero_weight_row):
    """the (3, 2, 2, 3, 8) case with a NaN in member 1 of row 1 of (c, l) = (1, 0); `zero_weight_row`: that row's weight is 0"""
    c = case((3, 2, 2, 3, 8))
    x, w = c["x"].copy(), c["w"].copy()
    x[1, 1, 0, 1, 5] = np.nan
    if zero_weight_row:
        w[1] = 0.0
    return dict(x=x, t=c["t"], w=w)


def pure_tone(W, k0, A, B, H=2):
    """rows holding exactly A cos(2 pi k0 j / W) + B (rounded to fp32) -> (y (H, W), the expected spectrum (K,))"""
    j = np.arange(W)
    y = (A * np.cos(2 * np.pi * k0 * j / W) + B).astype(f32)
    want = np.zeros(W // 2 + 1)
    want[0] = B * B
    want[k0] = A * A if k0 == W // 2 else A * A / 2
    return np.broadcast_to(y, (H, W)).copy(), want


def torch_composition_f32(x, t, w):
    """what a torch composition does: torch.fft.rfft in fp32 on the raw fields, the reductions in fp32 -> {NAMES: (C, L, K) fp32}"""
    import torch

    x, t, w = torch.from_numpy(np.array(x)), torch.from_numpy(np.array(t)), torch.from_numpy(np.array(w))
    return torch_composition(x, t, w)


def torch_composition(x, t, w):
    """tensors on any device; rows with NaN are not handled (the timing and accuracy comparison runs on clean data)"""
    import torch

    W = x.shape[-1]
    s = torch.full((W // 2 + 1,), 2.0, device=x.device)
    s[0] = s[-1] = 1.0
    wv = (w / w.sum()).view(-1, 1)

    def spec(y):
        return ((torch.fft.rfft(y, dim=-1).abs() ** 2) * (s / (W * W)) * wv).sum(-2)

    return dict(spec_members=spec(x).mean(0), spec_mean=spec(x.mean(0)), spec_truth=spec(t))
