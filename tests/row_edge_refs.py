"""float64 references, DERIVED per-element bounds, plain-fp32 restatements and the shared case tables of the row / layout / sampler /
DC-AE element-wise kernel edge tests (tests/test_gpu_row_edges.py runs the kernels, tests/test_row_edge_bounds_cpu.py proves on the CPU
that every bound admits a correct fp32 implementation and rejects three planted defects).

Every `*_ref` returns (want, bound) as float64 tensors; every bound is `redzone.elementwise_bound` of a count stated beside it (U =
2**-24 per fp32 rounding, a reduction over k terms counted as k roundings, rsqrt / rcp / exp at their documented ~1 ulp = 2 U), plus
the reduction terms written out where a reduction feeds a later stage.  `*_f32(..., drop=True)` drops one term of the reduction (the first one: a loop
that starts one late; for the sums over rows / pixels the largest row).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests.redzone import TINY, U, act_ref, elementwise_bound


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows_input(batch, rows, width, seed, plain=False):
    """fp32 [batch][rows][width]; NOT iid unless `plain`: each row scaled by 10 ** uniform(-3, 3), one column in 64 by 100"""
    g = gen(seed)
    x = torch.randn(batch, rows, width, generator=g)
    if not plain:
        o = x[..., ::64]
        x[..., ::64] = 100 * (o + torch.sign(o))  # (at least 100 row units, so that the outlier column is one in every row)
        x = x * 10 ** (torch.rand(batch, rows, 1, generator=g) * 6 - 3)
    return x


def vec(n, seed, scale=1.0, rows=1):
    return torch.randn(rows, n, generator=gen(seed)) * scale


# ---- LayerNorm + modulation (ldc_layernorm_mod / _mod2 / ldc_gate_residual_layernorm) -----------------------------------------
def _ln_mul_add(B, R, D, scale, shift, mode, split_row, scale2, shift2):
    """per-row multiplier / addend [B][R][D] (float64) of y = n * mul + add"""
    def one(sc, sh):
        one_ = 1.0 if mode == 0 else 0.0
        mul = torch.full((B, 1, D), 1.0, dtype=torch.float64) if sc is None else (one_ + sc.double().expand(B, D))[:, None]
        add = torch.zeros(B, 1, D, dtype=torch.float64) if sh is None else sh.double().expand(B, D)[:, None]
        return mul.expand(B, R, D), add.expand(B, R, D)
    mul, add = one(scale, shift)
    if split_row is not None and split_row < R:
        m2, a2 = one(scale2, shift2)
        mul, add = mul.clone(), add.clone()
        mul[:, split_row:], add[:, split_row:] = m2[:, split_row:], a2[:, split_row:]
    return mul, add


def layernorm_ref(x, scale=None, shift=None, mode=0, eps=1e-6, split_row=None, scale2=None, shift2=None):
    B, R, D = x.shape
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    mul, add = _ln_mul_add(B, R, D, scale, shift, mode, split_row, scale2, shift2)
    want = xc * rstd * mul + add
    n_term = xc.abs() * rstd * mul.abs()
    # roundings: x - mean, * rstd, 1 + scale, * mul, + add = 5; rstd itself: / D, + eps, rsqrt (1 ulp = 2) = 4; the three per-term
    # roundings of (x - mean)^2 reach rstd halved = 2  -> 11, on S = |x - mean| rstd |mul| + |add|
    bound = elementwise_bound(n_term + add.abs(), 11)
    # reduction terms: the mean is off by at most (D U) mean|x|, which moves every element by that times rstd |mul|; the variance by
    # (D U) var, i.e. rstd by half that, relative
    bound = bound + (D * U) * x.abs().mean(-1, keepdim=True) * rstd * mul.abs() + 0.5 * (D * U) * n_term
    return want, bound


def layernorm_f32(x, scale=None, shift=None, mode=0, eps=1e-6, split_row=None, scale2=None, shift2=None, drop=False):
    B, R, D = x.shape
    x = x.float()
    s = x[..., 1:].sum(-1, keepdim=True) if drop else x.sum(-1, keepdim=True)
    mean = s / D
    xc = x - mean
    rstd = torch.rsqrt((xc * xc).sum(-1, keepdim=True) / D + eps)
    mul, add = _ln_mul_add(B, R, D, scale, shift, mode, split_row, scale2, shift2)
    return xc * rstd * mul.float() + add.float()


# ---- per-head RMSNorm(128) + rotary embedding (ldc_qk_rmsnorm_rope) --------------------------------------------------------------
def qk_rmsnorm_rope_ref(x, w, eps, cos=None, sin=None):
    """x [..., rows, H, 128] fp32, w [128], cos / sin [rows][128] or None"""
    x = x.double()
    ss = (x * x).sum(-1, keepdim=True)
    r = 1 / torch.sqrt(ss / 128 + eps)
    v = x * r * w.double()
    # r: 128-term sum of squares (+1 square each) halved = 65, * (1/128), + eps, rsqrt (2) = 69; v: two products = 71
    bv = elementwise_bound(v.abs(), 71)
    if cos is None:
        return v, bv
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]  # broadcast over heads
    vx, vy = v[..., 0::2], v[..., 1::2]
    bx, by = bv[..., 0::2], bv[..., 1::2]
    ox = vx * c[..., 0::2] - vy * s[..., 0::2]
    oy = vy * c[..., 1::2] + vx * s[..., 1::2]
    # two products and one sum on top of the operands' own error
    box = bx * c[..., 0::2].abs() + by * s[..., 0::2].abs() + elementwise_bound((vx * c[..., 0::2]).abs() + (vy * s[..., 0::2]).abs(), 2)
    boy = by * c[..., 1::2].abs() + bx * s[..., 1::2].abs() + elementwise_bound((vy * c[..., 1::2]).abs() + (vx * s[..., 1::2]).abs(), 2)
    return torch.stack([ox, oy], -1).flatten(-2), torch.stack([box, boy], -1).flatten(-2)


def qk_rmsnorm_rope_f32(x, w, eps, cos=None, sin=None, drop=False):
    x = x.float()
    ss = (x[..., 1:] ** 2).sum(-1, keepdim=True) if drop else (x * x).sum(-1, keepdim=True)
    v = x * torch.rsqrt(ss * (1.0 / 128.0) + eps) * w
    if cos is None:
        return v
    c, s = cos[:, None, :], sin[:, None, :]
    vx, vy = v[..., 0::2], v[..., 1::2]
    return torch.stack([vx * c[..., 0::2] - vy * s[..., 0::2], vy * c[..., 1::2] + vx * s[..., 1::2]], -1).flatten(-2)


# ---- mean over rows (ldc_mean_rows / _split) -----------------------------------------------------------------------------------
def mean_rows_ref(x):
    """x [B][rows][D] -> [B][D]; rows roundings of the sum + the division"""
    rows = x.shape[1]
    x = x.double()
    return x.mean(1), elementwise_bound(x.abs().sum(1) / rows, rows + 1)


def mean_rows_f32(x, drop=False):
    x = x.float()
    if drop:  # the largest row missing from the sum
        x = x.clone()
        x[:, int(x.abs().amax((0, 2)).argmax())] = 0
    return x.sum(1) / x.shape[1]


# ---- gated residual (ldc_gate_residual) ---------------------------------------------------------------------------------------------
def gate_residual_ref(resid, y, gate):
    """resid, y [B][rows][D], gate [B][D]: one fma in the kernel; two roundings admit the unfused form too"""
    p = gate.double()[:, None] * y.double()
    return resid.double() + p, elementwise_bound(resid.double().abs() + p.abs(), 2)


def gate_residual_f32(resid, y, gate):
    return resid + gate[:, None] * y


# ---- timestep embedding (ldc_timestep_embedding, LDC_ACT_IN_TIMESTEP_SINCOS) ----------------------------------------------------------
def timestep_embedding_ref(t):
    """t [n] fp32 -> [n][256] = [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(1e4) k / 128)"""
    k = torch.arange(128, dtype=torch.float64)
    arg = -math.log(1e4) * k / 128
    f = torch.exp(arg)
    a = t.double()[:, None] * f
    want = torch.cat([torch.cos(a), torch.sin(a)], -1)
    # f_k in fp32: the constant and its product with k (2 roundings of an argument of size |arg|: 2 |arg| U absolute = relative in f), / 128
    # exact, expf ~1 ulp (2 U); t * f_k: 1 more -> the angle is off by |t| f_k (2 |arg| + 3) U; cos / sin have slope <= 1; + 2 ulp (4 U) of the result
    da = a.abs() * (2 * arg.abs() + 3) * U
    return want, torch.cat([da, da], -1) + 4 * U * want.abs()


def timestep_embedding_f32(t):
    k = torch.arange(128, dtype=torch.float32)
    f = torch.exp(-9.210340371976184 * k / 128.0)
    a = t.float()[:, None] * f
    return torch.cat([torch.cos(a), torch.sin(a)], -1)


# ---- temb * (1 + scale) + shift (ldc_temb_modulate, the `mod` epilogue of ldc_linear_small_mod) ---------------------------------------
def modulate_ref(v, bv, sc, sh):
    """float64 v with bound bv; 1 + sc, the product and the sum round once each"""
    f = 1 + sc.double()
    p = v * f
    return p + sh.double(), bv * f.abs() + v.abs() * U * (1 + sc.double().abs()) + U * p.abs() + U * (p.abs() + sh.double().abs())


def temb_modulate_ref(temb, te):
    """temb [B][D], te [te_rows][2 D]"""
    B, D = temb.shape
    tr = te[torch.arange(B) % te.shape[0]]
    return modulate_ref(temb.double(), torch.zeros(B, D, dtype=torch.float64), tr[:, :D], tr[:, D:])


def temb_modulate_f32(temb, te):
    B, D = temb.shape
    tr = te[torch.arange(B) % te.shape[0]]
    return temb * (1 + tr[:, :D]) + tr[:, D:]


# ---- small-M linear (ldc_linear_small / _mod / _grouped, VALU kernel) ----------------------------------------------------------------------
ACT_IN_TIMESTEP_SINCOS = 16


def linear_small_ref(x, W, bias, add, rows, act_in, act_out, mod=None):
    """x [x_rows][K] (or [x_rows] timesteps), W [N][K], bias [N] | None, add [add_rows][N] | None, mod [mod_rows][2 N] | None -> [rows][N]"""
    N, K = W.shape
    ridx = torch.arange(rows)
    if act_in == ACT_IN_TIMESTEP_SINCOS:
        xin, bx = timestep_embedding_ref(x)
    else:
        xin, bx = act_ref(x.double(), torch.zeros_like(x, dtype=torch.float64), act_in)
    xin, bx = xin[ridx % xin.shape[0]], bx[ridx % bx.shape[0]]
    Wd = W.double()
    dot = xin @ Wd.T
    s_dot = xin.abs() @ Wd.abs().T
    b = torch.zeros(N, dtype=torch.float64) if bias is None else bias.double()
    pre = dot + b
    # K products + K sums in the chain (K + 1), + bias (1); the staged input's own error passes through |W|
    bpre = elementwise_bound(s_dot + b.abs(), K + 2) + bx @ Wd.abs().T
    v, bv = act_ref(pre, bpre, act_out)
    if add is not None:
        a = add.double()[ridx % add.shape[0]]
        bv = bv + U * (v.abs() + a.abs())
        v = v + a
    if mod is not None:
        m = mod[ridx % mod.shape[0]]
        v, bv = modulate_ref(v, bv, m[:, :N], m[:, N:])
    return v, bv


def _act_f32(v, act):
    """the library's activations as it writes them (csrc/common.h), in fp32 torch: v / (1 + 2^t) - torch's own tanh form of GELU cancels
    1 + tanh(u) at negative v and is only absolutely, not relatively, accurate there"""
    if act == 1:
        return v * (1 / (1 + torch.exp2(-1.4426950408889634 * v)))
    if act == 2:
        c0 = torch.tensor(-2.0 * 0.7978845608028654 * 1.4426950408889634, dtype=torch.float32)
        return v * (1 / (1 + torch.exp2(v * (c0 + c0 * 0.044715 * v * v))))
    return v.clamp_min(0) if act == 3 else v


def linear_small_f32(x, W, bias, add, rows, act_in, act_out, mod=None, drop=False):
    N, K = W.shape
    ridx = torch.arange(rows)
    xin = timestep_embedding_f32(x) if act_in == ACT_IN_TIMESTEP_SINCOS else _act_f32(x.float(), act_in)
    xin = xin[ridx % xin.shape[0]]
    v = (xin[:, 1:] @ W[:, 1:].T) if drop else xin @ W.T
    if bias is not None:
        v = v + bias
    v = _act_f32(v, act_out)
    if add is not None:
        v = v + add[ridx % add.shape[0]]
    if mod is not None:
        m = mod[ridx % mod.shape[0]]
        v = v * (1 + m[:, :N]) + m[:, N:]
    return v


# ---- RMSNorm rows (ldc_rmsnorm_rows / _split) ----------------------------------------------------------------------------------------------
def rmsnorm_rows_ref(x, w, b, resid, eps, act):
    """x [rows][C], w / b [C], resid [rows][C] | None"""
    C = x.shape[-1]
    x = x.double()
    r = 1 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    t = x * r * w.double()
    o = t.clone()
    s = t.abs()
    if b is not None:
        o, s = o + b.double(), s + b.double().abs()
    if resid is not None:
        o, s = o + resid.double(), s + resid.double().abs()
    # r: C-term sum of squares (+1 square each) halved, / C, + eps, rsqrt (2): (C + 1) / 2 + 4; x r w: 2; + b, + resid: 2
    return act_ref(o, elementwise_bound(s, (C + 1) / 2 + 8), act)


def rmsnorm_rows_f32(x, w, b, resid, eps, act, drop=False):
    C = x.shape[-1]
    ss = (x[..., 1:] ** 2).sum(-1, keepdim=True) if drop else (x * x).sum(-1, keepdim=True)
    o = x * torch.rsqrt(ss / C + eps) * w
    if b is not None:
        o = o + b
    if resid is not None:
        o = o + resid
    return _act_f32(o, act)


# ---- DC-AE shuffles with a group mean (ldc_pixel_unshuffle_shortcut, ldc_chan_regroup down) -------------------------------------------------
def pixel_unshuffle_nhwc(t):
    """[B][2 H2][2 W2][c] -> [B][H2][W2][4 c], channel 4 c + 2 i + j <- pixel (2 h2 + i, 2 w2 + j)"""
    return F.pixel_unshuffle(t.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)


def pixel_unshuffle_shortcut_ref(cv, x, cout):
    """cv [B][2 H2][2 W2][cout / 4], x [B][2 H2][2 W2][cin] | None -> [B][H2][W2][cout]"""
    a = pixel_unshuffle_nhwc(cv.double())
    if x is None:
        return a, torch.zeros_like(a)
    xs = pixel_unshuffle_nhwc(x.double())
    G = xs.shape[-1] // cout
    g = xs.reshape(*xs.shape[:-1], cout, G)
    # G sums, the division, the add
    return a + g.mean(-1), elementwise_bound(a.abs() + g.abs().sum(-1) / G, G + 2)


def pixel_unshuffle_shortcut_f32(cv, x, cout, drop=False):
    a = pixel_unshuffle_nhwc(cv)
    xs = pixel_unshuffle_nhwc(x)
    G = xs.shape[-1] // cout
    g = xs.reshape(*xs.shape[:-1], cout, G)
    return a + (g[..., :-1] if drop else g).sum(-1) / G


def chan_regroup_down_ref(x, cout):
    G = x.shape[-1] // cout
    g = x.double().reshape(*x.shape[:-1], cout, G)
    return g.mean(-1), elementwise_bound(g.abs().sum(-1) / G, G + 1)


def chan_regroup_down_f32(x, cout, drop=False):
    G = x.shape[-1] // cout
    g = x.reshape(*x.shape[:-1], cout, G)
    return (g[..., :-1] if drop else g).sum(-1) / G


# ---- grouped 1 x 1 conv, 32 channels per group (ldc_grouped_conv1x1_nhwc) ---------------------------------------------------------------------
def grouped_conv1x1_ref(x, wt):
    """x [M][groups * 32], wt [groups * 32][32]: a 32-term fma chain per output"""
    M = x.shape[0]
    groups = wt.shape[0] // 32
    xg, wg = x.double().reshape(M, groups, 32), wt.double().reshape(groups, 32, 32)
    y = torch.einsum("mgi,goi->mgo", xg, wg).reshape(M, groups * 32)
    s = torch.einsum("mgi,goi->mgo", xg.abs(), wg.abs()).reshape(M, groups * 32)
    return y, elementwise_bound(s, 32)


def grouped_conv1x1_f32(x, wt, drop=False):
    M = x.shape[0]
    groups = wt.shape[0] // 32
    xg, wg = x.reshape(M, groups, 32), wt.reshape(groups, 32, 32)
    if drop:
        xg, wg = xg[..., :-1], wg[..., :-1]
    return torch.einsum("mgi,goi->mgo", xg, wg).reshape(M, groups * 32)


# ---- ReLU linear attention (ldc_relu_linear_attn_nhwc) --------------------------------------------------------------------------------------------
def relu_linear_attn_ref(qkv, groups, eps):
    """qkv [B][P][>= groups * 96] -> y [B][P][groups * 32]"""
    B, P = qkv.shape[:2]
    t = qkv.double()[..., : groups * 96].reshape(B, P, groups, 96)
    q, k, v = t[..., :32].clamp_min(0), t[..., 32:64].clamp_min(0), t[..., 64:]
    kv = torch.einsum("bpgc,bpgj->bgcj", v, k)
    kva = torch.einsum("bpgc,bpgj->bgcj", v.abs(), k)
    ks = k.sum(1)  # [B][g][j]
    num = torch.einsum("bgcj,bpgj->bpgc", kv, q)
    numa = torch.einsum("bgcj,bpgj->bpgc", kva, q)
    den = torch.einsum("bgj,bpgj->bpg", ks, q)[..., None] + eps
    y = num / den
    # numerator: P terms per KV entry (+1 product), 32 terms of the second contraction (+1): P + 34 on sum |v| k q; the denominator (all terms
    # >= 0): P + 32 + 1 (+ eps) relative, and the reciprocal and the product: 3 more - all on S = sum |v| k q / den >= |y|
    return y.reshape(B, P, groups * 32), elementwise_bound(numa / den, 2 * P + 70).reshape(B, P, groups * 32)


def relu_linear_attn_f32(qkv, groups, eps, drop=False):
    B, P = qkv.shape[:2]
    t = qkv[..., : groups * 96].reshape(B, P, groups, 96)
    q, k, v = t[..., :32].clamp_min(0), t[..., 32:64].clamp_min(0), t[..., 64:]
    if drop:  # the largest pixel missing from the KV sum
        v = v.clone()
        v[:, int(v.abs().amax((0, 2, 3)).argmax())] = 0
    kv, ks = torch.einsum("bpgc,bpgj->bgcj", v, k), k.sum(1)
    num = torch.einsum("bgcj,bpgj->bpgc", kv, q)
    den = torch.einsum("bgj,bpgj->bpg", ks, q)[..., None] + eps
    return (num * (1.0 / den)).reshape(B, P, groups * 32)


# ---- depthwise sphere conv (ldc_sphere_dwconv_nhwc) against oracle.sphere_conv in float64 ------------------------------------------------------------
def _oracle_dwconv(x_nchw, w, bias, ks):
    """oracle.sphere_conv.SphereConv2d (depthwise) in the dtype of its arguments.  H = 2 leaves the class's middle band (rows 1 .. H - 2) empty,
    which F.conv2d refuses; there the top and bottom rows - the whole output - are taken with the class's own padding and kernel flips."""
    from oracle.sphere_conv import SphereConv2d, sphere_pad

    C, p = x_nchw.shape[1], ks // 2
    if x_nchw.shape[2] > 2:
        m = SphereConv2d(C, C, ks, padding=p, groups=C, bias=bias is not None).to(x_nchw.dtype)
        with torch.no_grad():
            m.weight.copy_(w)
            if bias is not None:
                m.bias.copy_(bias)
            return m(x_nchw)
    xp = sphere_pad(x_nchw, (p, p))
    w_top = torch.cat([torch.flip(w[:, :, :p, :], dims=[3]), w[:, :, p:, :]], dim=2)
    w_bot = torch.cat([w[:, :, :-p, :], torch.flip(w[:, :, -p:, :], dims=[3])], dim=2)
    return torch.cat([F.conv2d(xp[:, :, :ks, :], w_top, bias, groups=C), F.conv2d(xp[:, :, -ks:, :], w_bot, bias, groups=C)], dim=2)


def sphere_dwconv_ref(x, wt, bias, ks, glu, dtype=torch.float64):
    """x [B][H][W][C] NHWC, wt [ks * ks][C], bias [C] | None -> (y [B][H][W][C or C / 2], bound)"""
    C = x.shape[-1]
    w = wt.to(dtype).T.reshape(C, 1, ks, ks)
    xn = x.to(dtype).permute(0, 3, 1, 2)
    b = None if bias is None else bias.to(dtype)
    d = _oracle_dwconv(xn, w, b, ks).permute(0, 2, 3, 1)
    if dtype != torch.float64:
        return (d[..., : C // 2] * F.silu(d[..., C // 2:]) if glu else d), None
    s = _oracle_dwconv(xn.abs(), w.abs(), None if b is None else b.abs(), ks).permute(0, 2, 3, 1)
    bd = elementwise_bound(s, ks * ks + 1)  # one fma per tap on top of the bias
    if not glu:
        return d, bd
    a0, a1, b0, b1 = d[..., : C // 2], d[..., C // 2:], bd[..., : C // 2], bd[..., C // 2:]
    g, bg = act_ref(a1, b1, 1)
    return a0 * g, a0.abs() * bg + g.abs() * b0 + U * (a0 * g).abs() + TINY


def sphere_dwconv_f32(x, wt, bias, ks, glu, drop=False):
    if drop:  # the last tap missing
        wt = wt.clone()
        wt[-1] = 0
    return sphere_dwconv_ref(x, wt, bias, ks, glu, dtype=torch.float32)[0]


# =================================================================================================================================
# Case tables of the kernels judged by a bound, and the builders of their seeded inputs (shared by the GPU and the CPU file).
# "refused" rows live in the GPU file, next to the error code they assert.
# =================================================================================================================================
def _seed(*k):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31)


# (B, rows, D, mode, scale given, shift given, kind)   kind: "scaled" | "plain" | "mean1e4"
LN_CASES = (
    [(1, r, D, 0, True, True, "scaled") for D in (4, 8, 252, 256, 260, 2044, 2048) for r in (1, 5)]
    + [(3, r, 260, m, True, True, "scaled") for r in (3, 4) for m in (0, 1)]
    + [(3, 5, 8, 1, sc, sh, "scaled") for sc in (False, True) for sh in (False, True)]
    + [(1, 3, 2044, 0, False, True, "scaled"), (1, 4, 252, 0, True, False, "scaled"), (3, 5, 256, 0, True, True, "plain"),
       (1, 3, 8, 1, True, True, "mean1e4")]
)


def ln_inputs(B, rows, D, mode, has_sc, has_sh, kind):
    s = _seed(B, rows, D, mode, has_sc, has_sh)
    x = rows_input(B, rows, D, s, plain=kind != "scaled")
    nb = B if mode == 0 else 1
    sc = vec(D, s + 1, rows=nb) if has_sc else None
    sh = vec(D, s + 2, rows=nb) if has_sh else None
    if kind == "mean1e4":  # row mean 1e4, std 1: the mean's D U mean|x| term is 5e-3 absolute, so the case carries a shift of +-50 .. 150, whose
        x = x + 1e4        # own roundings (and any defect in them) stay visible beside it
        sh = torch.sign(sh) * (50 + 100 * torch.rand(nb, D, generator=gen(s + 3)))
    return dict(x=x, scale=sc, shift=sh, mode=mode, eps=1e-6)


# (rows, H, row0, rope, plain)
QK_CASES = [(1, 1, 0, False, False), (1, 3, 2, True, False), (3, 1, 1, True, False), (3, 3, 2, False, False), (3, 3, 0, True, True)]


def qk_inputs(rows, H, row0, rope, plain, B=2):
    s = _seed(rows, H, row0, rope, 5)
    tot = row0 + rows + 1  # rows before row0 and one after stay untouched
    qkv = rows_input(B, tot, 3 * H * 128, s, plain=plain)
    wq, wk = vec(128, s + 1)[0], vec(128, s + 2)[0]
    cos = sin = None
    if rope:
        ang = torch.rand(rows, 64, generator=gen(s + 3)) * 6.28
        cos, sin = torch.cos(ang).repeat_interleave(2, 1).contiguous(), torch.sin(ang).repeat_interleave(2, 1).contiguous()
    return dict(qkv=qkv, wq=wq, wk=wk, cos=cos, sin=sin, eps=1e-6)


MEAN_ROWS = (1, 15, 16, 17, 63, 64, 65, 113)
MEAN_CASES = [(2, r, D, "scaled") for r in MEAN_ROWS for D in (8, 72)] + [(1, r, D, "scaled") for r in (17, 113) for D in (4, 64, 136)] + [(2, 65, 64, "plain")]


def mean_inputs(B, rows, D, kind):
    return rows_input(B, rows, D, _seed(B, rows, D, 11), plain=kind == "plain")


# (B, rows, D, in place, plain)
GATE_CASES = [(B, r, D, ip, False) for D in (4, 1020, 1024, 1028) for (B, r, ip) in ((1, 1, False), (3, 2, True))] + [(3, 2, 1028, False, True)]


def gate_inputs(B, rows, D, inplace, plain):
    s = _seed(B, rows, D, 13)
    return dict(resid=rows_input(B, rows, D, s, plain), y=rows_input(B, rows, D, s + 1, plain), gate=vec(D, s + 2, rows=B))


TIMESTEPS = (0.0, 1e-4, -1.55, 1.1, 999.0)
ACTS = (0, 1, 2, 3)
# (rows, x_rows, add_rows, N, K, act_in, act_out, bias, mod_rows)   add_rows 0: no add; mod_rows 0: no mod; act_in 16: timestep sinusoid (K = 256)
LS_CASES = (
    [(r, r, 1, N, 260, 0, 0, True, 0) for N in (1, 3, 4, 5, 15, 16, 17) for r in (1, 9)]
    + [(r, r, r, 5, K, 0, 0, True, 0) for K in (4, 252, 256, 260, 2048, 2052, 4100) for r in (7, 8)]
    + [(9, 2, 4, 17, 2052, 1, 0, False, 0), (7, 3, 2, 3, 4100, 0, 1, True, 0), (8, 1, 8, 16, 256, 0, 0, False, 0), (1, 1, 0, 1, 4, 0, 0, False, 0)]
    + [(7, 7, 3, 5, 252, ai, ao, True, 0) for ai in ACTS for ao in ACTS]
    + [(5, 5, 1, 17, 256, ACT_IN_TIMESTEP_SINCOS, ao, True, 0) for ao in (0, 1)]
    + [(r, xr, 1, N, K, 1, 0, True, mr) for (r, xr, N, K, mr) in ((1, 1, 5, 260, 1), (9, 9, 17, 2052, 2), (5, 1, 4, 256, 5))]
)


def ls_inputs(rows, x_rows, add_rows, N, K, act_in, act_out, has_bias, mod_rows):
    s = _seed(rows, x_rows, add_rows, N, K, act_in, act_out, has_bias, mod_rows)
    if act_in == ACT_IN_TIMESTEP_SINCOS:
        x = torch.tensor(TIMESTEPS).flip(0)[:x_rows].clone()  # (999 first: neighbouring rows differ)
    else:
        x = rows_input(1, x_rows, K, s, plain=act_in != 0)[0]  # (an activation of a 1e3-scaled row only saturates: unit rows reach its curved part)
        if act_in:  # the activation tails
            x[0, 0], x[-1, min(1, K - 1)] = 30.0, -30.0
    W = vec(K, s + 1, rows=N, scale=1 / math.sqrt(K))
    if K >= 2048:  # K + 2 worst-case roundings on sum |W x|: with signed terms the bound outgrows a bf16 rounding of the result, so the long
        W = W.abs()  # rows run without cancellation (sum |W x| = |sum W x|)
        if act_in != ACT_IN_TIMESTEP_SINCOS:
            x = x.abs()
    bias = vec(N, s + 2)[0] if has_bias else None
    if has_bias and act_out:  # outputs at the tails of act_out: a bias that dwarfs the product
        bias[0] = 30.0 if N == 1 else -30.0
        bias[-1] = 30.0
    add = vec(N, s + 3, rows=add_rows) if add_rows else None
    mod = vec(2 * N, s + 4, rows=mod_rows) if mod_rows else None
    return dict(x=x, W=W, bias=bias, add=add, rows=rows, act_in=act_in, act_out=act_out, mod=mod)


TEMB_CASES = [(B, te, D) for B in (1, 5) for te in (1, 2, 5) if te <= B or te == 2 for D in (4, 260)]


def temb_inputs(B, te_rows, D):
    s = _seed(B, te_rows, D, 17)
    return dict(temb=rows_input(1, B, D, s)[0], te=vec(2 * D, s + 1, rows=te_rows))


# (rows, C, act, bias, resid, kind)
RMS_CASES = (
    [(r, C, 0, True, True, "scaled") for C in (4, 8, 12, 1020, 1024, 1028, 2044, 2048) for r in (1, 5)]
    + [(3, C, 1, True, True, "scaled") for C in (12, 1028)] + [(3, 12, 0, False, False, "scaled"), (5, 1028, 1, True, False, "plain"), (3, 1028, 3, True, True, "plain")]
)


def rms_inputs(rows, C, act, has_b, has_r, kind):
    s = _seed(rows, C, act, has_b, has_r, 19)
    return dict(x=rows_input(1, rows, C, s, plain=kind == "plain")[0], w=vec(C, s + 1)[0], b=vec(C, s + 2)[0] if has_b else None,
                resid=rows_input(1, rows, C, s + 3, plain=True)[0] if has_r else None, eps=1e-5, act=act)


# (B, H2, W2, cout, cin)    cin None: no shortcut
UNSHUF_CASES = [(1, 1, 1, 4, 1), (1, 1, 2, 12, 3), (2, 3, 5, 12, 6), (1, 3, 5, 20, 15), (2, 3, 5, 12, 12), (1, 1, 2, 12, None), (2, 3, 5, 4, None)]


def unshuf_inputs(B, H2, W2, cout, cin):
    s = _seed(B, H2, W2, cout, cin or 0, 23)
    cv = rows_input(B, 4 * H2 * W2, cout // 4, s).reshape(B, 2 * H2, 2 * W2, cout // 4)
    x = None if cin is None else rows_input(B, 4 * H2 * W2, cin, s + 1).reshape(B, 2 * H2, 2 * W2, cin)
    return dict(cv=cv, x=x, cout=cout)


REGROUP_DOWN = [(1, 4, 4), (2, 12, 4), (15, 12, 4), (15, 8, 2), (3, 12, 3)]  # (M, cin, cout): group factors 1, 3, 3, 4, 4
GCONV_CASES = [(M, g) for M in (1, 63, 64, 65) for g in (1, 3)]


def gconv_inputs(M, groups):
    s = _seed(M, groups, 29)
    return dict(x=rows_input(1, M, groups * 32, s)[0], wt=vec(32, s + 1, rows=groups * 32, scale=0.2))


RLA_P = (1, 31, 33, 127, 129, 1023, 1024, 1025, 1151, 1153)
# (B, P, groups, kind)   kind: "scaled" | "plain" | "zero_q" (one pixel's relu(q) all zero) | "zero_k" (group 0's relu(k) all zero)
RLA_CASES = [(1 + i % 2, P, 1 + (i // 2) % 2, "scaled") for i, P in enumerate(RLA_P)] + [(2, 33, 2, "zero_q"), (1, 129, 2, "zero_k"), (2, 127, 1, "plain")]


def rla_inputs(B, P, groups, kind):
    s = _seed(B, P, groups, 31)
    # every pixel row scaled would make q's scale cancel in the quotient only; the scaling that matters is per pixel on k and v
    qkv = rows_input(B, P, groups * 96, s, plain=kind == "plain")
    if kind == "zero_q":
        qkv[0, P // 2, :32] = -qkv[0, P // 2, :32].abs()
    if kind == "zero_k":
        qkv[:, :, 32:64] = -qkv[:, :, 32:64].abs()
    return qkv


# (B, H, W, C, ks, glu, bias)   untiled kernel: W < 8 + ks - 1; tiled: W >= 8 + ks - 1
DW_CASES = (
    [(1, H, W, 4, 3, False, True) for W in (2, 4, 8) for H in (2, 3)] + [(2, 3, 4, 12, 5, False, False), (1, 2, 8, 8, 5, True, True), (1, 3, 10, 8, 5, False, True)]
    + [(1, H, W, 12, 3, False, True) for W in (10, 12, 14, 18) for H in (2, 5)] + [(2, 5, 12, 8, 5, False, True), (1, 2, 14, 4, 5, False, False),
                                                                                 (1, 5, 18, 16, 5, True, True), (2, 2, 10, 8, 3, True, False), (1, 3, 4, 16, 3, True, True)]
)


def dw_inputs(B, H, W, C, ks, glu, has_bias):
    s = _seed(B, H, W, C, ks, glu, 37)
    return dict(x=rows_input(B, H * W, C, s).reshape(B, H, W, C), wt=vec(C, s + 1, rows=ks * ks, scale=0.3), bias=vec(C, s + 2)[0] if has_bias else None,
                ks=ks, glu=glu)
