"""float64 references, DERIVED per-element bounds, fp32 restatements (with planted defects) and the shared case tables of the
matrix-core kernel edge tests: the ring GEMM in its three arithmetics, the register-staged stream-K GEMM, both attentions and the
sphere convs.  tests/test_gpu_mfma_edges.py runs the kernels; tests/test_mfma_edge_bounds_cpu.py proves on the CPU that every bound
admits a correct fp32 implementation with chunked accumulation and rejects the planted defects.

Every bound is `n * 2**-24 * S_i` (redzone.elementwise_bound): S_i the float64 sum of the absolute terms of element i, n counted from
the arithmetic below.  Nothing here is fitted to what a kernel returns.

GEMM  C = epilogue(A . W^T)
  exact fp32 ("f32"): terms a_k w_k.  The fp32 MFMA adds one product per step to the accumulator: K roundings.  A tile whose k range is
    cut is summed from its pieces (the planner, csrc/gemm_plan.hip, cuts a tile into at most 8 aligned pieces, an unaligned range adds one): + 9.  Bias: + 1.
    n = K + 10 on S = sum_k |a w| + |bias|.
  "bf16x3": the mode's own definition on the split operands, ah.wh + ah.wl + al.wh (hi = bf16(x), lo = bf16(x - hi)).  A product of two
    bf16 values has 16 significant bits and is exact in fp32, so only the accumulation rounds: n = 3 K + 10 on the sum of the three
    absolute products + |bias|.
  "bf16" (single term): ah.wh alone, n = K + 10.
  Epilogue, propagated: act through redzone.act_ref; gate: |gate| times the bound + one rounding of the product; residual: one
  rounding of the sum.

Attention  O = softmax(q k^T + bias) v, per (batch, head), scores in log2 units (q carries log2(e) / sqrt(128))
  Three sources, as the kernels compute (attn_f32.hip, attn_split.hip):
  (1) score error over the 128-term dot.  fp32 kernel: q * qscale (1 rounding, the constant itself a rounded product of two rounded
      constants: 3 more), 128 accumulations, the bias term bias * log2(e)f and its add (3): n_s = 135.  Split kernels: the products are
      exact, the accumulator starts from bias * log2(e)f (2) and takes `terms` x 128 additions: n_s = 128 terms + 2.
      ds_j = n_s U T_j,  T_j = sum |q k| (all terms) + |bias_j| log2(e).
  (2) through exp2: p_j = exp2(s_j - m).  The subtraction rounds once (U |s_j - m|), v_exp_f32 is 1 ulp (2 U):
      eps_j = ln 2 (ds_j + U (|s_j - m_row| + lazy)) + 2 U, relative, m_row the row's true maximum: a running maximum never exceeds it.
      lazy = 8 for the split kernels, whose running maximum only moves when a tile beats it by more than 8 (so p <= 2**8 and the
      argument is at most 8 larger in magnitude); 0 for the fp32 kernel.
      A weight error that is relative passes to O as sum_j eps_j w_j |v_jd - O_d| (first order; x 1.01 covers the second order at
      eps < 1e-2): the normaliser is summed from the same p_j, so a common factor cancels.
  (3) the S-term sums.  P.V: terms x S accumulations + 1 (fp32 product); the row sum l: S; every change of the running maximum
      multiplies O and l by exp2(m_old - m_new): 3 roundings (the subtraction's U |dm| ln 2 summed over the changes is at most
      U ln 2 (max_j s - min_j s)); at most ceil(S / 32) + 10 changes (one per key tile, the merge of the two key groups, the pieces of a
      balanced cut); 1 / l and the product: 2.   n_o = (terms + 1) S + 3 (ceil(S / 32) + 10) + 3, + ln 2 (max s - min s), on
      N_d = sum_j w_j |v_jd|.
  P quantisation (split kernels; the row sum l is taken from the fp32 p, so this does NOT cancel).  bf16 keeps 8 significant bits:
      round-to-nearest is off by at most 2**-8 relative.  Three-term: P = ph + pl with |p - ph - pl| <= 2**-16 p, and the dropped
      pl.vl <= 2**-16 p |v|: 2**-15 N_d.  Single-term: ph alone: 2**-8 N_d.
  exp2 results under the smallest normal are flushed to zero: + S 2**-126 max |v|.
  Nothing above had to be taken from a measured sensitivity.

Convs: the GEMM bound with K = ks * ks * cin_padded on the float64 sphere conv of oracle/sphere_conv.py (the zero taps of a padded cin
add no error but are counted: the bound only grows).

The tile-per-workgroup kernel of gemm_f32.hip (ldc_gemm_bias_act, ldc_sphere_conv_nhwc) sums a tile in one piece, K products in k order:
the same n = K + 10 holds it (the 9 pieces are counted though it has none).  Its conv at H = 2, where oracle/sphere_conv.py and the
reference raise, is DEFINED by the float64 gather-GEMM over sphere_gather (conv_ref(via_gather=True)), which equals the oracle conv
wherever that exists.
"""
from __future__ import annotations

import functools
import math

import torch

from tests.redzone import TINY, U, act_ref, elementwise_bound
from tests.row_edge_refs import _act_f32, gen, rows_input, vec

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
QSCALE = LOG2E / math.sqrt(128.0)
MODES = ("f32", "bf16x3", "bf16")
KSTEP = {"f32": 32, "bf16x3": 32, "bf16": 64}
PIECES = 9


def split_hi_lo(x):
    """fp32 -> (hi, lo) as fp32: hi = bf16(x) RNE, lo = bf16(x - hi)"""
    x = x.float()
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def gemm_terms(A, W, mode):
    """the (a, w) operand pairs (fp32 tensors holding the values the matrix core multiplies) of `mode`"""
    if mode == "f32":
        return [(A.float(), W.float())]
    ah, al = split_hi_lo(A)
    wh, wl = split_hi_lo(W)
    return [(ah, wh), (ah, wl), (al, wh)] if mode == "bf16x3" else [(ah, wh)]


def epilogue_ref(pre, bpre, act=0, gate=None, R=None):
    """float64 (value, bound) of act -> * gate[b][n] -> + R on top of a pre-activation with bound bpre ([B][M][N])"""
    v, bv = act_ref(pre, bpre, act)
    if gate is not None:
        g = gate.double()[:, None, :]
        v, bv = v * g, bv * g.abs() + U * (v * g).abs()
    if R is not None:
        r = R.double()
        bv = bv + U * (v.abs() + r.abs())
        v = v + r
    return v, bv


def gemm_ref(A, W, bias=None, gate=None, R=None, act=0, mode="f32"):
    """A [B][M][K], W [N][K], bias [N], gate [B][N], R [B][M][N] -> float64 (C, bound) [B][M][N]"""
    K = A.shape[-1]
    dot = s = 0
    terms = gemm_terms(A, W, mode)
    for a, w in terms:
        dot = dot + a.double() @ w.double().T
        s = s + a.double().abs() @ w.double().abs().T
    b = torch.zeros(W.shape[0], dtype=torch.float64) if bias is None else bias.double()
    return epilogue_ref(dot + b, elementwise_bound(s + b.abs(), len(terms) * K + PIECES + 1), act, gate, R)


def gemm_f32(A, W, bias=None, gate=None, R=None, act=0, mode="f32", cuts=(), drop_kstep=None, drop_lohi_panel=None, last_row_from_prev=False,
             piece_twice=False, stale_stage=False):
    """The kernels' arithmetic in fp32 torch: per 128 x 128 tile an fp32 accumulator that takes one k-step (32, or 64 single-term, values of
    every term) at a time; `cuts` (k-step indices) end a piece, the pieces are summed in order.  Planted defects:
      drop_kstep = (bm, bn, kt): that k-step of that tile is skipped;  drop_lohi_panel = bn: the al.wh term is missing in column panel bn;
      last_row_from_prev: row M - 1 is computed from row M - 2 of A;  piece_twice: the first piece of tile (0, 0) is added twice;
      stale_stage: k-step kt >= 2 multiplies the operands of k-step kt - 2 (a double-buffered LDS stage read before it was refilled)."""
    B, M, K = A.shape
    N = W.shape[0]
    ks = KSTEP[mode]
    terms = gemm_terms(A, W, mode)
    if last_row_from_prev and M > 1:
        terms = [(torch.cat([a[:, :-1], a[:, -2:-1]], 1), w) for a, w in terms]
    out = torch.zeros(B, M, N)
    for bm in range(0, M, 128):
        for bn in range(0, N, 128):
            pieces, acc = [], torch.zeros(B, min(128, M - bm), min(128, N - bn))
            for kt in range(K // ks + (1 if K % ks else 0)):
                if kt in cuts:
                    pieces.append(acc)
                    acc = torch.zeros_like(acc)
                if drop_kstep == (bm // 128, bn // 128, kt):
                    continue
                src = kt - 2 if stale_stage and kt >= 2 else kt
                k0, k1 = src * ks, min(K, src * ks + ks)
                for ti, (a, w) in enumerate(terms):
                    if ti == 2 and drop_lohi_panel == bn // 128:
                        continue
                    acc = acc + a[:, bm:bm + 128, k0:k1] @ w[bn:bn + 128, k0:k1].T
            pieces.append(acc)
            if piece_twice and bm == 0 and bn == 0:
                pieces.insert(0, pieces[0])
            tot = pieces[0]
            for p in pieces[1:]:
                tot = tot + p
            out[:, bm:bm + 128, bn:bn + 128] = tot
    v = out if bias is None else out + bias
    v = _act_f32(v, act)
    if gate is not None:
        v = v * gate[:, None, :]
    if R is not None:
        v = v + R
    return v


# ---- GEMM cases -------------------------------------------------------------------------------------------------------------------
GEMM_M = (1, 127, 128, 129, 257)
GEMM_N = (8, 120, 128, 136, 260)
GEMM_N_SCALAR = 133  # N % 4 != 0: the scalar epilogue (not with C in operand rows)
GEMM_K = {"f32": (32, 64, 288), "bf16x3": (32, 64, 288), "bf16": (64, 128, 320)}  # single-term: its own k-step, 2 BK = 64
GEMM_K_REGSTAGE = 36  # K % 32 != 0: a ragged last k-step, register-staged kernel only
# epilogue variants, one per (M, N) pair in turn: (bias, gate, residual: None | "inplace" | "separate", act, column offset)
EPILOGUES = ((True, False, None, 0, 0), (True, True, "inplace", 1, 0), (True, False, "separate", 2, 0), (False, False, None, 0, 8),
             (True, True, "separate", 3, 0))  # (the last one: ReLU launders NaN - a value-only case)


def _seed(*k):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K, batch, epi, mode):
    """seeded operands (rows of A scaled by 10 ** U(-2, 2): a row taken from its neighbour is far outside the bound); single-term mode: A
    holds bf16 values (its operand rows are plain bf16)"""
    has_bias, has_gate, res, act, col0 = EPILOGUES[epi]
    s = _seed(M, N, K, batch, epi)
    g = gen(s)
    A = torch.randn(batch, M, K, generator=g) * 10 ** (torch.rand(batch, M, 1, generator=g) * 4 - 2)
    if mode == "bf16":
        A = A.bfloat16().float()
    W = vec(K, s + 1, rows=N, scale=1 / math.sqrt(K))
    bias = vec(N, s + 2)[0] if has_bias else None
    gate = vec(N, s + 3, rows=batch) if has_gate else None
    R = rows_input(batch, M, N, s + 4, plain=True) if res else None
    return dict(A=A, W=W, bias=bias, gate=gate, R=R, act=act)


@functools.lru_cache(maxsize=None)
def gemm_case_ref(M, N, K, batch, epi, mode):
    return gemm_ref(mode=mode, **gemm_inputs(M, N, K, batch, epi, mode))


def gemm_shapes(mode, regstage=False):
    """(M, N, K, batch, epilogue variant) of every GEMM case of `mode`: M x N (+ the scalar-epilogue N) x K, batch and epilogue taking turns
    (2 and 5 are coprime: every pair occurs); regstage: + the ragged K of the register-staged kernel"""
    i = 0
    for K in GEMM_K[mode] + ((GEMM_K_REGSTAGE,) if regstage else ()):
        for M in GEMM_M:
            for N in GEMM_N + (GEMM_N_SCALAR,):
                i += 1
                yield M, N, K, (1, 3)[i % 2], i % len(EPILOGUES)


# the tile-per-workgroup kernel of gemm_f32.hip (ldc_gemm_bias_act): 4 = one float4 in one ragged k-tile; 36 = one whole tile and a ragged one of
# a single float4; 64 = two tiles, both LDS stages; 84 = the embedders' depth; 96 = three tiles, stage 0 reused
TILE_GEMM_K = (4, 36, 64, 84, 96)
TILE_GEMM_N = (5,) + GEMM_N + (GEMM_N_SCALAR,)


def tile_gemm_shapes(K=None):
    """(M, N, K, batch, epilogue variant) of every case of the tile-per-workgroup GEMM (mode "f32"), batch and epilogue taking turns as in
    gemm_shapes; K: only the cases of that depth (the turns are those of the whole table)"""
    i = 0
    for k in TILE_GEMM_K:
        for M in GEMM_M:
            for N in TILE_GEMM_N:
                i += 1
                if K is None or k == K:
                    yield M, N, k, (1, 3)[i % 2], i % len(EPILOGUES)


def sweep_K(mode, k32):
    """K of a sweep problem of k32 k-steps; capped at 768 (the single-term mode's 64-wide k-step then gives the single-tile problem 12
    k-steps, which the planner leaves whole: that mode's pieces come from the 3 x 3 problem and the group)"""
    return min(k32 * KSTEP[mode], 768)


# cut sweep: (name, [(M, N, K32, batch)])  K32: the depth in 32-wide k-steps (the single-term mode runs twice the K for the same k-steps,
# capped by sweep_K).  What the planner (csrc/gemm_plan.hip) does with each on the ring kernel is SWEEP_CUTS below, which
# test_streamk_cut_sweep asserts on `hip.gemm_plan` of the very problems it launches; why, per entry:
SWEEP_PROBLEMS = {
    "3x3 tiles, 9 k-steps": [(300, 260, 9, 1)],
    # one tile, 24 k-steps: the few-tiles branch cuts it into 3 aligned pieces of 8 k-steps on the exact-fp32 and bf16x3 ring kernels; the
    # register-staged kernels' U / sqrt(c kt) rule gives 3 ranges too.  NOT in the single-term mode: sweep_K caps it at 12 k-steps there,
    # which no rule cuts (G = 1 for every g: that mode's nine entries of this problem are one launch, repeated).
    "single tile, 24 k-steps": [(128, 128, 24, 1)],
    # unequal depths: the exact-fp32 ring and the register-staged kernels launch it as ONE group (unaligned ranges that cross the problem
    # boundary).  The split ring modes (bf16x3 with split A, single-term) never do: without a common depth there is no aligned cut and the
    # planner gives each problem a launch of its own - in those modes this entry sweeps two single launches.
    "two problems, 9 and 2 k-steps": [(300, 260, 9, 1), (129, 136, 2, 2)],
    # equal depth 16 (9 + 8 = 17 tiles): the few-tiles rule cuts at s = 2 (34 aligned ranges) and keeps the group whole on the exact-fp32 and
    # the bf16x3 ring kernel; smaller g: unaligned ranges across the problem boundary.  Single-term mode: capped at 12 k-steps, no s with
    # kt / s >= 8 - launched one by one again; its whole group is the next entry.
    "two problems, 16 k-steps each": [(300, 260, 16, 1), (129, 136, 16, 2)],
    # equal depth 2, 80 + 80 = 160 tiles: `best` = 160 whole-tile ranges, which EVERY ring mode keeps as one group (best >= 160); the limited
    # workspace then cuts U = 320 units into g ranges that cross tiles, batches and the problem boundary (unit0 / tile0 of the second
    # problem, urem in either)
    "two problems, 2 k-steps each, 160 tiles": [(1279, 1020, 2, 1), (639, 1020, 2, 2)],
}
# workgroups of each launch the planner makes of the set with the full workspace, per arithmetic of the ring kernel
SWEEP_CUTS = {
    "3x3 tiles, 9 k-steps": {"f32": [10], "bf16x3": [10], "bf16": [10]},
    "single tile, 24 k-steps": {"f32": [3], "bf16x3": [3], "bf16": [1]},
    "two problems, 9 and 2 k-steps": {"f32": [13], "bf16x3": [10, 4], "bf16": [10, 4]},
    "two problems, 16 k-steps each": {"f32": [34], "bf16x3": [34], "bf16": [10, 9]},
    "two problems, 2 k-steps each, 160 tiles": {"f32": [160], "bf16x3": [160], "bf16": [160]},
}
SWEEP_G = (1, 2, 3, 4, 5, 7, 10, 13, 20, 32, 40, 160)  # (the register-staged kernel picks 32 for the unequal group, every kernel 160 for the last)


# ---- attention ----------------------------------------------------------------------------------------------------------------------
ATTN_MODES = {"f32": dict(terms=1, n_s=135, lazy=0.0, pq=0.0), "split3": dict(terms=3, n_s=3 * 128 + 2, lazy=8.0, pq=2.0 ** -15),
              "split1": dict(terms=1, n_s=128 + 2, lazy=8.0, pq=2.0 ** -8)}
ATTN_S = (1, 31, 32, 33, 64, 65, 127, 128, 129, 257)
BIAS_KINDS = ("none", "middle tile negligible", "maximum in the last key", "key in the ragged last tile")


# more (query block, head, batch) units than CUs: 2 x 13 x 10 = 260 units of 5 key tiles.  Without a workspace the exact-fp32 attention runs its
# 4-wave form (two workgroups per CU); with one, its balanced cut (260 % 256 != 0, 1300 items >= 512: 256 ranges of 5 or 6 tiles, most units
# in two pieces, merged by the last arriver); the split attention its persistent form with 4 tail units in 5 key slices each and the merge launch
ATTN_SCHEDULE_CASE = (129, 129, 13, 10, "key in the ragged last tile")  # (S, Sq, H, B, bias kind)


def attn_combos(S):
    """(Sq, H, B, bias kind) run at every S"""
    return [(S, 1, 1, "none"), (S, 3, 2, "middle tile negligible"), (max(S - 1, 1), 1, 2, "maximum in the last key"), (1, 3, 1, "key in the ragged last tile")]


def key_bias(S, kind):
    if kind == "none":
        return None
    b = 0.5 * torch.randn(S, generator=gen(_seed(S, 41)))
    nt = (S + 31) // 32
    if kind == "middle tile negligible":  # exp2 of these underflows to exactly 0 in fp32
        lo, hi = (32 * (nt // 2), min(S, 32 * (nt // 2) + 32)) if nt > 1 else (0, S // 2)
        b[lo:hi] = -200.0
    elif kind == "maximum in the last key":  # every tile before the last one is rescaled
        b[S - 1] = 20.0
    else:
        b[32 * ((S - 1) // 32)] = 3.0
    return b


@functools.lru_cache(maxsize=None)
def attn_inputs(B, S, H):
    """fp32 q (x 2: a peaked softmax), k, v [B][S][H][128]"""
    g = gen(_seed(B, S, H, 43))
    q, k, v = (torch.randn(B, S, H, 128, generator=g) for _ in range(3))
    return 2.0 * q, k, v * 10 ** (torch.rand(B, S, 1, 1, generator=g) * 2 - 1)


def attn_qs(q):
    """q in log2 units as the split producers write it: two fp32 products"""
    return q * torch.tensor(0.08838834764831845, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)


def attn_operand_rows(q, k, v):
    """int32 bit image [B][S][3 H 128] of the fused operand rows of ldc_attn_fwd_split: q, k as 16 groups of [hi x8 | lo x8] bf16 per head,
    v as [hi x128 | lo x128]"""
    from tests.redzone import FMT_SPLIT, operand_rows

    B, S, H, _ = q.shape
    vh, vl = split_hi_lo(v)
    vi = torch.cat([vh.bfloat16(), vl.bfloat16()], -1).contiguous().view(torch.int32)  # [B][S][H][128]
    return torch.cat([operand_rows(attn_qs(q), FMT_SPLIT).reshape(B, S, H * 128), operand_rows(k, FMT_SPLIT).reshape(B, S, H * 128), vi.reshape(B, S, H * 128)], -1)


def attn_operands(q, k, v, mode):
    """what the kernel multiplies, as fp32 tensors: ([(q part, k part)], [v parts]); q in log2 units.  f32: the exact product q * QSCALE is
    formed in float64 by the reference (the kernel's own rounding of it is counted in n_s); split modes: the operand rows the producer
    writes - q * fp32(QSCALE) rounded to fp32, then split"""
    if mode == "f32":
        return [(q, k)], [v]
    qh, ql = split_hi_lo(attn_qs(q))
    kh, kl = split_hi_lo(k)
    vh, vl = split_hi_lo(v)
    if mode == "split3":
        return [(qh, kh), (qh, kl), (ql, kh)], [vh, vl]
    return [(qh, kh)], [vh]


def attn_ref(q, k, v, bias, Sq, mode):
    """q, k, v fp32 [B][S][H][128], bias [S] | None -> float64 (O, bound) [B][Sq][H * 128]"""
    cfg = ATTN_MODES[mode]
    B, S, H, _ = q.shape
    qk, vs = attn_operands(q, k, v, mode)
    sc = QSCALE if mode == "f32" else 1.0
    s = t = 0
    for qp, kp in qk:
        qd, kd = qp.double().permute(0, 2, 1, 3)[:, :, :Sq] * sc, kp.double().permute(0, 2, 1, 3)
        s = s + qd @ kd.transpose(-1, -2)
        t = t + qd.abs() @ kd.abs().transpose(-1, -2)
    if bias is not None:
        s, t = s + bias.double() * LOG2E, t + bias.double().abs() * LOG2E
    vd = sum(x.double() for x in vs).permute(0, 2, 1, 3)  # [B][H][S][128]
    m = s.amax(-1, keepdim=True)
    w = torch.softmax(s * LN2, -1)
    O = w @ vd
    eps = LN2 * (cfg["n_s"] * U * t + U * ((s - m).abs() + cfg["lazy"])) + 2 * U
    ew = eps * w
    first = torch.empty_like(O)
    for b in range(B):
        for h in range(H):
            first[b, h] = torch.einsum("qj,qjd->qd", ew[b, h], (vd[b, h][None] - O[b, h][:, None]).abs())
    nd = w @ vd.abs()
    n_o = (cfg["terms"] + 1) * S + 3 * ((S + 31) // 32 + 10) + 3
    rng = s.amax(-1, keepdim=True) - s.amin(-1, keepdim=True)
    bound = 1.01 * first + (n_o * U + LN2 * U * rng + cfg["pq"]) * nd + S * TINY * vd.abs().amax()
    return O.permute(0, 2, 1, 3).reshape(B, Sq, H * 128), bound.permute(0, 2, 1, 3).reshape(B, Sq, H * 128)


def attn_f32(q, k, v, bias, Sq, mode, skip_tile=None, ignore_bias_key=None):
    """online softmax over 32-key tiles in fp32 torch, P quantised as the mode does.  Planted defects: skip_tile: that key tile is left out;
    ignore_bias_key: that key's bias is not added."""
    B, S, H, _ = q.shape
    qk, vs = attn_operands(q, k, v, mode)
    if mode == "f32":
        qk = [(q * torch.tensor(QSCALE, dtype=torch.float32), k)]
    perm = lambda x: x.permute(0, 2, 1, 3)  # noqa: E731
    m = torch.full((B, H, Sq, 1), -1.0e30)
    l = torch.zeros(B, H, Sq, 1)
    o = torch.zeros(B, H, Sq, 128)
    for t0 in range(0, S, 32):
        if skip_tile == t0 // 32:
            continue
        t1 = min(S, t0 + 32)
        if bias is None:
            s = torch.zeros(B, H, Sq, t1 - t0)
        else:
            bb = bias[t0:t1].clone()
            if ignore_bias_key is not None and t0 <= ignore_bias_key < t1:
                bb[ignore_bias_key - t0] = 0.0
            s = (bb * torch.tensor(LOG2E, dtype=torch.float32)).expand(B, H, Sq, t1 - t0).clone()
        for qp, kp in qk:
            s = s + perm(qp)[:, :, :Sq] @ perm(kp)[:, :, t0:t1].transpose(-1, -2)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new)
        p = torch.exp2(s - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha
        if mode == "f32":
            o = o + p @ perm(vs[0])[:, :, t0:t1]
        else:
            ph, pl = split_hi_lo(p)
            o = o + ph @ perm(vs[0])[:, :, t0:t1]
            if mode == "split3":
                o = o + ph @ perm(vs[1])[:, :, t0:t1] + pl @ perm(vs[0])[:, :, t0:t1]
        m = m_new
    return perm(o * (1.0 / l)).reshape(B, Sq, H * 128)


# ---- sphere convs ---------------------------------------------------------------------------------------------------------------------
def conv_cin_padded(cin, cpk=32):
    p = cpk
    while p < cin:
        p *= 2
    return p


def _oracle_conv(x_nchw, w, bias, ks):
    """oracle.sphere_conv.SphereConv2d (dense, stride 1) in the dtype of its arguments"""
    from oracle.sphere_conv import SphereConv2d

    cout, cin = w.shape[:2]
    if ks == 1:  # (no padding, no kernel rows to flip: the class's slices by -0 are empty there)
        return torch.nn.functional.conv2d(x_nchw, w, bias)
    m = SphereConv2d(cin, cout, ks, padding=ks // 2, bias=bias is not None).to(x_nchw.dtype)
    with torch.no_grad():
        m.weight.copy_(w)
        if bias is not None:
            m.bias.copy_(bias)
        return m(x_nchw)


def _gather_conv(x_nchw, w, ks):
    """float64 sphere conv as the gather-GEMM: sum over taps and channels of sphere_gather(x) . w, defined index by index at any H >= 2"""
    cout, cin = w.shape[:2]
    g = sphere_gather(x_nchw.permute(0, 2, 3, 1), ks)  # [B][H][W][ks * ks][cin]
    return torch.einsum("bhwtc,otc->bohw", g, w.permute(0, 2, 3, 1).reshape(cout, ks * ks, cin))


def conv_ref(x, w, bias, ks, mode, act=0, R=None, via_gather=False):
    """x [B][H][W][cin] NHWC fp32, w [cout][cin][ks][ks], bias [cout] | None, R [B][H][W][cout] | None -> float64 (y, bound) NHWC: the float64
    sphere conv of every term of `mode`, the GEMM bound with K = ks * ks * padded cin.  via_gather: the float64 gather-GEMM over
    sphere_gather instead of oracle/sphere_conv.py - the two agree at every H >= 3 (judged on the CPU); at H = 2, where the oracle and the
    reference both raise (their middle slice has fewer than ks rows), the gather IS the definition"""
    conv = (lambda a, ww, b, k: _gather_conv(a, ww, k)) if via_gather else _oracle_conv
    xn = x.permute(0, 3, 1, 2)
    if mode == "f32":
        terms = [(xn.float(), w.float())]
    else:
        xh, xl = split_hi_lo(xn)
        wh, wl = split_hi_lo(w)
        terms = [(xh, wh), (xh, wl), (xl, wh)] if mode == "bf16x3" else [(xh, wh)]
    y = s = 0
    for a, ww in terms:
        y = y + conv(a.double(), ww.double(), None, ks)
        s = s + conv(a.double().abs(), ww.double().abs(), None, ks)
    cout, cin = w.shape[:2]
    b = torch.zeros(cout, dtype=torch.float64) if bias is None else bias.double()
    y, s = y.permute(0, 2, 3, 1) + b, s.permute(0, 2, 3, 1) + b.abs()
    K = ks * ks * conv_cin_padded(cin, KSTEP[mode])
    B, H, W_ = x.shape[:3]
    v, bv = epilogue_ref(y.reshape(1, B * H * W_, cout), elementwise_bound(s, len(terms) * K + PIECES + 1).reshape(1, B * H * W_, cout), act, None,
                         None if R is None else R.reshape(1, B * H * W_, cout))
    return v.reshape(B, H, W_, cout), bv.reshape(B, H, W_, cout)


def sphere_gather(x, ks, wrap_wrong_side=False, no_pole_roll=False, no_pole_flip=False, tile_first_image=False):
    """x [B][H][W][C] -> [B][H][W][ks * ks][C]: the source pixel of every tap under the sphere padding rule, written out index by index
    (rows past a pole: mirrored and rolled by W / 2; columns wrap; the oracle's flipped kernel rows at the poles are this gather).
    Planted defects:  wrap_wrong_side: the column that wraps around is taken from the side it is on - clamped instead of wrapped;
      no_pole_roll: a row past a pole is mirrored but not shifted by W / 2;  no_pole_flip: the kx flip at rows 0 and H - 1 is missing;
      tile_first_image: a pixel gathers from the image that holds the first pixel of its 128-row tile (one image base per tile)."""
    B, H, W_, C = x.shape
    p = ks // 2
    h, ky, kx = torch.arange(H)[:, None, None, None], torch.arange(ks)[None, None, :, None], torch.arange(ks)[None, None, None, :]
    flip = ((h == 0) & (ky < p)) | ((h == H - 1) & (ky >= ks - p))  # at the two pole rows the kernel rows over the pole are flipped left-right
    kx = kx.expand(H, 1, ks, ks) if no_pole_flip else torch.where(flip, ks - 1 - kx, kx.expand(H, 1, ks, ks))
    hh = (h + ky - p).expand(H, W_, ks, ks)
    ww = (torch.arange(W_)[None, :, None, None] + kx - p).expand(H, W_, ks, ks)
    over = (hh < 0) | (hh >= H)
    hs = torch.where(hh < 0, -1 - hh, torch.where(hh >= H, 2 * H - 1 - hh, hh))
    ws = ww if no_pole_roll else torch.where(over, ww + W_ // 2, ww)
    ws = ws.clamp(0, W_ - 1) if wrap_wrong_side else ws % W_
    if tile_first_image:
        pix = torch.arange(B * H * W_).reshape(B, H, W_)
        img = (pix // 128 * 128 // (H * W_))[..., None, None]
        return x[img, hs, ws].reshape(B, H, W_, ks * ks, C)
    return x[:, hs, ws].reshape(B, H, W_, ks * ks, C)


def conv_f32(x, w, bias, ks, mode, act=0, R=None, **defects):
    """the implicit GEMM in fp32: gathered rows [pix][tap][cin] . W[cout][tap][cin], through gemm_f32's chunked accumulation; defects: the
    planted defects of sphere_gather"""
    B, H, W_, cin = x.shape
    cout = w.shape[0]
    cp = conv_cin_padded(cin, KSTEP[mode])
    a = torch.zeros(B, H, W_, ks * ks, cp)
    a[..., :cin] = sphere_gather(x, ks, **defects)
    wt = torch.zeros(cout, ks * ks, cp)
    wt[..., :cin] = w.permute(0, 2, 3, 1).reshape(cout, ks * ks, cin)
    y = gemm_f32(a.reshape(1, B * H * W_, ks * ks * cp), wt.reshape(cout, ks * ks * cp), bias, None, None if R is None else R.reshape(1, B * H * W_, cout),
                 act, mode)
    return y.reshape(B, H, W_, cout)


# (B, H, W, cin, cout, ks, residual): cin tails 40 / 28, ragged output panels 136 / 86, two frames
CONV_CASES = [(2, 4, 8, 40, 136, 3, True), (2, 3, 6, 28, 86, 5, False), (2, 5, 4, 40, 86, 1, True), (2, 6, 12, 28, 136, 3, False)]
# the tile-per-workgroup conv of gemm_f32.hip (ldc_sphere_conv_nhwc), each with act 0 and 1:
TILE_CONV_CASES = [
    (2, 4, 8, 40, 136, 3, True),  # 64 pixels: both images in one 128-row tile; cin 40 = two k-tiles per tap, the second ragged; ragged output panel
    (3, 6, 12, 28, 136, 3, False),  # 216 pixels: two row tiles, the second ragged, image boundaries at 72 and 144 inside tiles; one ragged k-tile per tap
    (2, 3, 8, 28, 86, 5, False),  # 5 x 5 at H = 3: every output row reaches over a pole, the middle one over both with unflipped kernel rows
    (2, 5, 4, 40, 86, 5, True),  # 5 x 5 at W = 4: the roll by W / 2 and the wrap can apply to the same column
    (2, 3, 2, 4, 5, 3, True),  # the narrowest width, the smallest cin and cout
    (1, 3, 4, 68, 8, 5, True),  # three k-tiles per tap, the last one holding one float4
]
TILE_CONV_STRADDLING = TILE_CONV_CASES[:2]  # a 128-row tile holds pixels of more than one image, the first of them of image 0
TILE_CONV_H2_CASE = (2, 2, 4, 8, 8, 3, False)  # H = 2: defined by sphere_gather (conv_ref(via_gather=True)), not by the oracle
MODULE_CONV_CASE = (2, 4, 8, 6, 5, 3, False)  # ladcast_amd.models.SphereConv2d(6, 5, 3, 1, 1) on (2, 6, 4, 8): cin padded to 8 with zero weights
# the smallest (frames, H, W) at cin 40, cout 136 that ldc_sphere_conv_plan hands to the halo-staged kernel (the GPU test searches and asserts it)
HALO_CASE = (16, 18, 36, 40, 136, 3, True)


@functools.lru_cache(maxsize=None)
def conv_inputs(B, H, W_, cin, cout, ks, has_res):
    s = _seed(B, H, W_, cin, cout, ks, 47)
    g = gen(s)
    x = torch.randn(B, H, W_, cin, generator=g) * 10 ** (torch.rand(B, H, W_, 1, generator=g) * 2 - 1)  # pixels of different scale: a halo pixel
    w = torch.randn(cout, cin, ks, ks, generator=g) / math.sqrt(cin * ks * ks)                             # taken from elsewhere is far off
    return dict(x=x, w=w, bias=vec(cout, s + 1)[0], R=rows_input(B, H * W_, cout, s + 2, plain=True).reshape(B, H, W_, cout) if has_res else None)
