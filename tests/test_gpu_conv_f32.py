"""The exact-fp32 SphereConv2d: `ldc_sphere_conv_nhwc_split(in_fmt = LDC_FMT_F32)`, the conv-gather instance of the ring kernel
(`gemm_bf16x3_v3_kernel<128, 0, true>`: v_mfma_f32_16x16x4_f32 on plain fp32 pixel rows), which runs every dense conv, pointwise conv
and Linear of the DC-AE in the fp32 mode (models/DCAE.py `_conv` / `_mm`) - op by op against the oracle conv (oracle/sphere_conv.py,
pinned to fixtures of the reference class) run in float64.

Every case holds both pole rows (kernel-row flip) and the longitude wrap.  Per case:
* rel-L2 at fp32 grade: below FP32_GRADE x the rel-L2 of a CPU fp32 conv of the same operands (computed here);
* element-wise: |y - y64| / (|x| (*) |w| + |b| + |R|), the denominator being the same oracle conv on absolute values, stays within
  ELEM_GRADE x what the CPU fp32 conv reaches - one bad tile, row or tap that a tensor-wide norm averages away shows here;
* negative control: the split-bf16 conv (LDC_FMT_SPLIT) of the same data is ABOVE the fp32 ceiling, so the check can tell the two apart;
* repeated launches (another launch in between) are bitwise equal and leave the stream-K arrival counters at zero.
Operand rows carry NaN between cin and the row stride (never read: the channel tail of the last k-step of a tap comes from the zero
page) and finite garbage between the weight's channel count and cin (read, multiplied by the zero weight columns)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import ladcast_amd.hip as hip  # noqa: E402
from ladcast_amd.models.sphere_conv import ceil4, pack_dense_weight_bf16x3, pack_dense_weight_f32ring  # noqa: E402
from oracle.sphere_conv import SphereConv2d as OracleConv  # noqa: E402
from tests.synth import rel_l2  # noqa: E402

# The kernel sums each output's K = k*k*cin_pp products in ONE fp32 accumulator chain of K / 4 MFMA steps (unless stream-K cuts the tile),
# so its rounding error grows ~ sqrt(K / 4) x 2^-24, while the CPU conv blocks its sums: measured on an MI355X (this tree) the kernel's
# rel-L2 is 0.7x - 4.5x the CPU fp32 conv's and its element-wise figure 0.5x - 10x (both largest at 504 -> 1008, K = 4608), all of it
# 4x - 30x below the split-bf16 conv of the same data.
FP32_GRADE = 6.0  # rel-L2 ceiling: this many times the CPU fp32 conv's own rel-L2 against float64
ELEM_GRADE = 16.0  # element-wise ceiling: this many times the CPU fp32 conv's largest |err| / (|x| (*) |w| + |b| + |R|)
BM, BN = 128, 128  # the ring kernel's exact-fp32 tile (gemm_bf16x3_v3.hip: gemm_bf16x3_v3_kernel<128, 0, true>)

# (id, B, H, W, ci (the weight's input channels), cout, ksize, act, bias, resid, ldx (None: ceil4(ci)), ldy (None: cout))
CASES = [
    ("conv_in_89", 1, 120, 240, 89, 252, 3, hip.ACT_NONE, True, False, None, None),  # cin_p 92: a channel tail, 3 -> 4 k-steps per tap
    ("res_252", 1, 120, 240, 252, 252, 3, hip.ACT_SILU, True, False, None, None),
    ("down_504_1008", 1, 60, 120, 504, 1008, 3, hip.ACT_NONE, True, False, None, None),
    ("res_504_30x60", 2, 30, 60, 504, 504, 3, hip.ACT_NONE, True, True, None, None),  # residual; 3600 rows: ragged last row tile
    ("conv_out_15x30", 1, 15, 30, 1008, 84, 3, hip.ACT_NONE, True, False, None, None),  # 450 rows, one ragged column panel
    ("conv_in_15x30", 3, 15, 30, 84, 1008, 3, hip.ACT_RELU, True, True, None, None),
    ("k1_K36", 2, 15, 30, 36, 200, 1, hip.ACT_NONE, True, False, None, None),  # K % 32 != 0
    ("k1_K100_silu", 1, 30, 60, 100, 136, 1, hip.ACT_SILU, True, False, None, None),
    ("k1_K1008_qkv", 1, 15, 30, 1008, 3024, 1, hip.ACT_NONE, False, False, None, None),
    ("k1_K2016", 2, 30, 60, 2016, 504, 1, hip.ACT_NONE, True, False, None, None),  # 63 -> 64 k-steps
    ("k5_dense", 2, 10, 24, 36, 40, 5, hip.ACT_SILU, True, True, None, None),
    ("superrow_wide_ldx", 1, 30, 120, 32, 256, 3, hip.ACT_NONE, True, False, 4096, None),  # M * ldx * 4 >= 48e6: super-row tile order
    ("ldy_gt_cout", 2, 16, 32, 40, 136, 3, hip.ACT_RELU, True, True, 48, 144),
    ("cout_mod4_scalar_epi", 2, 16, 32, 40, 86, 3, hip.ACT_SILU, True, True, None, None),  # N % 4 != 0: the scalar epilogue
]


def _tile_order(M, N, ldx):
    """(row tiles, super-row height rm) of the conv launch, as the planner chooses them (csrc/gemm_plan.hip)"""
    tm, tn = -(-M // BM), -(-N // BN)
    rm = tm
    if M * ldx * 4.0 >= 48e6:
        want = math.sqrt(tm * tn / 8.0 * BN / BM)
        nsr = min(max(int(tm / max(want, 1.0) + 0.5), 1), tm)
        rm = -(-tm // nsr)
    return tm, rm


def _conv_ref(x, w, b, k, act, R, dtype):
    """act(SphereConv2d(x) + b) + R in `dtype` on the CPU (oracle conv; k = 1: the plain pointwise product); NCHW"""
    x, w = x.to(dtype), w.to(dtype)
    if k == 1:
        y = torch.einsum("oc,bchw->bohw", w[:, :, 0, 0], x)
    else:
        o = OracleConv(w.shape[1], w.shape[0], k, 1, k // 2, bias=False).to(dtype)
        with torch.no_grad():
            o.weight.copy_(w)
            y = o(x)
    if b is not None:
        y = y + b.to(dtype)[None, :, None, None]
    y = {hip.ACT_NONE: lambda v: v, hip.ACT_SILU: F.silu, hip.ACT_RELU: F.relu}[act](y)
    return y + R.to(dtype) if R is not None else y


def _rows(t):  # NCHW -> [B*H*W, C]
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _data(B, H, W, ci, co, k, bias, resid, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ci, H, W, generator=g)
    w = torch.randn(co, ci, k, k, generator=g) / (ci * k * k) ** 0.5
    b = torch.randn(co, generator=g) if bias else None
    R = torch.randn(B, co, H, W, generator=g) if resid else None
    return x, w, b, R


def _operand_rows(x, cin, ldx, seed):
    """fp32 pixel rows [M, ldx]: the channels, finite garbage up to cin (zero weight columns), NaN behind cin (never read)"""
    M, ci = x.shape[0] * x.shape[2] * x.shape[3], x.shape[1]
    X = torch.full((M, ldx), float("nan"))
    X[:, :ci] = _rows(x)
    if cin > ci:
        X[:, ci:cin] = 1e3 * torch.randn(M, cin - ci, generator=torch.Generator().manual_seed(seed))
    return X


def _conv_f32(X, wp, b, R, *, B, H, W, cin, cout, ldx, ldy, k, act):
    Y = torch.full((X.shape[0], ldy), -7.0, device="cuda")
    hip.sphere_conv_nhwc_split(X, wp, Y, B=B, H=H, W=W, cin=cin, ldx=ldx, cout=cout, ldy=ldy, bias=b, R=R, ldr=cout if R is not None else 0,
                               ksize=k, act=act, in_fmt=hip.FMT_F32, out_fmt=hip.FMT_F32)
    return Y


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exact_fp32_conv_is_fp32_grade(case):
    name, B, H, W, ci, co, k, act, bias, resid, ldx, ldy = case
    cin = ceil4(ci)
    ldx, ldy = ldx or cin, ldy or co
    M = B * H * W
    x, w, b, R = _data(B, H, W, ci, co, k, bias, resid, seed=len(name))
    if name.startswith("superrow"):
        tm, rm = _tile_order(M, co, ldx)
        assert rm < tm and tm % rm != 0, (tm, rm)  # several super-rows, the last one short
    # references: float64 (truth), the same on absolute values (the scale of each output's rounding), CPU fp32 (the grade)
    y64 = _conv_ref(x, w, b, k, act, R, torch.float64)
    den = _conv_ref(x.abs(), w.abs(), b.abs() if b is not None else None, k, hip.ACT_NONE, R.abs() if R is not None else None, torch.float64)
    y32 = _conv_ref(x, w, b, k, act, R, torch.float32)
    y64, den, y32 = _rows(y64), _rows(den), _rows(y32)
    e_cpu, q_cpu = rel_l2(y32, y64), ((y32.double() - y64).abs() / den).max().item()

    X = _operand_rows(x, cin, ldx, seed=len(name) + 1).cuda()
    wp = pack_dense_weight_f32ring(w.cuda())
    bd = b.cuda() if b is not None else None
    Rd = _rows(R).contiguous().cuda() if R is not None else None
    kw = dict(B=B, H=H, W=W, cin=cin, cout=co, ldx=ldx, ldy=ldy, k=k, act=act)
    Y = _conv_f32(X, wp, bd, Rd, **kw)
    torch.cuda.synchronize()
    Yc = Y.cpu()
    got = Yc[:, :co]
    assert torch.isfinite(got).all(), name
    if ldy > co:
        assert (Yc[:, co:] == -7.0).all(), "columns behind cout were written"
    err = rel_l2(got, y64)
    q = ((got.double() - y64).abs() / den).max().item()
    g5 = got.reshape(B, H, W, co)
    w5, ceiling = y64.reshape(B, H, W, co), FP32_GRADE * e_cpu
    e_edges = [rel_l2(g5[:, 0], w5[:, 0]), rel_l2(g5[:, -1], w5[:, -1]), rel_l2(g5[:, :, 0], w5[:, :, 0]), rel_l2(g5[:, :, -1], w5[:, :, -1])]

    # negative control: the split-bf16 conv of the same operands
    c8 = -(-cin // 8) * 8
    xs = torch.empty(M, c8, device="cuda")
    hip.split_rows(X[:, :cin].contiguous(), xs, rows=M, C=cin)
    Ys = torch.empty(M, co, device="cuda")
    hip.sphere_conv_nhwc_split(xs, pack_dense_weight_bf16x3(w.cuda()), Ys, B=B, H=H, W=W, cin=cin, ldx=c8, cout=co, bias=bd, R=Rd,
                               ldr=co if R is not None else 0, ksize=k, act=act)
    e_split = rel_l2(Ys.cpu(), y64)
    print(f"\nfp32 conv {name}: rel-L2 {err:.2e} (CPU fp32 {e_cpu:.2e}, split-bf16 {e_split:.2e}; pole rows / wrap columns max "
          f"{max(e_edges):.2e}), max |err| / (|x| (*) |w|) {q:.2e} (CPU fp32 {q_cpu:.2e})")
    assert err < ceiling, (name, err, e_cpu)
    assert max(e_edges) < ceiling, (name, e_edges, e_cpu)
    assert q < ELEM_GRADE * q_cpu, (name, q, q_cpu)
    assert e_split > ceiling, (name, e_split, ceiling)  # the check tells split-bf16 arithmetic from fp32

    # bitwise reproducible, counters re-armed (another launch with other data in between)
    _conv_f32(X * 2.0, wp, bd, Rd, **kw)
    Y2 = _conv_f32(X, wp, bd, Rd, **kw)
    assert torch.equal(Y2, Y), name
    ws = hip._grouped_workspace(X.device)
    assert int(ws.view(torch.int32)[: (1 << 20) // 4].abs().sum().item()) == 0


def test_exact_fp32_conv_rejects_what_it_cannot_gather():
    """the fp32 operand rows are read in 16-byte chunks of 4 channels: cin and ldx must be multiples of 4 (LDC_ERR_ALIGN, nothing written)"""
    X = torch.zeros(2 * 8 * 16, 40, device="cuda")
    wp = torch.zeros(8, 9 * 64, device="cuda")
    Y = torch.full((2 * 8 * 16, 8), 3.0, device="cuda")
    for cin, ldx in ((38, 40), (36, 38)):
        with pytest.raises(RuntimeError, match="status -2"):
            hip.sphere_conv_nhwc_split(X, wp, Y, B=2, H=8, W=16, cin=cin, ldx=ldx, cout=8, ksize=3, in_fmt=hip.FMT_F32)
    torch.cuda.synchronize()
    assert (Y == 3.0).all()
