"""Edges of the exact-fp32 128-row ring GEMM (gemm_bf16x3_v3_kernel<128, 0, false>) that the copy-free k-step (csrc/gemm_v3_kstep_f32_nocopy.inc)
must leave as they were: ragged row tiles whose idle waves run the loop body without MFMAs, partial column panels through the generic
epilogue, unit ranges across a problem boundary and inside a tile, the fast and the fused-QKV epilogues, and bit-equal repeated launches.
Through the C ABI, against float64 on the CPU with the derived bound of tests/mfma_edge_refs.py (n = K + 10 roundings; the 9 of them that stand
for the pieces of a cut tile are replaced by the launch's own worst piece count, read from `hip.gemm_plan`, where that is larger), operands and
outputs in the guard bands of tests/redzone.py.  (The cases are those written for the 32x32x2 k-step, which was measured slower and is not in
the tree - DESIGN.md 4.2; they hold for any k-step of this kernel.)
  130 x 128 x 32   the second row tile holds 2 rows: seven of its eight waves have no row (no MFMA); one k-step
  97 x 200 x 96    rows end one row into the seventh 16-row block; the second column panel holds 72 columns, through the generic epilogue;
                   three k-steps = one trip round the ring
  33 x 64 x 64     the upper half of the column panel wholly past N
  two problems of 9 and 2 k-steps in one launch: a unit range crosses the problem boundary
  a tile cut mid-k (unit ranges not aligned to tiles), launched four times with other data in the slabs in between
  the fast epilogue (whole 128-column panels): bias + GELU-tanh, bias + gate + residual
  the fused QKV epilogue against the two-step route
"""
import math

import pytest
import torch

from tests import mfma_edge_refs as R
from tests.redzone import assert_elementwise, elementwise_bound, guarded
from tests.row_edge_refs import gen
from tests.test_gpu_mfma_edges import COUNTER_BYTES, Gemm, finite, gin, gvec, same_bits, untouched

pytestmark = pytest.mark.gpu

ACT_GELU_TANH = 2


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ladcast_amd.hip as h

    return h


def unit_ranges(plan, launch=0):
    """[start, end) of every workgroup's unit range of a ring launch (ldc_gemm_plan: g units_per_group + min(g, units_rem))"""
    G, upg, rem = plan.workgroups[launch], plan.units_per_group[launch], plan.units_rem[launch]
    s = [g * upg + min(g, rem) for g in range(G + 1)]
    assert s[-1] == plan.units[launch]
    return list(zip(s[:-1], s[1:]))


def max_pieces(plan, batches):
    """the most pieces any tile of the (one-launch) group is summed from"""
    assert plan.launches == 1 and plan.kernel == 0
    ranges, worst, u = unit_ranges(plan), 1, 0
    for p, batch in enumerate(batches):
        kt = plan.k_steps[p]
        for _ in range(plan.tile_rows_m[p] * plan.tile_cols_n[p] * batch):
            worst = max(worst, sum(1 for a, b in ranges if a < u + kt and b > u))
            u += kt
    assert u == plan.units[0]
    return worst


def reference(kw, pieces):
    """float64 (value, bound): tests/mfma_edge_refs.gemm_ref with the launch's own piece count where it exceeds the 9 counted there"""
    A, W, bias = kw["A"], kw["W"], kw["bias"]
    dot = A.double() @ W.double().T
    s = A.double().abs() @ W.double().abs().T
    b = torch.zeros(W.shape[0], dtype=torch.float64) if bias is None else bias.double()
    return R.epilogue_ref(dot + b, elementwise_bound(s + b.abs(), A.shape[-1] + max(R.PIECES, pieces) + 1), kw["act"], kw["gate"], kw["R"])


class Case:
    """one exact-fp32 problem in guard bands: bias always, gate / residual (its own buffer) / activation as asked"""

    def __init__(self, hip, M, N, K, batch=1, gate=False, res=False, act=0):
        g = gen(R._seed(M, N, K, batch, int(gate), int(res), act))
        A = torch.randn(batch, M, K, generator=g) * 10 ** (torch.rand(batch, M, 1, generator=g) * 4 - 2)  # rows of very different size
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.kw = dict(A=A, W=W, bias=torch.randn(N, generator=g), gate=torch.randn(batch, N, generator=g) if gate else None,
                       R=torch.randn(batch, M, N, generator=g) if res else None, act=act)
        self.M, self.N, self.K, self.batch = M, N, K, batch
        self.A, self.W, self.bias = gin(A, pad=4, gap=8), gin(W, pad=0, gap=0), gvec(self.kw["bias"])
        self.gate = guarded(1, N, batch=batch, batch_stride=N + 4).fill(self.kw["gate"][:, None]) if gate else None
        self.Rbuf = gin(self.kw["R"], pad=12, gap=8) if res else None
        self.new_output()

    def new_output(self):
        self.C = guarded(self.M, self.N, self.N + 4, batch=self.batch, batch_stride=self.M * (self.N + 4) + 8)

    def problem(self, hip):
        Rb, gt = self.Rbuf, self.gate
        return hip.gemm_problem(self.A.view, self.W.view, self.C.view, M=self.M, N=self.N, K=self.K, batch=self.batch, lda=self.A.ld, ldw=self.K,
                                ldc=self.C.ld, a_bs=self.A.bs, c_bs=self.C.bs, bias=self.bias.view, gate=None if gt is None else gt.view,
                                gate_bs=0 if gt is None else gt.bs, R=None if Rb is None else Rb.view, ldr=0 if Rb is None else Rb.ld,
                                r_bs=0 if Rb is None else Rb.bs, act=self.kw["act"])

    def result(self, what):
        untouched(self.A, self.W, self.bias, self.gate, self.Rbuf, self.C)
        return finite(self.C.payload(), what)


def run(hip, case, what, tiles=None):
    plan = hip.gemm_plan([case.problem(hip)])
    assert (plan.kernel, plan.terms, plan.launches, plan.tile_rows[0]) == (hip.GEMM_KERNEL_RING, 0, 1, 128), what
    if tiles is not None:
        assert plan.tiles[0] == tiles, what
    hip.gemm_grouped([case.problem(hip)])
    want, bound = reference(case.kw, max_pieces(plan, [case.batch]))
    r = assert_elementwise(case.result(what), want, bound, what)
    print(f"{what}: worst err / bound {r:.3f}")
    return plan


EDGES = {
    "130 x 128 x 32: seven idle waves": (130, 128, 32, 2),
    "97 x 200 x 96: ragged rows and a 72-column panel": (97, 200, 96, 2),
    "33 x 64 x 64: half a column panel": (33, 64, 64, 1),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edges_of_the_tile(hip, name):
    M, N, K, tiles = EDGES[name]
    run(hip, Case(hip, M, N, K), name, tiles)


def test_range_across_the_problem_boundary(hip):
    """tests/mfma_edge_refs.py, "two problems, 9 and 2 k-steps": one launch of 13 unit ranges, one of which holds the last units of the
    first problem and the first of the second"""
    name = "two problems, 9 and 2 k-steps"
    gemms = [Gemm(hip, "f32 ring", M, N, R.sweep_K("f32", k32), batch, i) for i, (M, N, k32, batch) in enumerate(R.SWEEP_PROBLEMS[name])]
    probs = [g.problem(hip) for g in gemms]
    plan = hip.gemm_plan(probs)
    assert plan.kernel == hip.GEMM_KERNEL_RING and list(plan.workgroups[: plan.launches]) == R.SWEEP_CUTS[name]["f32"]
    first = plan.tile_rows_m[0] * plan.tile_cols_n[0] * gemms[0].batch * plan.k_steps[0]  # units of the first problem
    assert any(a < first < b for a, b in unit_ranges(plan)), "no range crosses the problem boundary"
    assert max_pieces(plan, [g.batch for g in gemms]) <= R.PIECES
    hip.gemm_grouped(probs)
    for i, g in enumerate(gemms):
        want, bound = R.gemm_case_ref(g.M, g.N, g.K, g.batch, i, "f32")
        r = assert_elementwise(g.result(f"{name}, problem {i}"), want, bound, f"{name}, problem {i}")
        print(f"{name}, problem {i}: worst err / bound {r:.3f}")


MID_K = (384, 256, 9600)  # 6 tiles of 300 k-steps: 1800 units over 256 workgroups = 7 each and 8 left over


def test_tile_cut_mid_k_is_reproducible(hip):
    """6 tiles x 300 k-steps over a grid that does not divide them (units_rem != 0, asserted): ranges of 7 and 8 k-steps that start anywhere in
    a tile, more than 40 pieces per tile (the bound counts them).  Four launches, the slabs overwritten with other data in between: the same bits, every tile counter back at zero."""
    M, N, K = MID_K
    case = Case(hip, M, N, K)
    plan = hip.gemm_plan([case.problem(hip)])
    assert plan.tiles[0] <= 12 and plan.k_steps[0] >= 256 and plan.units_rem[0] != 0, (plan.tiles[0], plan.k_steps[0], plan.workgroups[0], plan.units_rem[0])
    pieces = max_pieces(plan, [1])
    assert pieces > 1
    want, bound = reference(case.kw, pieces)
    ws = hip._grouped_workspace(case.C.view.device)
    outs = []
    for rep in range(4):
        case.new_output()
        hip.gemm_grouped([case.problem(hip)])
        outs.append(case.result(f"mid-k cut, launch {rep}"))
        assert int(ws.view(-1).view(torch.int32)[: COUNTER_BYTES // 4].abs().max()) == 0, "tile counters not re-armed"
        ws.view(-1)[COUNTER_BYTES // 4:].normal_(0.0, 1e6)  # other data in the slabs
    r = assert_elementwise(outs[0], want, bound, "mid-k cut")
    print(f"mid-k cut ({plan.workgroups[0]} workgroups, at most {pieces} pieces per tile): worst err / bound {r:.3f}")
    for rep in range(1, 4):
        same_bits(outs[rep], outs[0], f"mid-k cut, launch {rep}")


@pytest.mark.parametrize("epi", ["bias + GELU-tanh", "bias + gate + residual"])
def test_fast_epilogue(hip, epi):
    """whole 128-column panels, 16-byte aligned rows: the epilogue whose loads are issued ahead (gemm_v3_common.inc: tile_epilogue_fast)"""
    kw = dict(act=ACT_GELU_TANH) if epi == "bias + GELU-tanh" else dict(gate=True, res=True)
    run(hip, Case(hip, 130, 256, 64, batch=2, **kw), f"fast epilogue, {epi}", tiles=8)


def _rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("Nx,Nc,H,batch", [(37, 11, 1, 2), (70, 0, 2, 1)])
def test_qkv_epilogue(hip, Nx, Nc, H, batch):
    """ldc_gemm_grouped_qkv_f32 against the two-step route (ldc_gemm_grouped, then ldc_qk_rmsnorm_rope in place), a rotary table on the first
    stream: q and k within the 3e-7 of tests/test_gpu_ops.py::test_gemm_qkv_epilogue_exact_fp32, v and the ordinary problem of the same launch
    bit for bit, and a second launch bit for bit"""
    from oracle import layers as L

    D, K, S = H * 128, 256, Nx + Nc
    d = lambda t: t.to("cuda")  # noqa: E731
    A = d(_rnd(batch, S, K, seed=1))
    Wx, Wc = d(_rnd(3 * D, K, seed=2) / math.sqrt(K)), d(_rnd(3 * D, K, seed=3) / math.sqrt(K))
    bx, bc = d(_rnd(3 * D, seed=4) * 0.1), d(_rnd(3 * D, seed=5) * 0.1)
    Wm, bm = d(_rnd(512, K, seed=6) / math.sqrt(K)), d(_rnd(512, seed=7))
    wq0, wk0, wq1, wk1 = [d(1 + 0.1 * _rnd(128, seed=s_)) for s_ in (12, 13, 14, 15)]
    cos0, sin0 = [d(t) for t in L.get_1d_rotary_pos_embed(128, torch.arange(Nx).float() * 0.37, 256.0)]

    def problems(qkv_, mlp_):
        pr = [hip.gemm_problem(A, Wx, qkv_, M=Nx, N=3 * D, K=K, batch=batch, a_bs=S * K, c_bs=S * 3 * D, bias=bx)]
        if Nc:
            pr.append(hip.gemm_problem(A[:, Nx:], Wc, qkv_[:, Nx:], M=Nc, N=3 * D, K=K, batch=batch, a_bs=S * K, c_bs=S * 3 * D, bias=bc))
        pr.append(hip.gemm_problem(A, Wm, mlp_, M=S, N=512, K=K, batch=batch, a_bs=S * K, c_bs=S * 512, bias=bm, act=ACT_GELU_TANH))
        return pr

    epis = [hip.qkv_epilogue(wq0, wk0, hip.compact_rope_table(cos0, sin0), eps=1e-7, heads=H, qscale=1.0)]
    if Nc:
        epis.append(hip.qkv_epilogue(wq1, wk1, None, eps=1e-7, heads=H, qscale=1.0))
    epis.append(None)
    outs = []
    for rep in range(2):
        qkv = torch.full((batch, S, 3 * D), float("nan"), device="cuda")
        mlp = torch.full((batch, S, 512), float("nan"), device="cuda")
        assert hip.gemm_grouped_qkv_f32(problems(qkv, mlp), epis)
        outs.append((qkv, mlp))
    (qkv, mlp), (qkv_b, mlp_b) = outs
    qkv2 = torch.full((batch, S, 3 * D), float("nan"), device="cuda")
    mlp2 = torch.full((batch, S, 512), float("nan"), device="cuda")
    hip.gemm_grouped(problems(qkv2, mlp2))
    hip.qk_rmsnorm_rope(qkv2[:, :, :D], qkv2[:, :, D: 2 * D], B=batch, row0=0, rows=Nx, H=H, ld=3 * D, bs=S * 3 * D, wq=wq0, wk=wk0, eps=1e-7, cos=cos0, sin=sin0)
    if Nc:
        hip.qk_rmsnorm_rope(qkv2[:, :, :D], qkv2[:, :, D: 2 * D], B=batch, row0=Nx, rows=Nc, H=H, ld=3 * D, bs=S * 3 * D, wq=wq1, wk=wk1, eps=1e-7)
    torch.cuda.synchronize()
    assert torch.isfinite(qkv).all() and torch.isfinite(mlp).all()
    for name, lo in (("q", 0), ("k", D)):
        got, want = qkv[..., lo: lo + D].double().cpu(), qkv2[..., lo: lo + D].double().cpu()
        err = ((got - want).norm() / want.norm()).item()
        print(f"qkv epilogue ({Nx}, {Nc}, {H}, {batch}) {name}: rel-L2 against the two-step route {err:.3e}")
        assert err < 3e-7, (name, err)
    same_bits(qkv[..., 2 * D:], qkv2[..., 2 * D:], "v: bias only")
    same_bits(mlp, mlp2, "the ordinary problem of the same launch")
    same_bits(qkv_b, qkv, "second launch, qkv")
    same_bits(mlp_b, mlp, "second launch, ordinary problem")
