"""Guard-band and per-element edge tests of the matrix-core kernels: the ring GEMM in its three arithmetics, the register-staged stream-K
GEMM, both attentions and the sphere convs, all through the C ABI.

Every operand and output is a `redzone.guarded` buffer: inputs with poisoned pad columns (lda > K, ld_qkv > 3 D, ldx > cin, ldr > N) and
poisoned batch gaps, outputs UNWRITTEN, `assert_untouched` on every one after the launch - workspaces included.  A read past an extent pulls
a NaN into the output, where the finite-ness check finds it; every element is then held to the DERIVED bound of tests/mfma_edge_refs.py
against float64 (tests/test_mfma_edge_bounds_cpu.py judges those bounds).  The cut sweep calls the grouped entry points with a workspace
that only fits g unit ranges, which the planner (csrc/gemm_plan.hip) documents it shrinks the grid to: every cut from one range up
to the planner's own choice, without an environment variable; what that choice is, per problem set and path, is asserted through `hip.gemm_plan`.  The attentions run their small one-unit-per-workgroup grids over the
S / Sq / bias table and, at one 260-unit shape, the other schedules: the exact-fp32 kernel's 4-wave form and balanced cut, the split
kernel's persistent form with its key-sliced tail and merge launch - each shown to have run by what it leaves in its workspace.

The tile-per-workgroup kernel of gemm_f32.hip runs behind its own two entry points, `ldc_gemm_bias_act` (175 shapes over the ragged
depths 4 / 36 / 84 and the LDS-stage depths 64 / 96, W strided too) and `ldc_sphere_conv_nhwc` (six cases at act 0 and 1: tiles that
straddle images, ragged channel tiles, 5 x 5 kernels at H = 3 and W = 4, the narrowest width; H = 2 against the float64 gather-GEMM; one
case through `ladcast_amd.models.SphereConv2d` with cin padded by zero weights), under the same method plus the same bits on a second
launch; every argument the two entry points refuse is passed once, with the status asserted and the outputs still unwritten.

Not covered here: the pixel-count refusal of `ldc_sphere_conv_nhwc` (see test_tile_conv_refusals); three pieces of one tile in the
single-term mode (K <= 768 gives it 12 k-steps, which no rule cuts: its pieces come from the sweeps of the other problem sets).

LDC_MFMA_EDGE_RATIOS=<file>: the worst err / bound ratio of every case is written there as JSON (profiles/mfma_edge_worst_ratios.json)."""
import json
import os
from ctypes import byref, c_void_p

import pytest
import torch

from tests import mfma_edge_refs as R
from tests import redzone as rz
from tests.redzone import FMT_BF16, FMT_F32, FMT_SPLIT, assert_elementwise, assert_untouched, guarded, operand_rows, operand_width

pytestmark = pytest.mark.gpu

ERR_ARG = -1
COUNTER_BYTES = 1 << 20  # LDC_GEMM_COUNTER_BYTES
SLOT_BYTES = 128 * 128 * 4  # one partial-tile slab of the 128-row kernels
RATIOS = []


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ladcast_amd.hip as h

    yield h
    out = os.environ.get("LDC_MFMA_EDGE_RATIOS")
    if out:
        with open(out, "w") as f:
            json.dump(RATIOS, f, indent=0)


def note(op, mode, shape, ratio):
    RATIOS.append(dict(op=op, mode=mode, shape=str(shape), ratio=round(ratio, 4)))


def gin(t, pad=4, gap=8, align=16):
    """poisoned guarded input holding fp32 t [B][rows][width]: row stride width + pad, batch stride rows * ld + gap"""
    t = t if t.dim() == 3 else t[None]
    B, rows, w = t.shape
    return guarded(rows, w, w + pad, align_bytes=align, batch=B, batch_stride=rows * (w + pad) + gap).fill(t)


def gbits(img, ld, gap, align=32):
    """poisoned guarded fp32-typed buffer holding the int32 bit image img [B][rows][width] (operand rows)"""
    B, rows, w = img.shape
    g = guarded(rows, w, ld, align_bytes=align, batch=B, batch_stride=rows * ld + gap)
    g.view.view(torch.int32).copy_(img)
    return g


def gvec(v):
    return gin(v.reshape(1, 1, -1), pad=0, gap=0)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(got, want, what):
    got, want = bits(got), bits(want)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} words differ, first at {tuple(bad[0].tolist())}")


def finite(p, what):
    bad = ~torch.isfinite(p)
    assert not bad.any(), f"{what}: {int(bad.sum())} non-finite values (a poisoned read or a missing write), first at {tuple(bad.nonzero()[0].tolist())}"
    return p


def still_unwritten(p, what):
    assert bool((bits(p) == rz._signed(rz.UNWRITTEN32, 32)).all()), f"{what}: written"


def untouched(*bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        if b is not None:
            assert_untouched(b, f"buffer {i}")


def ok(status, what):
    assert status == 0, f"{what} failed with status {status}"


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------
# path -> (arithmetic, A format, flags, split_bf16 entry point, strided W)
PATHS = {
    "f32 ring": ("f32", FMT_F32, 0, False, False),
    "f32 register-staged": ("f32", FMT_F32, 8, False, True),  # GEMM_F32_REGSTAGE
    "bf16x3, fp32 A": ("bf16x3", FMT_F32, 0, True, True),  # the register-staged kernel splits A in its loop
    "bf16x3, split A": ("bf16x3", FMT_SPLIT, 1, True, True),
    "bf16x3, split A and C": ("bf16x3", FMT_SPLIT, 1 | 2, True, True),
    "bf16 single term": ("bf16", FMT_BF16, 1 | 4, True, True),
    "bf16 single term, bf16 C": ("bf16", FMT_BF16, 1 | 2 | 4, True, True),
}
REGSTAGE_PATHS = ("f32 register-staged", "bf16x3, fp32 A")  # what `hip.gemm_plan` must say of every launch on these paths, and of no other
TILE_PATH = "f32 tile-per-workgroup"  # ldc_gemm_bias_act: its own entry point, not a path of the grouped ones
TILE_PATHS = {TILE_PATH: ("f32", FMT_F32, 0, False, True)}


class Gemm:
    """the guarded operands of one GEMM problem on one path, and its launch struct"""

    def __init__(self, hip, path, M, N, K, batch, epi, c_fmt=None, rows_layout=False, inputs=R.gemm_inputs):
        mode, a_fmt, flags, self.split_entry, strided_w = PATHS[path] if path in PATHS else TILE_PATHS[path]
        has_bias, has_gate, res, act, col0 = R.EPILOGUES[epi]
        kw = inputs(M, N, K, batch, epi, mode)
        self.c_fmt = c_fmt = (0 if not flags & 2 else FMT_SPLIT if mode == "bf16x3" else FMT_BF16) if c_fmt is None else c_fmt
        if c_fmt or rows_layout:  # operand rows out (or their fp32 twin): no column offset; the residual from its own buffer (C is not fp32 rows)
            col0, res = 0, "separate" if res else None
        if not c_fmt:
            flags &= ~2
        self.M, self.N, self.col0, self.batch, self.kw = M, N, col0, batch, kw
        if a_fmt == FMT_F32:
            self.A = gin(kw["A"], pad=8 if mode == "bf16x3" else 4, gap=8)
        else:
            self.A = gbits(operand_rows(kw["A"], a_fmt), ld=K + 8, gap=16)
        Wd = gin(kw["W"], pad=4 if strided_w else 0, gap=0)  # [1][N][K], ldw = K + 4 | K
        if mode == "f32":
            self.W, ldw = Wd, Wd.ld
        else:  # packed by the library into a guarded buffer of its own
            self.Wsrc, ldw = Wd, K
            self.W = guarded(1, N * K if mode == "bf16x3" else N * K // 2, align_bytes=16)
            pack = hip.lib.ldc_pack_weight_bf16x2 if mode == "bf16x3" else hip.lib.ldc_pack_weight_bf16
            ok(pack(c_void_p(Wd.view.data_ptr()), c_void_p(self.W.view.data_ptr()), N, K, Wd.ld, hip._stream()), "pack weight")
        self.bias = gvec(kw["bias"]) if has_bias else None
        self.gate = guarded(1, N, batch=batch, batch_stride=N + 4).fill(kw["gate"][:, None]) if has_gate else None
        self.Rbuf = gin(kw["R"], pad=12, gap=8) if res == "separate" else None
        self.res, self.act, self.flags, self.ldw, self.K = res, act, flags, ldw, K
        self.new_output()

    def new_output(self):
        M, N, col0, batch = self.M, self.N, self.col0, self.batch
        if self.c_fmt:
            w = operand_width(N, self.c_fmt)
            ld = (N + 7) // 8 * 8 + 8
            self.C = guarded(M, w, ld, align_bytes=32, batch=batch, batch_stride=M * ld + 16)
        else:
            self.C = guarded(M, col0 + N, col0 + N + 4, batch=batch, batch_stride=M * (col0 + N + 4) + 8)
            if self.res == "inplace":
                self.C.view[:, :, col0:].copy_(self.kw["R"])
        return self.C

    def problem(self, hip):
        C, Rb = self.C, self.Rbuf
        cv = C.view[:, :, self.col0:]
        Rt, ldr, r_bs = (cv, C.ld, C.bs) if self.res == "inplace" else (Rb.view, Rb.ld, Rb.bs) if Rb is not None else (None, 0, 0)
        return hip.gemm_problem(self.A.view, self.W.view, cv, M=self.M, N=self.N, K=self.K, batch=self.batch, lda=self.A.ld, ldw=self.ldw, ldc=C.ld,
                                a_bs=self.A.bs, c_bs=C.bs, bias=None if self.bias is None else self.bias.view, gate=None if self.gate is None else self.gate.view,
                                gate_bs=0 if self.gate is None else self.gate.bs, R=Rt, ldr=ldr, r_bs=r_bs, act=self.act, flags=self.flags)

    def buffers(self):
        return [self.A, self.W, getattr(self, "Wsrc", None), self.bias, self.gate, self.Rbuf, self.C]

    def result(self, what):
        """fp32 payload [B][M][N] after the guards and (fp32 rows) the finite-ness were checked"""
        untouched(*self.buffers())
        p = self.C.payload()
        if self.c_fmt:
            return p
        if self.col0:
            still_unwritten(p[..., : self.col0], f"{what}: columns before the column offset")
        return finite(p[..., self.col0:], what)


def _run_gemm_case(hip, path, M, N, K, batch, epi, cached=True, tile=None):
    """tile: the (tile rows, tiles) the planner must give the very problem that is launched"""
    mode = PATHS[path][0]
    what = f"gemm[{path}] {M} x {N} x {K}, batch {batch}, epilogue {epi}"
    inputs = R.gemm_inputs if cached else R.gemm_inputs.__wrapped__
    g = Gemm(hip, path, M, N, K, batch, epi, inputs=inputs)
    plan = hip.gemm_plan([g.problem(hip)], split_bf16=g.split_entry)
    assert (plan.kernel == hip.GEMM_KERNEL_REGSTAGE) == (path in REGSTAGE_PATHS) and plan.launches == 1, what
    if tile is not None:
        assert (plan.tile_rows[0], plan.tiles[0]) == tile, what
    hip.gemm_grouped([g.problem(hip)], split_bf16=g.split_entry)
    got = g.result(what)
    if g.c_fmt:  # operand rows out = the split of the fp32 rows the same launch shape writes, bit for bit
        f = Gemm(hip, path, M, N, K, batch, epi, c_fmt=0, rows_layout=True)
        hip.gemm_grouped([f.problem(hip)], split_bf16=True)
        c32 = f.result(what + " (fp32 rows)")
        same_bits(got, operand_rows(c32, g.c_fmt), what)
        got = c32
    want, bound = R.gemm_case_ref(M, N, K, batch, epi, mode) if cached else R.gemm_ref(mode=mode, **g.kw)
    r = assert_elementwise(got, want, bound, what)
    note("gemm", path, (M, N, K, batch, epi), r)
    return r


@pytest.mark.parametrize("path", list(PATHS))
def test_gemm_edges(hip, path):
    mode, csplit = PATHS[path][0], bool(PATHS[path][2] & 2)
    worst = 0.0
    for M, N, K, batch, epi in R.gemm_shapes(mode, regstage=path == "f32 register-staged"):
        if csplit and N % 4:  # operand rows out need N % 4 == 0 (LDC_ERR_ALIGN): the scalar epilogue has no such path
            continue
        worst = max(worst, _run_gemm_case(hip, path, M, N, K, batch, epi))
    print(f"gemm[{path}]: worst err / bound {worst:.3f}")


def test_gemm_256_row_tile(hip):
    """the planner takes the 256-row tile (two 16-row tiles per wave) - asserted on its plan of this launch: 20 x 21 = 420 of them;
    5000 = 19 x 256 + 136 rows, 2570 = 20 x 128 + 10 columns"""
    M, N, K = 5000, 2570, 64
    r = _run_gemm_case(hip, "bf16x3, split A", M, N, K, 1, 0, cached=False, tile=(256, 420))  # (its 200 MB of float64 reference are not kept)
    print(f"256-row tile: worst err / bound {r:.3f}")


def test_gemm_group_launched_problem_by_problem(hip):
    """240 + 64 = 304 tiles of 8 k-steps: no k-aligned cut reaches 160 workgroups (every aligned grid is a multiple of 19), so the split
    mode's planner gives each problem a launch of its own - 240 whole tiles, then 64"""
    path, mode = "bf16x3, split A", "bf16x3"
    gemms = [Gemm(hip, path, M, 2048, 256, 1, i, inputs=R.gemm_inputs.__wrapped__) for i, M in enumerate((1920, 512))]
    probs = [g.problem(hip) for g in gemms]
    plan = hip.gemm_plan(probs, split_bf16=True)
    assert plan.launches == 2
    assert (plan.kernel, list(plan.tile_rows[:2]), list(plan.workgroups[:2]), list(plan.tiles[:2])) == (hip.GEMM_KERNEL_RING, [128, 128], [240, 64], [240, 64])
    hip.gemm_grouped(probs, split_bf16=True)
    for i, g in enumerate(gemms):
        what = f"split group, problem {i}"
        want, bound = R.gemm_ref(mode=mode, **g.kw)
        note("gemm", path, ("split group", i), assert_elementwise(g.result(what), want, bound, what))


# ---- the stream-K cut sweep -------------------------------------------------------------------------------------------------------
def _workspace(hip, g):
    nbytes = COUNTER_BYTES + 2 * g * SLOT_BYTES
    ws = guarded(1, nbytes // 4, align_bytes=16)  # slabs start UNWRITTEN: a piece summed from a slab nobody wrote is a NaN in C
    ok(hip.lib.ldc_gemm_grouped_workspace_init(c_void_p(ws.view.data_ptr()), nbytes, hip._stream()), "workspace init")
    return ws, nbytes


def _launch(hip, gemms, ws, nbytes, split_entry):
    probs = [g.problem(hip) for g in gemms]
    arr = (hip.GemmProblem * len(probs))(*[p[0] for p in probs])
    fn = hip.lib.ldc_gemm_grouped_bf16x3 if split_entry else hip.lib.ldc_gemm_grouped
    return fn(arr, len(probs), c_void_p(ws.view.data_ptr()), nbytes, hip._stream())


SWEEP_PATHS = ("f32 ring", "f32 register-staged", "bf16x3, fp32 A", "bf16x3, split A", "bf16 single term")


@pytest.mark.parametrize("name", list(R.SWEEP_PROBLEMS))
@pytest.mark.parametrize("path", SWEEP_PATHS)
def test_streamk_cut_sweep(hip, path, name):
    """what each problem set makes each dispatcher do is written beside R.SWEEP_PROBLEMS (the split ring modes launch a group of unequal
    depths one by one: their grouped launches are the two equal-depth sets).  The exact-fp32 ring kernel asks for 256 KiB of slabs, i.e.
    g >= 2: at g = 1 ldc_gemm_grouped runs the register-staged kernel."""
    mode = PATHS[path][0]
    gemms = [Gemm(hip, path, M, N, R.sweep_K(mode, k32), batch, i) for i, (M, N, k32, batch) in enumerate(R.SWEEP_PROBLEMS[name])]
    refs = [R.gemm_case_ref(g.M, g.N, g.K, g.batch, i, mode) for i, g in enumerate(gemms)]
    split_entry = gemms[0].split_entry
    plan = hip.gemm_plan([g.problem(hip) for g in gemms], split_bf16=split_entry)
    if path in REGSTAGE_PATHS:
        assert (plan.kernel, plan.launches) == (hip.GEMM_KERNEL_REGSTAGE, 1)
    else:  # ring kernel: (launches, workgroups of each) as written beside R.SWEEP_PROBLEMS
        assert plan.kernel == hip.GEMM_KERNEL_RING and list(plan.workgroups[: plan.launches]) == R.SWEEP_CUTS[name][mode], (path, name)
    for g_ranges in R.SWEEP_G:
        ws, nbytes = _workspace(hip, g_ranges)
        outs = []
        for rep in range(2):
            for g in gemms:
                g.new_output()
            ok(_launch(hip, gemms, ws, nbytes, split_entry), f"{path}, {name}, g = {g_ranges}")
            outs.append([g.result(f"{path}, {name}, g = {g_ranges}, problem {i}") for i, g in enumerate(gemms)])
        for i, (got, (want, bound)) in enumerate(zip(outs[0], refs)):
            r = assert_elementwise(got, want, bound, f"{path}, {name}, g = {g_ranges}, problem {i}")
            note("gemm cut sweep", path, (name, i, g_ranges), r)
            same_bits(outs[1][i], got, f"{path}, {name}, g = {g_ranges}: second launch")
        untouched(ws)
        assert int(bits(ws.payload())[0, 0, : COUNTER_BYTES // 4].abs().max()) == 0, "tile counters not re-armed"
    # one byte short of two slabs: refused, nothing written
    ws, _ = _workspace(hip, 1)
    for g in gemms:
        g.new_output()
    assert _launch(hip, gemms, ws, COUNTER_BYTES + 2 * SLOT_BYTES - 1, split_entry) == ERR_ARG
    untouched(ws, *[g.C for g in gemms])
    for g in gemms:
        if g.res == "inplace":  # C started as the residual: still exactly that
            same_bits(g.C.payload(), g.kw["R"], "C of a refused launch")
        else:
            still_unwritten(g.C.payload(), "C of a refused launch")
    still_unwritten(ws.payload()[0, 0, COUNTER_BYTES // 4:], "slabs of a refused launch")


# ---- attention ----------------------------------------------------------------------------------------------------------------------
def _attn_case(hip, kernel, S, Sq, H, B, kind, ws=None, ws_bytes=0):
    """one guarded launch of `kernel` ("f32" | "split3" | "split1"), with the workspace (a Guarded) when one is given; returns the worst ratio"""
    lib, P = hip.lib, lambda t: None if t is None else c_void_p(t.data_ptr())  # noqa: E731
    what = f"attention[{kernel}] S {S} Sq {Sq} H {H} B {B}, bias: {kind}, workspace {ws_bytes}"
    D = H * 128
    q, k, v = R.attn_inputs(B, S, H)
    bias = R.key_bias(S, kind)
    ld = 3 * D + 8
    if kernel == "f32":
        qkv = gin(torch.cat([t.reshape(B, S, D) for t in (q, k, v)], -1), pad=8, gap=2 * ld)
        gb = None if bias is None else gvec(bias)  # the words behind entry S - 1 are poison
    else:
        qkv = gbits(R.attn_operand_rows(q, k, v), ld=ld, gap=2 * ld)
        gb = None if bias is None else gvec(torch.cat([bias, torch.zeros(-S % 32)]))  # 32 * ceil(S / 32) entries, as the header asks
    O = guarded(S, D, D + 8, align_bytes=32, batch=B, batch_stride=S * (D + 8) + 2 * (D + 8))
    Q, K_, V = (qkv.view[:, :, i * D:] for i in range(3))
    kb = None if gb is None else gb.view
    wv = None if ws is None else ws.view
    if kernel == "f32" and ws is None:
        st = (lib.ldc_attn_fwd(P(Q), P(K_), P(V), P(O.view), B, S, H, ld, qkv.bs, O.ld, O.bs, P(kb), hip._stream()) if Sq == S else
              lib.ldc_attn_fwd_qrows(P(Q), P(K_), P(V), P(O.view), B, S, Sq, H, ld, qkv.bs, O.ld, O.bs, P(kb), hip._stream()))
    elif kernel == "f32":
        st = lib.ldc_attn_fwd_ws_qrows(P(Q), P(K_), P(V), P(O.view), B, S, Sq, H, ld, qkv.bs, O.ld, O.bs, P(kb), P(wv), ws_bytes, hip._stream())
    else:
        st = lib.ldc_attn_fwd_split_qrows(P(Q), P(K_), P(V), P(O.view), B, S, Sq, H, ld, qkv.bs, O.ld, O.bs, P(kb), 2 if kernel == "split1" else 0,
                                          P(wv), ws_bytes, hip._stream())
    ok(st, what)
    untouched(qkv, gb, O, ws)
    got = O.payload()
    if Sq < S:
        still_unwritten(got[:, Sq:], what + ": rows >= Sq of O")
    want, bound = R.attn_ref(q, k, v, bias, Sq, kernel)
    return assert_elementwise(finite(got[:, :Sq], what), want, bound, what)


@pytest.mark.parametrize("S", R.ATTN_S)
@pytest.mark.parametrize("kernel", list(R.ATTN_MODES))
def test_attention_edges(hip, kernel, S):
    """at most 18 (query block, head, batch) units: the one-unit-per-workgroup grids with two key groups of both kernels (8 waves).  The
    other schedules - the exact-fp32 kernel's 4-wave form and balanced cut, the split kernel's persistent form with its key-sliced tail -
    need more units than CUs: test_attention_schedules"""
    for Sq, H, B, kind in R.attn_combos(S):
        note("attention", kernel, (S, Sq, H, B, kind), _attn_case(hip, kernel, S, Sq, H, B, kind))


ATTN_SCHEDULES = ("f32, 4-wave form", "f32, balanced cut", "split3, persistent form + tail", "split1, persistent form + tail")


@pytest.mark.parametrize("schedule", ATTN_SCHEDULES)
def test_attention_schedules(hip, schedule):
    """R.ATTN_SCHEDULE_CASE: 260 units of 5 key tiles.  Each schedule is shown to have run by what it leaves in its workspace."""
    S, Sq, H, B, kind = R.ATTN_SCHEDULE_CASE
    kernel = schedule.split(",")[0]
    units = -(-Sq // 128) * H * B
    assert units > 256 and units % 256 <= 128 and units * -(-S // 32) >= 512
    if schedule == "f32, 4-wave form":  # no workspace and more units than CUs: two 4-wave workgroups per CU, one key group
        r = _attn_case(hip, kernel, S, Sq, H, B, kind)
    elif kernel == "f32":
        n = int(hip.lib.ldc_attn_fwd_workspace_bytes())
        ws = guarded(1, n // 4, align_bytes=16, unwritten=False)
        ws.view.zero_()  # zero-filled once by the caller, as the header asks
        r = _attn_case(hip, kernel, S, Sq, H, B, kind, ws, n)
        w = bits(ws.payload())[0, 0]
        assert int(w[:65536].abs().max()) == 0, "ticket counters of the balanced schedule not zero after the launch"
        assert int((w[65536:] != 0).sum()) > 0, "no slab was written: the balanced cut did not run"
        r2 = _attn_case(hip, kernel, S, Sq, H, B, kind, ws, n)  # the same workspace again, nothing re-zeroed
        assert r2 == r
    else:
        n = int(hip.lib.ldc_attn_fwd_split_qrows_workspace_bytes(B, S, Sq, H))
        assert n > 0, "the call shape does not take the tail schedule"
        ws = guarded(1, n // 4, align_bytes=16)  # exactly what the call asks for: the guards sit right behind the last slice
        r = _attn_case(hip, kernel, S, Sq, H, B, kind, ws, n)
        assert int((bits(ws.payload()) != rz._signed(rz.UNWRITTEN32, 32)).sum()) > 0, "no key slice was written: the tail schedule did not run"
    note("attention", schedule, (S, Sq, H, B, kind), r)


# ---- sphere convs -----------------------------------------------------------------------------------------------------------------
CONV_FMT = {"f32": FMT_F32, "bf16x3": FMT_SPLIT, "bf16": FMT_BF16}


def _run_conv(hip, mode, case, act, expect_halo, ws_ranges=64):
    from ladcast_amd.models import sphere_conv as SC

    B, H, W, cin, cout, ks, has_res = case
    what = f"sphere conv[{mode}] {case}"
    fmt = CONV_FMT[mode]
    assert hip.sphere_conv_plan(B, H, W, cin, cout, ks, fmt)[0] == expect_halo, what
    kw = R.conv_inputs(*case)
    rows = kw["x"].reshape(1, B * H * W, cin)
    c8 = (cin + 7) // 8 * 8
    X = gin(rows, pad=c8 - cin + 8, gap=0, align=32) if fmt == FMT_F32 else gbits(operand_rows(rows, fmt), ld=c8 + 8, gap=0)
    wd = kw["w"].cuda()
    Wp = {FMT_F32: SC.pack_dense_weight_f32ring, FMT_SPLIT: SC.pack_dense_weight_bf16x3, FMT_BF16: SC.pack_dense_weight_bf16}[fmt](wd)
    gW = guarded(1, Wp.numel() * Wp.element_size() // 4, align_bytes=16)
    gW.view.view(-1).view(Wp.dtype).copy_(Wp.reshape(-1))
    gb = gvec(kw["bias"])
    Rb = gin(kw["R"].reshape(1, B * H * W, cout), pad=12, gap=0) if has_res else None
    Y = guarded(B * H * W, cout, cout + 4)
    ws, nbytes = _workspace(hip, ws_ranges)
    P = lambda g: None if g is None else c_void_p(g.view.data_ptr())  # noqa: E731
    ok(hip.lib.ldc_sphere_conv_nhwc_split(P(X), P(gW), P(gb), P(Rb), P(Y), B, H, W, cin, X.ld, cout, Y.ld, 0 if Rb is None else Rb.ld, ks, act, fmt, FMT_F32,
                                          P(ws), nbytes, hip._stream()), what)
    untouched(X, gW, gb, Rb, Y, ws)
    got = finite(Y.payload(), what).reshape(B, H, W, cout)
    want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, mode, act=act, R=kw["R"])
    r = assert_elementwise(got, want, bound, what)  # every element: both pole rows, the wrap columns and the frame boundary included
    note("sphere conv" + (" (halo-staged)" if expect_halo else ""), mode, case, r)
    assert int(bits(ws.payload())[0, 0, : COUNTER_BYTES // 4].abs().max()) == 0


@pytest.mark.parametrize("mode", list(CONV_FMT))
@pytest.mark.parametrize("case", R.CONV_CASES, ids=str)
def test_gathered_conv_edges(hip, mode, case):
    """the CONV = true instances of the ring GEMM (exact fp32, split-bf16, single-term bf16) at a few tiles: cin tails 40 / 28, ragged
    output panels 136 / 86, ks 1 / 3 / 5, two frames"""
    _run_conv(hip, mode, case, act=1, expect_halo=False)


def _smallest_halo_shape(hip, fmt):
    """the smallest (frames, H, W) at cin 40, cout 136 that ldc_sphere_conv_plan still hands to the halo-staged kernel, searched by size"""
    best = None
    for B in (2, 3, 4, 6, 8, 12, 16):
        for H in range(4, 41, 2):
            for W in range(8, 81, 4):
                if hip.sphere_conv_plan(B, H, W, 40, 136, 3, fmt)[0] and (best is None or B * H * W < best[0] * best[1] * best[2]):
                    best = (B, H, W)
    return best


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_halo_conv_edges(hip, mode):
    shape = _smallest_halo_shape(hip, CONV_FMT[mode])
    assert shape == R.HALO_CASE[:3], f"smallest shape the plan gives to the halo-staged kernel: {shape}, the case table holds {R.HALO_CASE[:3]}"
    # the plan assumes the full grouped-GEMM workspace (two workgroups per tile need 2 x 128 KiB per tile; with less the gathered kernel runs)
    assert COUNTER_BYTES + 2 * 512 * SLOT_BYTES == hip.lib.ldc_gemm_grouped_workspace_bytes()
    _run_conv(hip, mode, R.HALO_CASE, act=0, expect_halo=True, ws_ranges=512)


# ---- the tile-per-workgroup kernel of gemm_f32.hip: ldc_gemm_bias_act -----------------------------------------------------------------
ERR_ALIGN, ERR_UNSUPPORTED = -2, -3
VP = lambda g: None if g is None else c_void_p(g.view.data_ptr())  # noqa: E731


def _tile_gemm_launch(hip, g):
    p = g.problem(hip)[0]
    return hip.lib.ldc_gemm_bias_act(c_void_p(p.A), c_void_p(p.W), c_void_p(p.bias), c_void_p(p.gate), c_void_p(p.R), c_void_p(p.C), byref(p.d), hip._stream())


@pytest.mark.parametrize("K", R.TILE_GEMM_K)
def test_tile_gemm_edges(hip, K):
    """35 launches per depth (R.tile_gemm_shapes): staging predicated per float4 on kk < K, gm < M, gn < N with poison behind K in A AND W
    (ldw = K + 4), behind N in C, R and the gate, and between the batches; both LDS stages at K = 64, stage 0 reused at K = 96.  The pad
    columns of C are guard words (assert_untouched), the columns before a column offset payload that must still be UNWRITTEN."""
    worst = 0.0
    for M, N, K_, batch, epi in R.tile_gemm_shapes(K):
        what = f"gemm[{TILE_PATH}] {M} x {N} x {K_}, batch {batch}, epilogue {epi}"
        g = Gemm(hip, TILE_PATH, M, N, K_, batch, epi)
        assert g.A.ld > K_ and g.W.ld > K_ and g.C.ld > g.col0 + N and g.A.bs > M * g.A.ld and g.C.bs > M * g.C.ld, what
        assert (g.gate is None or g.gate.bs > N) and (g.Rbuf is None or (g.Rbuf.ld > N and g.Rbuf.bs > M * g.Rbuf.ld)), what
        ok(_tile_gemm_launch(hip, g), what)
        got = g.result(what)
        want, bound = R.gemm_case_ref(M, N, K_, batch, epi, "f32")
        r = assert_elementwise(got, want, bound, what)
        g.new_output()
        ok(_tile_gemm_launch(hip, g), what + ": second launch")
        same_bits(g.result(what + ": second launch"), got, what + ": second launch")
        note("gemm", TILE_PATH, (M, N, K_, batch, epi), r)
        worst = max(worst, r)
    print(f"gemm[{TILE_PATH}] K {K}: worst err / bound {worst:.3f}")


def _refused(st, code, what, outputs, buffers):
    assert st == code, f"{what}: status {st}, expected {code}"
    untouched(*buffers)
    for o in outputs:
        still_unwritten(o.payload(), f"output of the refused call ({what})")


def test_tile_gemm_refusals(hip):
    """every `return` of ldc_gemm_bias_act before its launch.  The two grid-limit cases run at N = 1, K = 4 with lda = ldc = a_bs = c_bs = 0:
    were the check wrong, every workgroup would stay inside row 0 of A and element 0 of C."""
    M = N = K = 8
    g = torch.Generator().manual_seed(5)
    A, W = gin(torch.randn(1, M, K, generator=g)), gin(torch.randn(1, N, K, generator=g), gap=0)
    C = guarded(M, N, N + 4)
    base = dict(A=A.view.data_ptr(), W=W.view.data_ptr(), C=C.view.data_ptr(), desc=True, M=M, N=N, K=K, batch=1, lda=A.ld, ldw=W.ld, ldc=C.ld, a_bs=A.bs,
                c_bs=C.bs, act=0, flags=0)

    def call(**change):
        a = dict(base, **change)
        d = hip.GemmDesc(a["M"], a["N"], a["K"], a["batch"], a["lda"], a["ldw"], a["ldc"], 0, a["a_bs"], a["c_bs"], 0, 0, a["act"], a["flags"], 0)
        return hip.lib.ldc_gemm_bias_act(c_void_p(a["A"]), c_void_p(a["W"]), None, None, None, c_void_p(a["C"]), byref(d) if a["desc"] else None, hip._stream())

    one_row = dict(N=1, K=4, lda=0, ldc=0, a_bs=0, c_bs=0)
    cases = [(dict(A=None), ERR_ARG), (dict(W=None), ERR_ARG), (dict(C=None), ERR_ARG), (dict(desc=False), ERR_ARG)]
    cases += [({k: v}, ERR_ARG) for k in ("M", "N", "K", "batch") for v in (0, -1)]
    cases += [(dict(A=base["A"] + 4), ERR_ALIGN), (dict(W=base["W"] + 4), ERR_ALIGN)]
    cases += [(dict(K=6), ERR_ALIGN), (dict(lda=A.ld + 1), ERR_ALIGN), (dict(ldw=W.ld + 1), ERR_ALIGN), (dict(a_bs=A.bs + 2), ERR_ALIGN)]
    cases += [(dict(act=-1), ERR_UNSUPPORTED), (dict(act=4), ERR_UNSUPPORTED), (dict(flags=1), ERR_UNSUPPORTED), (dict(flags=8), ERR_UNSUPPORTED)]
    cases += [(dict(one_row, batch=65536), ERR_UNSUPPORTED), (dict(one_row, M=65535 * 128 + 1), ERR_UNSUPPORTED)]
    for change, code in cases:
        _refused(call(**change), code, f"ldc_gemm_bias_act with {change}", [C], [A, W, C])
    ok(call(), "the call that every refusal above changes in one argument")
    untouched(A, W, C)
    want, bound = R.gemm_ref(A.payload(), W.payload()[0])
    assert_elementwise(finite(C.payload(), "the accepted call"), want, bound, "the accepted call")


# ---- the tile-per-workgroup kernel of gemm_f32.hip: ldc_sphere_conv_nhwc --------------------------------------------------------------
def _tile_conv(hip, case, act, via_gather=False):
    from ladcast_amd.models.sphere_conv import pack_dense_weight

    B, H, W, cin, cout, ks, has_res = case
    what = f"sphere conv[{TILE_PATH}] {case}, act {act}"
    kw = R.conv_inputs(*case)
    npix = B * H * W
    X = gin(kw["x"].reshape(1, npix, cin), gap=0)  # ldx = cin + 4: a float4 that reaches behind cin reads poison
    gW = gvec(pack_dense_weight(kw["w"]))  # [cout][ks * ks * cin], dense: the back guard starts behind row cout - 1
    gb = gvec(kw["bias"])
    Rb = gin(kw["R"].reshape(1, npix, cout), gap=0) if has_res else None
    outs = []
    for rep in range(2):
        Y = guarded(npix, cout, cout + 4)
        ok(hip.lib.ldc_sphere_conv_nhwc(VP(X), VP(gW), VP(gb), VP(Rb), VP(Y), B, H, W, cin, X.ld, cout, Y.ld, 0 if Rb is None else Rb.ld, ks, act, hip._stream()),
           what)
        untouched(X, gW, gb, Rb, Y)  # (the pad columns of Y are guard words)
        outs.append(finite(Y.payload(), what).reshape(B, H, W, cout))
    want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32", act=act, R=kw["R"], via_gather=via_gather)
    r = assert_elementwise(outs[0], want, bound, what)  # every element: both pole rows, the wrap columns and the image boundaries included
    same_bits(outs[1], outs[0], what + ": second launch")
    note("sphere conv", TILE_PATH, case + (act,), r)
    return r


@pytest.mark.parametrize("act", (0, 1))
@pytest.mark.parametrize("case", R.TILE_CONV_CASES, ids=str)
def test_tile_conv_edges(hip, case, act):
    """what each case is for is written beside R.TILE_CONV_CASES"""
    _tile_conv(hip, case, act)


@pytest.mark.parametrize("act", (0, 1))
def test_tile_conv_two_rows(hip, act):
    """H = 2: the entry point accepts it, the oracle and the reference raise there.  Held to the float64 gather-GEMM over R.sphere_gather,
    which tests/test_mfma_edge_bounds_cpu.py shows to equal the oracle conv at every H >= 3 case"""
    _tile_conv(hip, R.TILE_CONV_H2_CASE, act, via_gather=True)


def test_sphere_conv_module_with_padded_cin(hip):
    """SphereConv2d(6, 5, 3, 1, 1) on (2, 6, 4, 8): cin is padded to 8 with zero weights, so columns 6 and 7 of the token buffer must BE zeros
    (0 x NaN is NaN).  The module takes that buffer from torch.empty: the allocator is first handed freed blocks full of NaN of every size
    the forward asks for, and the layout kernel is shown directly to zero the columns of a NaN-filled buffer."""
    from ladcast_amd.models import SphereConv2d

    B, H, W, cin, cout, ks, _ = R.MODULE_CONV_CASE
    kw = R.conv_inputs(*R.MODULE_CONV_CASE)
    x = kw["x"].permute(0, 3, 1, 2).contiguous().cuda()
    tok = torch.full((B, H * W, 8), float("nan"), device="cuda")
    hip.chan_to_token(x, tok, B=B, C=cin, N=H * W, ldo=8)
    assert bool((tok[..., cin:] == 0).all()) and torch.equal(tok[..., :cin].cpu(), kw["x"].reshape(B, H * W, cin))
    m = SphereConv2d(cin, cout, ks, 1, 1).cuda()
    with torch.no_grad():
        m.weight.copy_(kw["w"])
        m.bias.copy_(kw["bias"])
    torch.cuda.synchronize()
    junk = [torch.full((n,), float("nan"), device="cuda") for n in (B * H * W * 8, B * H * W * cout, cout * ks * ks * 8) for _ in range(4)]
    del tok, junk
    y = m(x)
    torch.cuda.synchronize()
    want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32")
    got = finite(y.cpu(), "SphereConv2d(6, 5, 3)").permute(0, 2, 3, 1)
    note("sphere conv", "SphereConv2d module", R.MODULE_CONV_CASE, assert_elementwise(got, want, bound, "SphereConv2d(6, 5, 3)"))


def test_tile_conv_refusals(hip):
    """every `return` of ldc_sphere_conv_nhwc before its launch but one: the pixel-count limit (B H W above 2**31 - 1, or above 65535 row
    tiles) is NOT run here - ldx >= cin is required, so a wrongly accepted call would read gigabytes behind X on a shared machine.  It is
    covered by reading: `M` is formed in 64 bits from the three extents, compared with 0x7fffffff and, divided by 128 and rounded up, with
    65535, before anything is narrowed to int."""
    B, H, W, cin, cout, ks = 1, 3, 4, 8, 8, 3
    g = torch.Generator().manual_seed(7)
    x, w = torch.randn(B, H, W, cin, generator=g), torch.randn(cout, cin, ks, ks, generator=g) / 8
    X, Wt = gin(x.reshape(1, B * H * W, cin), gap=0), gvec(w.permute(0, 2, 3, 1).reshape(-1))
    Y = guarded(B * H * W, cout, cout + 4)
    base = dict(X=X.view.data_ptr(), Wt=Wt.view.data_ptr(), Y=Y.view.data_ptr(), B=B, H=H, W=W, cin=cin, ldx=X.ld, cout=cout, ldy=Y.ld, ksize=ks, act=0)

    def call(**change):
        a = dict(base, **change)
        return hip.lib.ldc_sphere_conv_nhwc(c_void_p(a["X"]), c_void_p(a["Wt"]), None, None, c_void_p(a["Y"]), a["B"], a["H"], a["W"], a["cin"], a["ldx"], a["cout"],
                                            a["ldy"], 0, a["ksize"], a["act"], hip._stream())

    cases = [(dict(X=None), ERR_ARG), (dict(Wt=None), ERR_ARG), (dict(Y=None), ERR_ARG)]
    cases += [({k: v}, ERR_ARG) for k in ("B", "H", "W", "cin", "cout") for v in (0, -2)]
    cases += [(dict(ksize=k), ERR_UNSUPPORTED) for k in (1, 4, 7)]
    cases += [(dict(W=3), ERR_UNSUPPORTED), (dict(H=1), ERR_UNSUPPORTED)]
    cases += [(dict(X=base["X"] + 4), ERR_ALIGN), (dict(Wt=base["Wt"] + 4), ERR_ALIGN)]
    cases += [(dict(cin=6), ERR_ALIGN), (dict(ldx=X.ld + 1), ERR_ALIGN), (dict(ldx=cin - 4), ERR_ALIGN), (dict(ldy=cout - 4), ERR_ALIGN)]
    cases += [(dict(act=-1), ERR_UNSUPPORTED), (dict(act=4), ERR_UNSUPPORTED)]
    for change, code in cases:
        _refused(call(**change), code, f"ldc_sphere_conv_nhwc with {change}", [Y], [X, Wt, Y])
    ok(call(), "the call that every refusal above changes in one argument")
    untouched(X, Wt, Y)
    want, bound = R.conv_ref(x, w, None, ks, "f32")
    assert_elementwise(finite(Y.payload(), "the accepted call").reshape(B, H, W, cout), want, bound, "the accepted call")
