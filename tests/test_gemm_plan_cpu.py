"""The grouped GEMMs' host planner, pinned without a GPU: `hip.gemm_plan` (ldc_gemm_grouped_plan - the code that plans the launches
themselves, csrc/gemm_plan.hip) against tests/golden/gemm_plan_parent.json, the cuts RECORDED from the commit before the planner was
moved behind one module: its A/B library printed every launch's cut on an MI355X (terms, n, tiles, k-depth of problem 0, tile rows,
workgroups, units).  The groups: every distinct grouped launch of a 375M and a 1.6B forward at (B, Nx, Nc) = (1, 1800, 450) in the three
arithmetics, the shapes of tools/vendor_gemm_yardstick.py, the edge and sweep shapes of tests/mfma_edge_refs.py, a few anchors.  The
problems are rebuilt with made-up addresses of the recorded alignment: the planner reads no buffer.

What the record does not hold, and how it is covered: `super_row` (the parent printed no rm) - two hand-derived anchors plus
super_row == tile_rows_m for every problem below 48e6 activation bytes; register-staged launches print no line - the record says "no
line", the plan must say "register-staged".  The gathered convs of the record plan through ldc_sphere_conv_nhwc_split, not through this
query (their tile-height rule, 200 tiles, is the conv's own): the four whose tile height the GEMM rule shares are compared through the
equivalent GEMM problem."""
import json
import os
import types

import pytest

import ladcast_amd.hip as hip
from benchlib.kernel_timer import KernelTimer

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_parent.json")))
PTRS = ("A", "W", "bias", "gate", "R", "C")


def fake(mod, k):
    """a made-up address with the recorded address % 64 (None stays NULL)"""
    return None if mod is None else (k + 1) * (1 << 32) + mod


def problems_of(rec):
    """[(GemmProblem, None)] as `hip.gemm_problem` returns them, from a recorded group"""
    out = []
    for i, p in enumerate(rec["problems"]):
        d = hip.GemmDesc(*[p[k] for k, _ in hip.GemmDesc._fields_])
        out.append((hip.GemmProblem(*[fake(p[k], 8 * i + j) for j, k in enumerate(PTRS)], d), None))
    return out


def epilogues_of(rec):
    if rec["epilogues"] is None:
        return None
    out = []
    for i, e in enumerate(rec["epilogues"]):
        out.append(None if e is None else (hip.QkvEpilogue(fake(e["wq"], 100 + 4 * i), fake(e["wk"], 101 + 4 * i), fake(e["rope"], 102 + 4 * i), None,
                                                          e["eps"], e["qscale"], e["heads"], e["rope_row0"]), None))
    return out


def plan_of(rec):
    return hip.gemm_plan(problems_of(rec), epilogues_of(rec), split_bf16=rec["entry"] in ("split", "qkv"))


def cdiv(a, b):
    return -(-a // b)


def check_against_cuts(plan, probs, cuts, what):
    """every field of the plan against the recorded cut lines (integers, exactly)"""
    if not cuts:  # no line: the parent ran a register-staged kernel
        assert (plan.kernel, plan.launches, plan.tile_rows[0]) == (hip.GEMM_KERNEL_REGSTAGE, 1, 128), what
        return
    assert (plan.kernel, plan.launches, plan.terms) == (hip.GEMM_KERNEL_RING, len(cuts), cuts[0]["terms"]), what
    first = 0
    for l, c in enumerate(cuts):
        mine = probs[first:first + c["n"]]
        bm, kstep = c["BM"], 64 if c["terms"] == 1 else 32
        got = (plan.tile_rows[l], plan.workgroups[l], plan.units[l], plan.tiles[l], plan.units_per_group[l], plan.units_rem[l])
        assert got == (bm, c["G"], c["U"], c["tiles"], c["U"] // c["G"], c["U"] % c["G"]), f"{what}, launch {l}: {got} vs {c}"
        assert c["terms"] == plan.terms and plan.k_steps[first] == c["kt0"], f"{what}, launch {l}"
        tiles = units = 0
        for i, p in enumerate(mine, first):
            assert (plan.tile_rows_m[i], plan.tile_cols_n[i], plan.k_steps[i]) == (cdiv(p["M"], bm), cdiv(p["N"], 128), p["K"] // kstep), f"{what}, problem {i}"
            if 4.0 * p["batch"] * p["M"] * p["K"] < 48e6:
                assert plan.super_row[i] == plan.tile_rows_m[i], f"{what}, problem {i}: one super-row below 48e6 activation bytes"
            assert 1 <= plan.super_row[i] <= plan.tile_rows_m[i]
            tiles += p["batch"] * plan.tile_rows_m[i] * plan.tile_cols_n[i]
            units += p["batch"] * plan.tile_rows_m[i] * plan.tile_cols_n[i] * plan.k_steps[i]
        assert (tiles, units) == (c["tiles"], c["U"]), f"{what}, launch {l}"
        first += c["n"]
    assert first == len(probs), what


def test_recorded_groups_cover_the_listed_sources():
    src = {g["source"].split(",")[0] for g in GOLD["groups"]}
    assert {"375M forward", "1.6B forward", "edge shape", "256-row tile"} <= src
    full = {g["source"] for g in GOLD["groups"]}
    assert sum(s.startswith("yardstick") for s in full) == 9 * 3 and sum(s.startswith("sweep") for s in full) == 5 * 3  # x the three arithmetics
    assert {g["entry"] for g in GOLD["groups"] if g["source"].startswith("375M")} == {"f32", "split", "qkv", "qkv_f32"}
    assert GOLD["workspace_bytes"] == hip.lib.ldc_gemm_grouped_workspace_bytes()


def test_plans_equal_the_parents_recorded_cuts():
    kinds = set()
    for rec in GOLD["groups"]:
        plan = plan_of(rec)
        check_against_cuts(plan, rec["problems"], rec["cuts"], f"{rec['source']} [{rec['entry']}] {[(p['M'], p['N'], p['K'], p['batch']) for p in rec['problems']]}")
        kinds.add((plan.kernel, plan.terms, plan.tile_rows[0], plan.launches > 1))
    # both kernels, the three arithmetics, both tile heights and a group launched problem by problem are all in the record
    assert {(k, t) for k, t, _, _ in kinds} == {(0, 0), (0, 1), (0, 3), (1, 0), (1, 3)}
    assert {(0, 3, 256, False), (0, 1, 256, False), (0, 3, 128, True), (0, 1, 128, True)} <= kinds


def _one(M, N, K, mode, batch=1, flags=0):
    base = {"f32": 0, "split": hip.GEMM_A_SPLIT, "bf16": hip.GEMM_A_SPLIT | hip.GEMM_BF16_1TERM}[mode] | flags
    d = hip.GemmDesc(M, N, K, batch, K, K, N, 0, M * K, M * N, 0, 0, 0, base, 0)
    return (hip.GemmProblem(fake(0, 1), fake(0, 2), None, None, None, fake(0, 3), d), None)


def test_anchor_cuts():
    """the hand-derived cuts of the planner's branches (each also agrees with the record above)"""
    p = hip.gemm_plan([_one(1800, 84, 1536, "split")], split_bf16=True)  # few tiles: 15 tiles x 48 k-steps, s = 6
    assert (p.tile_rows[0], p.tiles[0], p.k_steps[0], p.workgroups[0], p.units_per_group[0], p.units_rem[0]) == (128, 15, 48, 90, 8, 0)
    p = hip.gemm_plan([_one(2304, 2048, 10240, "split")], split_bf16=True)  # aligned, s = 5
    assert (p.tiles[0], p.k_steps[0], p.workgroups[0]) == (288, 320, 240)
    p = hip.gemm_plan([_one(1920, 2048, 256, "split"), _one(512, 2048, 256, "split")], split_bf16=True)  # 304 tiles, no aligned cut: one by one
    assert (p.launches, p.workgroups[0], p.tiles[0], p.tiles[1], p.k_steps[0]) == (2, 240, 240, 64, 8)
    p = hip.gemm_plan([_one(1920, 2048, 256, "f32"), _one(512, 2048, 256, "f32")])  # exact fp32 keeps the group
    assert (p.launches, p.tiles[0], p.workgroups[0]) == (1, 304, 256)
    p = hip.gemm_plan([_one(2250, 4608, 1536, "f32")])  # one range per CU
    assert (p.kernel, p.tile_rows[0], p.terms, p.tiles[0], p.units[0], p.workgroups[0], p.units_per_group[0], p.units_rem[0]) == (0, 128, 0, 648, 31104, 256, 121, 128)
    p = hip.gemm_plan([_one(2250, 1536, 7680, "split")], split_bf16=True)  # 69 MB activation panel: super-rows
    assert (p.tile_rows_m[0], p.super_row[0]) == (18, 6)
    p = hip.gemm_plan([_one(2250, 4608, 1536, "split")], split_bf16=True)  # 14 MB panel: one super-row
    assert (p.tile_rows_m[0], p.super_row[0]) == (18, 18)
    for K in (64, 1536):
        p = hip.gemm_plan([_one(5000, 2688, K, "split")], split_bf16=True)  # 20 x 21 = 420 tiles of 256 rows
        assert (p.tile_rows[0], p.tiles[0]) == (256, 420)
    assert hip.gemm_plan([_one(4999, 2560, 64, "split")], split_bf16=True).tile_rows[0] == 256  # 400 tiles: the threshold itself
    assert hip.gemm_plan([_one(4864, 2688, 64, "split")], split_bf16=True).tile_rows[0] == 128  # 399
    for prob in (_one(300, 260, 36, "f32"), _one(2250, 4608, 1536, "f32", flags=hip.GEMM_F32_REGSTAGE), _one(300, 260, 64, "f32", batch=2)):
        regstage = prob[0].d.K == 36 or bool(prob[0].d.flags)
        assert hip.gemm_plan([prob]).kernel == (hip.GEMM_KERNEL_REGSTAGE if regstage else hip.GEMM_KERNEL_RING)
    assert hip.gemm_plan([_one(300, 260, 64, "f32")], split_bf16=True).kernel == hip.GEMM_KERNEL_REGSTAGE  # fp32 A in the split entry


def test_refusals_have_the_launch_status():
    for r in GOLD["refusals"]:
        arr = (hip.GemmProblem * len(r["problems"]))(*[p[0] for p in problems_of(r)])
        plan = hip.GemmPlan()
        st = hip.lib.ldc_gemm_grouped_plan(arr, None, r["n"], int(r["entry"] == "split"), GOLD["workspace_bytes"], plan)
        assert st == r["status"], f"{r['what']}: status {st}, the launch returned {r['status']}"
        assert plan.launches == 0 and plan.workgroups[0] == 0
    with pytest.raises(RuntimeError, match="status -2"):
        hip.gemm_plan([(hip.GemmProblem(fake(4, 1), fake(0, 2), None, None, None, fake(0, 3), _one(300, 260, 64, "f32")[0].d), None)])
    # a workspace one byte short of two slabs, and the exact-fp32 ring kernel's own floor (two 256-row slabs: below it, the register-staged kernel)
    arr, plan = (hip.GemmProblem * 1)(_one(300, 260, 64, "f32")[0]), hip.GemmPlan()
    assert hip.lib.ldc_gemm_grouped_plan(arr, None, 1, 0, (1 << 20) + 2 * 128 * 128 * 4 - 1, plan) == -1
    assert hip.lib.ldc_gemm_grouped_plan(arr, None, 1, 0, (1 << 20) + 2 * 128 * 128 * 4, plan) == 0 and (plan.kernel, plan.workgroups[0]) == (1, 1)
    assert hip.lib.ldc_gemm_grouped_plan(arr, None, 1, 0, (1 << 20) + 2 * 256 * 128 * 4, plan) == 0 and (plan.kernel, plan.workgroups[0]) == (0, 2)
    assert hip.lib.ldc_gemm_grouped_plan(arr, None, 1, 0, GOLD["workspace_bytes"], None) == -1


def test_kernel_timer_names_are_the_parents():
    """benchlib/kernel_timer.py names a launch by its plan: for every grouped launch of the 375M forward in the three modes (the default
    workload and the bf16 mixed one) the name is the string its hand-written mirror produced at the parent"""
    names = []
    ns = types.SimpleNamespace(**{k: (lambda *a, **kw: None) for k in KernelTimer.WRAPPED}, gemm_kernel_name=hip.gemm_kernel_name)
    timer = KernelTimer()
    timer._bracket = lambda name, work, fn, *a, **kw: names.append(name)
    timer.install(ns)
    recs = [g for g in GOLD["groups"] if g["source"].startswith("375M forward")]
    for rec in recs:
        probs, epis = problems_of(rec), epilogues_of(rec)
        if rec["entry"] == "qkv":
            ns.gemm_grouped_qkv(probs, epis)
        elif rec["entry"] == "qkv_f32":
            ns.gemm_grouped_qkv_f32(probs, epis)
        else:
            ns.gemm_grouped(probs, split_bf16=rec["entry"] == "split")
    assert names == [r["timer_name"] for r in recs]
    assert set(names) == {f"gemm_bf16x3_v3_kernel<{bm}, {terms}, false>" for bm, terms in ((128, 0), (128, 3), (256, 3), (128, 1), (256, 1))}


def test_gathered_conv_cuts_through_the_equivalent_gemm():
    compared = 0
    for c in GOLD["convs"]:
        (cut,) = c["cuts"]
        one = c["in_fmt"] == hip.FMT_BF16
        mode = "f32" if c["in_fmt"] == hip.FMT_F32 else "bf16" if one else "split"
        M, K = c["B"] * c["H"] * c["W"], c["ksize"] ** 2 * c["cin"]
        assert (cut["conv"], cut["tiles"], cut["U"]) == (1, cdiv(M, cut["BM"]) * cdiv(c["cout"], 128), cdiv(M, cut["BM"]) * cdiv(c["cout"], 128) * cut["kt0"])
        if cut["BM"] == 128:  # (256-row conv tiles start at 200 tiles, the GEMM's at 400: not reachable through this query)
            check_against_cuts(hip.gemm_plan([_one(M, c["cout"], K, mode)], split_bf16=mode != "f32"), [dict(M=M, N=c["cout"], K=K, batch=1)], c["cuts"], f"conv {c}")
            compared += 1
    assert compared == 4
