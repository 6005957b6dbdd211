"""Edge tests of the scoring kernels (csrc/scoring.hip) through their three entry points - ldc_ensemble_scores (with both point maps),
ldc_rollout_scores, ldc_validation_scores - against the float64 oracle and the DERIVED bounds of tests/score_edge_refs.py (judged on the
CPU by tests/test_score_edge_bounds_cpu.py):
  a. every M in 1..64 on small integers (all eight sort arms, every dispatch boundary, the INV and SINGLE templates): the point maps are
     the float64 value rounded once, bit for bit; the grid scores within their bounds; the entry points give each other's bits
  b. physical scale (geopotential 2e5 +- 1e2, MSLP 101325 +- 150, ...) through the fused inverse normalisation
  c. the finish loop: 65 and 129 workgroup records per plane, and one NaN member in the last record
  d. guard bands around every buffer, strides above the extents, both forecast layouts, slot tables; inputs poisoned with the largest
     finite fp32 (NaN is a legal input here), outputs UNWRITTEN
  e. the NaN / inf table against the reference's rules (oracle/scoring.py is the contract)

LDC_SCORE_EDGE_RATIOS=<file>: the worst err / bound ratio of every case, with the ratio of the reference's own fp32 arithmetic for the
same case beside it, is written there as JSON (profiles/score_edge_worst_ratios.json)."""
import ctypes
import json
import os

import pytest
import torch

from oracle import scoring as S
from tests import score_edge_refs as R
from tests.redzone import UNWRITTEN32, assert_untouched, guarded

pytestmark = pytest.mark.gpu

RATIOS = []
GROUPS = ("maps", "scores", "validation")


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    yield eu
    out = os.environ.get("LDC_SCORE_EDGE_RATIOS")
    if out:
        with open(out, "w") as f:
            json.dump(RATIOS, f, indent=0)


def note(case, ratio, oracle_ratio, **more):
    RATIOS.append(dict(case=case, ratio=round(ratio, 4), oracle_fp32_ratio=round(oracle_ratio, 4), **more))


def oracle_ratio(x, t, cl, w, nan_channel, ref, groups=GROUPS):
    got = R.oracle_f32(x, t, cl, w, nan_channel)
    return max(R.ratio_of(got[g][k], *ref[g][k]) for g in groups for k in ref[g])


def ensemble(E, x, t, cl, w, nan_channel=-1):
    """ldc_ensemble_scores with both maps on device tensors -> maps / scores as score_edge_refs.scores_ref"""
    out, skill, spread = E._scores(x, t, cl, w, nan_channel, True)
    return dict(maps=dict(skill=skill, spread=spread), scores={k: out[i] for i, k in enumerate(R.KEYS)})


def judge_group(got, ref, group, what):
    worst = 0.0
    for k, r in ref[group].items():
        v = got[group][k] if group in got else got[k]
        print(f"{what} {group} {k}: err / bound {R.ratio_of(v, *r):.4f}, relative error {R.relative_errors(v, r[0]):.3e}")
        worst = max(worst, R.judge(v, r, f"{what} {group} {k}"))
    return worst


def maps_exact(got, ref, what):
    for k in ("skill", "spread"):
        assert R.same_bits(got["maps"][k], ref["maps"][k][0].float()), f"{what}: {k}_map is not the float64 value rounded once"


# ---- a. every M, bit-exact on integers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.ALL_M)
def test_every_ensemble_size_on_integers(E, M):
    c = R.integer_case(M)
    x, t, cl, w = c["x"], c["t"], c["cl"], c["w"]
    xd, td, cd, wd = x.cuda(), t.cuda(), cl.cuda(), w.cuda()
    ref = R.scores_ref(x, t, cl, w)
    got = ensemble(E, xd, td, cd, wd)
    maps_exact(got, ref, f"M={M}")
    r = judge_group(got, ref, "scores", f"M={M}")
    # one channel through the other two entry points and templates: INV off, INV on with the identity, INV on with powers of two
    ch = slice(1, 2)
    x1, t1, c1 = xd[:, ch, None], td[ch, None], cd[ch, None]  # (M, 1, 1, H, W), (1, 1, H, W)
    one, zero = torch.ones(1, device="cuda"), torch.zeros(1, device="cuda")
    roll = E.rollout_scores(x1, t1, c1, wd, -1)
    roll_id = E.rollout_scores(x1, t1, c1, wd, -1, mean=zero, std=one, target_std=1.0)
    for k in R.KEYS:
        assert R.same_value_bits(roll[k][:, 0], got["scores"][k][ch]), (k, "rollout_scores against ensemble_scores")
        assert R.same_value_bits(roll_id[k][:, 0], roll[k][:, 0]), (k, "fused identity normalisation")
    val = E.validation_scores(x1, t1, wd)
    val_id = E.validation_scores(x1, t1, wd, mean=zero, std=one, target_std=1.0)
    noclim = E.rollout_scores(x1, t1, None, wd, -1)
    for k in ("ens_mse", "crps"):
        assert R.same_value_bits(val[k], noclim[k]) and R.same_value_bits(val[k], roll[k]), (k, "validation_scores against rollout_scores")
    for k in R.VKEYS:
        assert R.same_value_bits(val_id[k], val[k]), (k, "fused identity normalisation, validation")
    rv = R.judge(val["single_mse"][:, 0], tuple(v[ch] for v in ref["validation"]["single_mse"]), f"M={M} single_mse")
    n = R.POW2_NORM
    mean, std = torch.tensor(n["mean"][1:]), torch.tensor(n["std"][1:])
    x2 = R.inv_norm_f32(x[:, ch], mean, std, n["target_std"])  # exact: integers again
    ref2 = R.scores_ref(x2, t[ch], cl[ch], w)
    got2 = ensemble(E, x2.cuda(), td[ch], cd[ch], wd)
    maps_exact(got2, ref2, f"M={M}, power-of-two normalisation")
    r2 = judge_group(got2, ref2, "scores", f"M={M} pow2")
    roll2 = E.rollout_scores(x1, t1, c1, wd, -1, mean=mean.cuda(), std=std.cuda(), target_std=n["target_std"])
    val2 = E.validation_scores(x1, t1, wd, mean=mean.cuda(), std=std.cuda(), target_std=n["target_std"])
    val2_plain = E.validation_scores(x2.cuda()[:, :, None], t1, wd)
    for k in R.KEYS:
        assert R.same_value_bits(roll2[k][:, 0], got2["scores"][k]), (k, "fused power-of-two normalisation")
    for k in R.VKEYS:
        assert R.same_value_bits(val2[k], val2_plain[k]), (k, "fused power-of-two normalisation, validation")
    note(f"integers M={M} arm {R.sort_arm(M)}", max(r, rv, r2), oracle_ratio(x, t, cl, w, -1, ref, ("scores", "validation")), maps="bit-exact")


# ---- b. physical scale ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M):
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D

    c = R.physical_case(M)
    L = c["x"].shape[2]
    vd, td, cd, wd = c["v"].cuda(), c["t"].cuda(), c["cl"].cuda(), c["w"].cuda()
    md, sd = c["mean"].cuda(), c["std"].cuda()
    xd = inverse_normalize_transform_3D(vd, md, sd, c["target_std"])
    assert R.same_bits(xd, c["x"])  # the bits the oracle starts from
    roll = E.rollout_scores(vd, td, cd, wd, -1, mean=md, std=sd, target_std=c["target_std"])
    val = E.validation_scores(vd, td, wd, mean=md, std=sd, target_std=c["target_std"])
    worst, worst_o, rel = 0.0, 0.0, {}
    for l in range(L):
        x, t, cl = c["x"][:, :, l], c["t"][:, l], c["cl"][:, l]
        ref = R.scores_ref(x, t, cl, c["w"])
        got = ensemble(E, xd[:, :, l], td[:, l], cd[:, l], wd)
        worst = max(worst, judge_group(got, ref, "maps", f"M={M} lead {l}"), judge_group(got, ref, "scores", f"M={M} lead {l} ensemble_scores"))
        worst = max(worst, judge_group({k: roll[k][:, l] for k in R.KEYS}, ref, "scores", f"M={M} lead {l} rollout_scores"))
        worst = max(worst, judge_group({k: val[k][:, l] for k in R.VKEYS}, ref, "validation", f"M={M} lead {l} validation_scores"))
        for k in R.KEYS:
            assert R.same_value_bits(roll[k][:, l], got["scores"][k]), (k, l)
        worst_o = max(worst_o, oracle_ratio(x, t, cl, c["w"], -1, ref))
        for i, p in enumerate(R.PHYS):  # relative errors actually seen, per channel (for the record)
            e = rel.setdefault(p[0], dict(ens_mse=0.0, spread_point=0.0))
            e["ens_mse"] = max(e["ens_mse"], R.relative_errors(got["scores"]["ens_mse"][i], ref["scores"]["ens_mse"][0][i]))
            e["spread_point"] = max(e["spread_point"], R.relative_errors(got["maps"]["spread"][i], ref["maps"]["spread"][0][i]))
    note(f"physical M={M}", worst, worst_o, relative_error={k: {q: float(f"{v:.3g}") for q, v in e.items()} for k, e in rel.items()})


# ---- c. the finish loop --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.FINISH_SHAPES)
def test_finish_loop(E, H, W):
    c = R.finish_case(H, W)
    x, t, cl, w = c["x"], c["t"], c["cl"], c["w"]
    ref = R.scores_ref(x, t, cl, w)
    got = ensemble(E, x.cuda(), t.cuda(), cl.cuda(), w.cuda())
    r = max(judge_group(got, ref, "maps", f"{H}x{W}"), judge_group(got, ref, "scores", f"{H}x{W}"))
    note(f"finish loop {H}x{W}: {-(-H * W // R.TPB)} records", r, oracle_ratio(x, t, cl, w, -1, ref, ("maps", "scores")))
    xn = x.clone()
    xn[1, 0, H - 1, W - 1] = float("nan")  # the last thread of the last record
    for nan_channel in (-1, 0):
        ref = R.scores_ref(xn, t, cl, w, nan_channel)
        got = ensemble(E, xn.cuda(), t.cuda(), cl.cuda(), w.cuda(), nan_channel)
        for k in ("ens_mse", "crps_spread", "crps_skill", "crps"):  # the count rule: plain mean -> NaN, nanmean -> the other points
            assert bool(torch.isnan(got["scores"][k]).all()) == (nan_channel < 0), (k, nan_channel)
        assert bool(torch.isfinite(got["scores"]["ens_acc"]).all())
        judge_group(got, ref, "maps", f"{H}x{W} NaN member")
        judge_group(got, ref, "scores", f"{H}x{W} NaN member, nan_channel {nan_channel}")


# ---- d. guard bands --------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", R.GUARD_CASES)
def test_guard_bands(E, case, layout):
    from ladcast_amd import hip

    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    HW, ld, FMAX = H * W, H * W + 8, R.FLT_MAX_BITS
    inp = dict(poison=FMAX, unwritten=False)
    if layout == "ens_C_L_H_W":  # planes ld apart, channels L * ld, members further than C * L * ld
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(c["x"].reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:  # the decoder's (L * ens, C, H, W) frames: channels ld, members C * ld, lead times further than ens * C * ld
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(c["x"].permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gt = guarded(C, HW, ld, batch=R.N_TRUTH, batch_stride=C * ld + 16, **inp).fill(c["truth_table"].reshape(R.N_TRUTH, C, HW))
    gc = guarded(C, HW, ld, batch=R.N_CLIM, batch_stride=C * ld + 16, **inp).fill(c["clim_table"].reshape(R.N_CLIM, C, HW))
    gl = guarded(1, H, **inp).fill(c["w"])
    # a slot read from a guard word points one entry past its table, into the table's poisoned back guard (gt.bs, gc.bs < the guard)
    assert max(gt.bs, gc.bs) < 4096
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    gcs = guarded(1, L, dtype=torch.int32, poison=R.N_CLIM, unwritten=False).fill(torch.tensor(c["c_slots"]))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    inputs = dict(forecast=gf, truth=gt, clim=gc, lat_weight=gl, truth_slot=gts, clim_slot=gcs, mean=gm, std=gs)

    def untouched(extra):
        torch.cuda.synchronize()
        for k, g in {**inputs, **extra}.items():
            assert_untouched(g, k)

    # ldc_rollout_scores, forecast in physical units
    nbytes = int(hip.lib.ldc_rollout_scores_workspace_bytes(C, L, H, W))
    gw, go = guarded(1, nbytes // 4, unwritten=False), guarded(5 * C, Lt)
    assert hip.lib.ldc_rollout_scores(_p(gf.view), ms, ls, cs, None, None, 1.0, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gc.view), gc.bs, ld, _p(gcs.view),
                                      _p(gl.view), M, C, L, H, W, sst, _p(go.view), Lt, 1, _p(gw.view), nbytes, stream) == 0
    untouched(dict(workspace=gw, out=go))
    roll = go.payload()[0].reshape(5, C, Lt)
    assert _unwritten(roll[:, :, 0]) and _unwritten(roll[:, :, L + 1])
    # ldc_validation_scores with the fused inverse normalisation
    nbytes = int(hip.lib.ldc_validation_scores_workspace_bytes(C, L, H, W))
    gwv, gv = guarded(1, nbytes // 4, unwritten=False), guarded(3 * C, Lt)
    assert hip.lib.ldc_validation_scores(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gl.view), M, C, L, H, W,
                                         _p(gv.view), Lt, 1, _p(gwv.view), nbytes, stream) == 0
    untouched(dict(workspace=gwv, out=gv))
    val = gv.payload()[0].reshape(3, C, Lt)
    assert _unwritten(val[:, :, 0]) and _unwritten(val[:, :, L + 1])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    worst = worst_o = 0.0
    nbytes = int(hip.lib.ldc_ensemble_scores_workspace_bytes(C, H, W))
    for l in range(L):
        t, cl = c["truth_table"][c["t_slots"][l]], c["clim_table"][c["c_slots"][l]]
        ref = R.scores_ref(c["x"][:, :, l], t, cl, c["w"], sst)
        worst = max(worst, judge_group({k: roll[i, :, 1 + l] for i, k in enumerate(R.KEYS)}, ref, "scores", f"lead {l} rollout_scores"))
        refv = R.scores_ref(xp[:, :, l], t, None, c["w"])
        worst = max(worst, judge_group({k: val[i, :, 1 + l] for i, k in enumerate(R.VKEYS)}, refv, "validation", f"lead {l} validation_scores"))
        # ldc_ensemble_scores on the same buffers: this lead time's planes, the slot's truth and climatology entries, both maps
        gwe, ge, gk, gp = guarded(1, nbytes // 4, unwritten=False), guarded(5, C), guarded(C, HW), guarded(C, HW)
        fc = ctypes.c_void_p(gf.view.data_ptr() + 4 * l * ls)
        tr = ctypes.c_void_p(gt.view.data_ptr() + 4 * c["t_slots"][l] * gt.bs)
        cp = ctypes.c_void_p(gc.view.data_ptr() + 4 * c["c_slots"][l] * gc.bs)
        assert hip.lib.ldc_ensemble_scores(fc, ms, cs, tr, ld, cp, ld, _p(gl.view), M, C, H, W, sst, _p(ge.view), _p(gk.view), _p(gp.view), _p(gwe.view), nbytes,
                                           stream) == 0
        untouched(dict(workspace=gwe, out=ge, skill_map=gk, spread_map=gp))
        got = dict(maps=dict(skill=gk.payload()[0].reshape(C, H, W), spread=gp.payload()[0].reshape(C, H, W)),
                   scores={k: ge.payload()[0][i] for i, k in enumerate(R.KEYS)})
        worst = max(worst, judge_group(got, ref, "maps", f"lead {l}"), judge_group(got, ref, "scores", f"lead {l} ensemble_scores"))
        for i, k in enumerate(R.KEYS):
            assert R.same_value_bits(got["scores"][k], roll[i, :, 1 + l]), (k, l)
        worst_o = max(worst_o, oracle_ratio(c["x"][:, :, l], t, cl, c["w"], sst, ref, ("maps", "scores")))
    note(f"guard bands {case} {layout}", worst, worst_o)


# ---- e. NaN / inf table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan_channel", [0, 1, 2, 3])
@pytest.mark.parametrize("M", [R.NAN_M, 1])
def test_nan_inf_table(E, M, nan_channel):
    """M = 1 beside M = 5: the reference's spread of one member is zeros, NaN member or not"""
    c = R.nan_table_case(M)
    x, t, cl, w = c["x"], c["t"], c["cl"], c["w"]
    xd, td, cd, wd = x.cuda(), t.cuda(), cl.cuda(), w.cuda()
    ref = R.scores_ref(x, t, cl, w, nan_channel)
    got = ensemble(E, xd, td, cd, wd, nan_channel)
    r = max(judge_group(got, ref, "maps", f"M={M}"), judge_group(got, ref, "scores", f"M={M} nan_channel {nan_channel}"))
    want = S.ensemble_scores(x.double(), t.double(), cl.double(), w.double(), sst_channel=nan_channel)  # the contract itself
    for k in R.KEYS:
        g = got["scores"][k].cpu().double()
        assert torch.equal(torch.isnan(g), torch.isnan(want[k])) and torch.equal(g[torch.isinf(want[k])], want[k][torch.isinf(want[k])]), k
    roll = E.rollout_scores(xd[:, :, None], td[:, None], cd[:, None], wd, nan_channel)
    for k in R.KEYS:
        assert R.same_value_bits(roll[k][:, 0], got["scores"][k]), k
    val = E.validation_scores(xd[:, :, None], td[:, None], wd)
    rv = judge_group({k: val[k][:, 0] for k in R.VKEYS}, ref, "validation", f"M={M} validation_scores")
    note(f"NaN / inf table M={M} nan_channel {nan_channel}", max(r, rv), oracle_ratio(x, t, cl, w, nan_channel, ref))
