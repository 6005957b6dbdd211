"""The energy score kernel (csrc/energy.hip: ldc_rollout_energy) through the C ABI and `rollout_energy`, against the float64 oracle and
the COUNTED bounds of tests/energy_refs.py (judged on the CPU by tests/test_energy_cpu.py):
  a. integer-valued cases (every fp32 value and every fp64 sum exact): bit for bit, dist2 included
  b. physical scale through the fused inverse normalisation, within the counted bounds; the same bits from de-normalised fields
  c. both layouts, two leads with permuted slots, l_off > 0 in a wider L_total; a column's bits alone, among other channels, with and
     without groups, with and without dist2; two runs
  d. the NaN / inf table
  e. groups: overlapping, a channel in no group, an SST-like channel with NaN points
  f. consistency with ldc_ensemble_scores' crps at one point and with ldc_rollout_reliability's n_invalid
  g. guard bands around every buffer; refused arguments launch nothing
  h. the driver: score_latent_rollout(..., energy=True, energy_groups=...) on the tiny synthetic DC-AE, and the command line"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import energy_refs as R
from tests.redzone import UNWRITTEN32, UNWRITTEN64, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.energy as en

    return en


def run_one(E, c, groups=(), scales=None, dist2=True, **over):
    """a single-lead case of energy_refs on the device -> dict(energy (5, C), n_invalid (C,), dist2 (C, N, N), energy_group (5, G))"""
    c = dict(c, **over)
    kw = {}
    if c["norm"] is not None:
        kw = dict(mean=c["norm"][0].cuda(), std=c["norm"][1].cuda(), target_std=c["norm"][2])
    if groups:
        kw.update(groups=[E.EnergyGroup(f"g{k}", tuple(g)) for k, g in enumerate(groups)], scales=scales)
    d = E.rollout_energy(c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), return_dist2=dist2, **kw)
    M, C = c["v"].shape[:2]
    assert d["energy_score"].dtype == torch.float64 and d["energy_score"].shape == (C, 1) and d["energy_n_invalid"].dtype == torch.int32
    out = dict(energy=torch.stack([d[k][:, 0] for k in E.ENERGY_NAMES]).cpu(), n_invalid=d["energy_n_invalid"][:, 0].cpu())
    if dist2:
        assert d["energy_dist2"].shape == (C, 1, M + 1, M + 1)
        out["dist2"] = d["energy_dist2"][:, 0].cpu()
    if groups:
        out["energy_group"] = torch.stack([d[k][:, 0] for k in E.ENERGY_GROUP_NAMES]).cpu()
    return out


def ref_of(c, groups=(), scales=None):
    return R.energy_ref(c["x"], c["t"], c["w"], groups, scales)


def same(a, b):
    """two results of run_one hold the same bits"""
    return a.keys() == b.keys() and all(R.same_bits(a[k], b[k]) for k in a)


# ---- a. integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W", R.INT_CASES)
def test_integers_are_exact(E, M, H, W):
    c = R.integer_case(M, H, W)
    groups, scales = ((0, 1), (1,)), torch.tensor([2.0, 0.5])  # powers of two: the group sums are exact too
    got, ref = run_one(E, c, groups, scales), ref_of(c, groups, scales)
    assert torch.equal(got["n_invalid"].long(), ref["n_invalid"]) and int(ref["n_invalid"].sum()) == 0
    d, want = got["dist2"], ref["dist2"][0]
    bad = (d != want).nonzero()
    assert bad.numel() == 0, f"M={M} {H}x{W}: dist2 differs at {bad[:4].tolist()}: {d[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
    assert torch.equal(d, d.transpose(1, 2)) and float(d.diagonal(dim1=1, dim2=2).abs().sum()) == 0.0
    assert R.exact(got, ref), f"M={M} {H}x{W}: {got['energy'].tolist()} vs {ref['energy'][0].tolist()}; groups {got['energy_group'].tolist()} vs {ref['energy_group'][0].tolist()}"
    if M == 1:
        assert R.same_bits(got["energy"][0], got["energy"][2]) and R.same_bits(got["energy"][1], got["energy"][2])  # es == es_fair == skill


# ---- b. physical scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M):
    c = R.physical_case(M)
    got, ref = run_one(E, c, R.PHYS_GROUPS, c["scales"]), ref_of(c, R.PHYS_GROUPS, c["scales"])
    r = R.check(got, ref, f"M={M}")
    print(f"physical M={M}: worst err / bound {r:.4f}")
    plain = run_one(E, c, R.PHYS_GROUPS, c["scales"], v=c["x"], norm=None)  # the same bits from fields de-normalised first
    assert same(plain, got)


# ---- c. layouts, slots, columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
def test_two_leads_slots_and_columns(E, layout):
    M, C, L, H, W, sst = R.GUARD_CASES[1]
    c = R.guard_case(*R.GUARD_CASES[1])
    xd = c["x"].cuda()
    groups, scales = [E.EnergyGroup("all", (0, 1))], torch.tensor([1.5, 0.75])
    kw = dict(truth_slot=c["t_slots"], groups=groups, scales=scales, return_dist2=True)
    assert c["t_slots"] != sorted(c["t_slots"])
    if layout == "frame_major":
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    d = E.rollout_energy(xd, c["truth_table"].cuda(), c["w"].cuda(), **kw)
    assert d["energy_score"].shape == (C, L) and d["energy_group_score"].shape == (1, L) and d["energy_dist2"].shape == (C, L, M + 1, M + 1)
    for l in range(L):
        ref = R.energy_ref(c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], [(0, 1)], scales)
        got = dict(energy=torch.stack([d[k][:, l] for k in E.ENERGY_NAMES]), n_invalid=d["energy_n_invalid"][:, l], dist2=d["energy_dist2"][:, l],
                   energy_group=torch.stack([d[k][:, l] for k in E.ENERGY_GROUP_NAMES]))
        r = R.check(got, ref, f"{layout} lead {l}")
        print(f"{layout} lead {l}: worst err / bound {r:.4f}")
        assert int(ref["n_invalid"][sst]) > 0 and int(ref["n_invalid"][1 - sst]) == 0  # the land points of the SST channel are counted
    out = E.empty_energy(M, C, 1, L + 2, "cuda", dist2=True)
    for b in out._buffers:
        b.fill_(7)
    d2 = E.rollout_energy(xd, c["truth_table"].cuda(), c["w"].cuda(), out=out, l_off=1, **kw)
    assert d2.keys() == d.keys()
    for k in d:
        assert R.same_bits(d2[k][:, 1 : 1 + L], d[k]), k
        assert bool((d2[k][:, 0] == 7).all()) and bool((d2[k][:, L + 1] == 7).all()), k


def test_a_columns_bits_do_not_depend_on_its_company(E):
    """general floats on a grid of more than one chunk: channel 1 of lead 1 alone, among three channels and two leads, with and without
    groups, with and without dist2, in the other layout"""
    g = R.gen(167)
    M, C, L, H, W = 7, 3, 2, 41, 103  # 4223 points: two chunks
    x = torch.randn(M, C, L, H, W, generator=g) * 3 + 1
    t = torch.randn(C, L, H, W, generator=g)
    x[2, 1, 1, 5, 7] = float("nan")
    w = R.cos_weights(H).cuda()
    xd, td = x.cuda(), t.cuda()
    full = E.rollout_energy(xd, td, w, groups=[E.EnergyGroup("a", (0, 1)), E.EnergyGroup("b", (1, 2))], scales=torch.tensor([1.0, 2.0, 3.0]),
                            return_dist2=True)
    alone = E.rollout_energy(xd[:, 1:2, 1:2].contiguous(), td[1:2, 1:2].contiguous(), w)
    bare = E.rollout_energy(xd, td, w)
    other = E.rollout_energy(xd.permute(2, 0, 1, 3, 4).contiguous(), td, w, lead_dim=0, return_dist2=True)
    wide = E.rollout_energy(xd[:, :, 1:2], td[:, 1:2], w, out=E.empty_energy(M, C, 0, 5, "cuda"), l_off=3)
    for k in E.ENERGY_NAMES + ("energy_n_invalid",):
        assert R.same_bits(alone[k][0, 0], full[k][1, 1]), k
        assert R.same_bits(bare[k], full[k]) and R.same_bits(other[k], full[k]) and R.same_bits(wide[k][:, 3], full[k][:, 1]), k
    assert R.same_bits(other["energy_dist2"], full["energy_dist2"]) and int(full["energy_n_invalid"][1, 1]) == 1
    again = E.rollout_energy(xd, td, w, groups=[E.EnergyGroup("b", (1, 2))], scales=torch.tensor([1.0, 2.0, 3.0]))
    for k in E.ENERGY_GROUP_NAMES:  # a group's bits do not depend on the other groups
        assert R.same_bits(again[k][0], full[k][1]), k


def test_two_runs_give_the_same_bits(E):
    for c, groups, scales in ((R.physical_case(50), R.PHYS_GROUPS, R.physical_case(50)["scales"]), (R.nan_table_case(), (), None),
                              (R.integer_case(88, 17, 241), (), None)):
        a, b = run_one(E, c, groups, scales), run_one(E, c, groups, scales)
        assert same(a, b)


# ---- d. NaN / inf ----------------------------------------------------------------------------------------------------------------------
def test_nan_inf_table(E):
    c = R.nan_table_case()
    got, ref = run_one(E, c), ref_of(c)
    R.check(got, ref, "nan table")
    H, W = R.NAN_HW
    assert got["n_invalid"].tolist() == [0, len(R.NAN_POINTS), len(R.NAN_POINTS), H * W, 0, 0]  # one member, the truth, all
    e, d = got["energy"], got["dist2"]
    assert bool(torch.isfinite(e[:, :3]).all()) and bool(torch.isfinite(d[:3]).all())
    assert R.same_bits(e[:, 1], e[:, 2]) and R.same_bits(d[1], d[2])  # the same points left out, whoever held the NaN
    assert bool(torch.isnan(e[:4, 3]).all()) and float(e[4, 3]) == 0.0 and float(d[3].abs().sum()) == 0.0  # no valid point
    clean = run_one(E, R.nan_table_case(poison=False))
    inf = float("inf")
    # +inf in member 1: its row and column are +inf, the other entries the bits of the clean field
    keep = torch.ones(R.NAN_M + 1, R.NAN_M + 1, dtype=torch.bool)
    keep[1, :], keep[:, 1] = False, False
    assert bool((d[4][~keep & ~torch.eye(R.NAN_M + 1, dtype=torch.bool)] == inf).all()) and R.same_bits(d[4][keep], clean["dist2"][4][keep])
    assert float(e[2, 4]) == inf and bool(torch.isnan(e[0, 4]))  # the skill is +inf, the score inf - inf
    # +inf in members 1 and 3 at one point: entry (1, 3) is inf - inf = NaN, the rest of their rows +inf, the others untouched
    keep[3, :], keep[:, 3] = False, False
    assert bool(torch.isnan(d[5][1, 3])) and bool(torch.isnan(d[5][3, 1])) and float(d[5][1, 0]) == inf and float(d[5][3, R.NAN_M]) == inf
    assert R.same_bits(d[5][keep], clean["dist2"][5][keep]) and float(d[5].diagonal().abs().sum()) == 0.0
    assert float(e[2, 5]) == inf and bool(torch.isnan(e[[0, 1, 3], 5]).all())
    assert R.same_bits(e[4, 5], clean["energy"][4, 5])  # every point is valid: the weight is whole


# ---- e. groups ---------------------------------------------------------------------------------------------------------------------------
def test_groups(E):
    c = R.group_case()
    got, ref = run_one(E, c, c["groups"], c["scales"]), ref_of(c, c["groups"], c["scales"])
    r = R.check(got, ref, "groups")
    print(f"groups: worst err / bound {r:.4f}")
    wv, n_land = got["energy"][4], int(c["land"].sum())
    assert got["n_invalid"].tolist() == [0, 0, 0, n_land, 0] and float(wv[R.GROUP_SST]) < float(wv[0])
    for k, chans in enumerate(c["groups"]):  # Wv_g = sum of Wv_c, in ascending channel order
        s = 0.0
        for ch in sorted(chans):
            s = s + float(wv[ch])
        assert float(got["energy_group"][4, k]) == s, k
    alone = run_one(E, c, (c["groups"][1],), c["scales"])  # a group's bits do not depend on the other groups
    assert R.same_bits(alone["energy_group"][:, 0], got["energy_group"][:, 1]) and R.same_bits(alone["energy"], got["energy"])
    none = run_one(E, c)
    assert "energy_group" not in none and R.same_bits(none["energy"], got["energy"]) and R.same_bits(none["dist2"], got["dist2"])


# ---- f. consistency with the shipped kernels -------------------------------------------------------------------------------------------
def test_one_point_agrees_with_ensemble_scores_crps(E):
    """H x W = 1: es_fair is the point's CRPS.  ldc_ensemble_scores forms it in fp32 (bound: score_edge_refs.point_ref's crps; the weight 1
    and the mean over one point are exact), this kernel within the counted bound of es_fair; the two float64 formulas themselves agree to
    float64 rounding (1e-12 relative to the skill covers it)."""
    from ladcast_amd.evaluate import ensemble_scores
    from tests.score_edge_refs import point_ref

    M, C = 20, 4
    g = R.gen(173)
    x, t = torch.randn(M, C, 1, 1, generator=g) * 3 + 1, torch.randn(C, 1, 1, generator=g)
    w = torch.ones(1)
    d = E.rollout_energy(x.cuda()[:, :, None], t.cuda()[:, None], w.cuda())
    crps = ensemble_scores(x.cuda(), t.cuda(), None, w.cuda(), -1)["crps"].cpu().double()
    ref = R.energy_ref(x, t, w)
    val, b_crps = point_ref(x.reshape(M, C), t.reshape(C))["crps"]
    fair, b_fair = ref["energy"][0][1], ref["energy"][1][1]
    err = (d["energy_score_fair"][:, 0].cpu() - crps).abs()
    bound = b_fair + b_crps + 1e-12 * ref["energy"][0][2].abs()
    print(f"one point: worst err / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    assert bool(((fair - val).abs() <= 1e-12 * ref["energy"][0][2].abs()).all())


def test_n_invalid_equals_rollout_reliability(E):
    from ladcast_amd.evaluate import rollout_reliability

    M, C, L, H, W, sst = R.GUARD_CASES[1]
    c = R.guard_case(*R.GUARD_CASES[1])
    x = c["x"].clone()
    x[3, 1, 1, 7, 5] = float("nan")  # one more, in the channel without land
    args = (x.cuda(), c["truth_table"].cuda(), c["w"].cuda())
    d = E.rollout_energy(*args, truth_slot=c["t_slots"])
    rel = rollout_reliability(*args, sst, truth_slot=c["t_slots"])
    assert torch.equal(d["energy_n_invalid"], rel["n_invalid"]) and int(d["energy_n_invalid"][1, 1]) == 1 and int(d["energy_n_invalid"][sst].min()) > 0


# ---- g. guard bands, arguments ---------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    t = t.detach().cpu().contiguous()
    return bool((t.view(torch.int64) == UNWRITTEN64).all()) if t.dtype == torch.float64 else bool((t.view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", R.GUARD_CASES)
def test_guard_bands(case, layout):
    from ladcast_amd import hip
    from ladcast_amd.evaluate.energy import EnergyGroup, group_words

    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    groups = [tuple(range(C)), (C - 1,), (0,)]
    G, N = len(groups), M + 1
    HW, ld, FMAX = H * W, H * W + 8, R.FLT_MAX_BITS
    inp = dict(poison=FMAX, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(c["x"].reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(c["x"].permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gt = guarded(C, HW, ld, batch=R.N_TRUTH, batch_stride=C * ld + 16, **inp).fill(c["truth_table"].reshape(R.N_TRUTH, C, HW))
    gl = guarded(1, H, **inp).fill(c["w"])
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    scales = torch.linspace(0.5, 2.0, C)
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    ggm = guarded(1, C, dtype=torch.int32, poison=0x7FFFFFFF, unwritten=False).fill(group_words([EnergyGroup(str(k), g) for k, g in enumerate(groups)], C))
    gis = guarded(1, C, dtype=torch.float64, poison=0x7FEFFFFFFFFFFFFF, unwritten=False).fill(R.inv_scale2(scales))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    nbytes = int(hip.lib.ldc_rollout_energy_workspace_bytes(M, C, G, L, H, W))
    assert nbytes == R.workspace_bytes(M, C, L, HW) and nbytes % 8 == 0
    gw = guarded(1, nbytes // 4, unwritten=False)
    gen_, geg = guarded(5 * C, Lt, dtype=torch.float64), guarded(5 * G, Lt, dtype=torch.float64)
    gni, gd2 = guarded(C, Lt, dtype=torch.int32), guarded(C * Lt, N * N, dtype=torch.float64)
    assert hip.lib.ldc_rollout_energy(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gl.view),
                                      _p(ggm.view), _p(gis.view), G, M, C, L, H, W, _p(gen_.view), _p(geg.view), _p(gni.view), _p(gd2.view), Lt, 1,
                                      _p(gw.view), nbytes, stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, lat_weight=gl, truth_slot=gts, mean=gm, std=gs, group_mask=ggm, inv_scale2=gis, workspace=gw,
                     energy=gen_, energy_group=geg, n_invalid=gni, dist2=gd2).items():
        assert_untouched(g, k)
    en, eg = gen_.payload()[0].reshape(5, C, Lt), geg.payload()[0].reshape(5, G, Lt)
    ni, d2 = gni.payload()[0].reshape(C, Lt), gd2.payload()[0].reshape(C, Lt, N, N)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(en[:, :, col]) and _unwritten(eg[:, :, col]) and _unwritten(ni[:, col]) and _unwritten(d2[:, col])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    for l in range(L):
        ref = R.energy_ref(xp[:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], groups, scales)
        r = R.check(dict(energy=en[:, :, 1 + l], n_invalid=ni[:, 1 + l], dist2=d2[:, 1 + l], energy_group=eg[:, :, 1 + l]), ref, f"{case} {layout} lead {l}")
        print(f"guard bands {case} {layout} lead {l}: worst err / bound {r:.4f}")
        assert bool(torch.isfinite(en[:, :, 1 + l]).all()) and int(ref["n_invalid"][sst]) > 0  # the land points of the SST channel


def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M0, C, L0, H0, W0, G0 = 5, 2, 1, 4, 8, 2
    x, t = torch.zeros(M0, C, L0, H0, W0, device="cuda"), torch.zeros(C, L0, H0, W0, device="cuda")
    w, slot = torch.ones(H0, device="cuda"), torch.zeros(L0, dtype=torch.int32, device="cuda")
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    gmask, inv = torch.full((C,), 3, dtype=torch.int32, device="cuda"), torch.ones(C, dtype=torch.float64, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)
    NOPE = object()

    def call(M=M0, L=L0, H=H0, W=W0, Cn=C, G=G0, L_total=L0, l_off=0, nbytes=1 << 18, forecast=x, mean=None, std=None, mask=gmask, scale=inv,
             group_out=NOPE, dist=True, ws_off=0, en_off=0, eg_off=0, d2_off=0):
        ge, gg = guarded(5 * C, L0, dtype=torch.float64), guarded(5 * G0, L0, dtype=torch.float64)
        gn, gd = guarded(C, L0, dtype=torch.int32), guarded(C * L0, (M0 + 1) ** 2, dtype=torch.float64)
        eg = ctypes.c_void_p(gg.view.data_ptr() + eg_off) if group_out is NOPE else group_out
        st = hip.lib.ldc_rollout_energy(None if forecast is None else _p(forecast), x.stride(0), x.stride(2), x.stride(1), None if mean is None else _p(mean),
                                        None if std is None else _p(std), 1.0, _p(t), t.stride(1), t.stride(0), _p(slot), _p(w),
                                        None if mask is None else _p(mask), None if scale is None else _p(scale), G, M, Cn, L, H, W,
                                        ctypes.c_void_p(ge.view.data_ptr() + en_off), eg, _p(gn.view),
                                        ctypes.c_void_p(gd.view.data_ptr() + d2_off) if dist else None, L_total, l_off,
                                        ctypes.c_void_p(gw.view.data_ptr() + ws_off), nbytes, stream)
        torch.cuda.synchronize()
        untouched = all(_unwritten(g.payload()) for g in (ge, gg, gn, gd))
        for g in (ge, gg, gn, gd, gw):
            assert_untouched(g)
        return st, untouched

    ARG, UNSUPPORTED, ALIGN = (-1, True), (-3, True), (-2, True)
    need = int(hip.lib.ldc_rollout_energy_workspace_bytes(M0, C, G0, L0, H0, W0))
    assert need == R.workspace_bytes(M0, C, L0, H0 * W0)
    assert call(forecast=None) == ARG
    for kw in (dict(M=0), dict(M=-3), dict(Cn=0), dict(L=0), dict(H=0), dict(W=0), dict(G=-1), dict(L_total=0), dict(l_off=-1), dict(mean=mean),
               dict(mask=None), dict(scale=None), dict(group_out=None), dict(G=0)):  # G == 0 with an energy_group; G > 0 without one
        assert call(**kw) == ARG, kw
    assert call(L_total=1, l_off=1) == ARG and call(L_total=3, l_off=3) == ARG  # l_off + L > L_total
    assert call(nbytes=need - 8) == ARG  # a short workspace
    assert call(M=257, nbytes=1 << 40) == UNSUPPORTED and call(G=33) == UNSUPPORTED
    assert call(L=65536, L_total=65536, nbytes=1 << 40) == UNSUPPORTED and call(Cn=65536, nbytes=1 << 40) == UNSUPPORTED
    assert call(H=4097, W=4096, nbytes=1 << 40) == UNSUPPORTED
    for kw in (dict(ws_off=4), dict(en_off=4), dict(eg_off=4), dict(d2_off=4)):  # fp64: every such pointer must be 8-byte aligned
        assert call(**kw) == ALIGN, kw
    # and the calls that are served
    assert call(nbytes=need) == (0, False)
    assert call(mean=mean, std=std, dist=False)[0] == 0
    assert call(G=0, group_out=None, mask=None, scale=None)[0] == 0
    # the wrappers
    with pytest.raises(ValueError):
        E.rollout_energy(torch.zeros(257, 1, 1, 2, 4, device="cuda"), torch.zeros(1, 1, 2, 4, device="cuda"), torch.ones(2, device="cuda"))
    with pytest.raises(RuntimeError):
        E.rollout_energy(x.cpu(), t, w)  # device tensors only
    out = E.empty_energy(M0, C, 0, L0, "cuda")
    with pytest.raises(RuntimeError, match="ldc_rollout_energy"):
        hip.rollout_energy(x, t, slot, w, out._buffers[0], out._buffers[1], M=257, C=C, L=L0, H=H0, W=W0, member_stride=x.stride(0),
                           lead_stride=x.stride(2), channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0), L_total=L0)


# ---- h. the driver ---------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double()), torch.nan_to_num(b.double())) \
        and torch.equal(torch.isnan(a.double()), torch.isnan(b.double()))


def test_driver_energy():
    """The decoder is not batch-invariant (tests/test_gpu_regional.py: a frame decoded among 6 differs from the same frame decoded among 3
    by up to 1.3e-6), so across decode batch sizes the driver owes this: under each batching the result is the bits of a direct call on
    the frames as that batching decodes them, and two batchings that decode the same batches (decode_batch_frames = ENS and 2 ENS - 1:
    one lead time per call, as the default) give equal bits.  A batching that decodes other batches agrees as closely as its frames do:
    1e-4 of the skill, a hundred times the relative difference of the decoded values."""
    from ladcast_amd.evaluate import EnergyGroup, rollout_energy
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.evaluate_encdec_model import equiangular_lat_weights
    from ladcast_amd.models import AutoencoderDC
    from tests.synth import make_dcae, tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 3, 8, 3, 6, 8, 8, 48, 64, 3
    cfg = tiny_dcae_config()
    model = AutoencoderDC.from_config(cfg)
    model.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(179)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    latents = torch.randn(ENS, C_LAT, 1 + T, h, w_, generator=gen)
    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = torch.randn(6, C, H, W, generator=gen) * scale + shift
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    clim = torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift
    t_slots, c_slots = [2, 5, 3], [2, 1, 4]
    lat_w = equiangular_lat_weights(H + 1, True)
    groups = [EnergyGroup("upper", (0, 1, 2)), EnergyGroup("with_sst", (2, SST, 7))]
    args = (latents, model, mean, std, truth.cuda(), t_slots, clim.cuda(), c_slots, lat_w)
    kw = dict(sst_channel=SST, crop_init=True)
    plain = EG.score_latent_rollout(*args, **kw)
    got = EG.score_latent_rollout(*args, energy=True, energy_groups=groups, **kw)
    keys = EG.ENERGY_KEYS + EG.ENERGY_GROUP_NAMES
    assert set(got) == set(plain) | set(keys)
    for k in SCORES:  # the five scores are the bits of a call without the energy score
        assert _same(got[k], plain[k]), k
    for k in EG.ENERGY_KEYS:
        assert got[k].shape == (C, T) and got[k].device.type == "cpu" and got[k].dtype == (torch.int32 if k == "energy_n_invalid" else torch.float64), k
    for k in EG.ENERGY_GROUP_NAMES:
        assert got[k].shape == (2, T) and got[k].dtype == torch.float64 and bool(torch.isfinite(got[k]).all()), k
    assert int(got["energy_n_invalid"][SST].min()) > 0 and int(got["energy_n_invalid"][0].max()) == 0  # land: the SST channel only
    assert bool(torch.isfinite(got["energy_score"]).all()) and bool((got["energy_skill"] > 0).all())
    only = EG.score_latent_rollout(*args, energy=True, **kw)  # without groups: the channel scores are the same bits
    assert set(only) == set(plain) | set(EG.ENERGY_KEYS) and all(_same(only[k], got[k]) for k in EG.ENERGY_KEYS)
    # a direct call on the fields decoded in one go per lead time, as the driver decodes them; the default scales are std
    frames = torch.stack([model.decode(latents[:, :, 1 + l].contiguous().cuda()).sample for l in range(T)])  # (T, ens, C, H, W), normalised
    direct = rollout_energy(frames, truth.cuda(), lat_w.cuda(), groups=groups, scales=std, truth_slot=t_slots, lead_dim=0, mean=mean.cuda(), std=std.cuda())
    for k in keys:
        assert R.same_bits(got[k], direct[k].cpu()), k
    for dbf in (ENS, 2 * ENS - 1):  # the same decode batches: the same bits
        again = EG.score_latent_rollout(*args, energy=True, energy_groups=groups, decode_batch_frames=dbf, **kw)
        assert all(_same(again[k], got[k]) for k in keys), dbf
    other = EG.score_latent_rollout(*args, energy=True, energy_groups=groups, decode_batch_frames=2 * ENS, **kw)  # two lead times per call
    lat = latents[:, :, 1:]
    chunks = [model.decode(lat[:, :, s0 : s0 + 2].permute(2, 0, 1, 3, 4).reshape(-1, C_LAT, h, w_).contiguous().cuda()).sample for s0 in (0, 2)]
    frames2 = torch.cat(chunks).reshape(T, ENS, C, H, W)
    direct2 = rollout_energy(frames2, truth.cuda(), lat_w.cuda(), groups=groups, scales=std, truth_slot=t_slots, lead_dim=0, mean=mean.cuda(), std=std.cuda())
    for k in keys:
        assert R.same_bits(other[k], direct2[k].cpu()), k
    assert torch.equal(other["energy_n_invalid"], got["energy_n_invalid"])
    for pre in ("energy_", "energy_group_"):
        for k in ("score", "score_fair", "skill", "spread"):
            assert bool(((other[pre + k] - got[pre + k]).abs() <= 1e-4 * got[pre + "skill"]).all()), pre + k
    wide = EG.score_latent_rollout(*args, energy=True, energy_groups=groups, total_num_steps=T + 2, **kw)
    for k in keys:
        assert _same(wide[k][:, :T].contiguous(), got[k]), k
        assert bool(torch.isnan(wide[k][:, T:].double()).all()) if k != "energy_n_invalid" else int(wide[k][:, T:].abs().sum()) == 0, k
    scaled = EG.score_latent_rollout(*args, energy_groups=groups, energy_scales=2 * std, **kw)  # groups imply energy; scales of one's own
    assert np.allclose(scaled["energy_group_score"].numpy(), got["energy_group_score"].numpy() / 2, rtol=1e-12)


def test_command_line_energy_flags(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.pipelines.io import save_latent_npy
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]
    gen = torch.Generator().manual_seed(181)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    lv = (300, 500, 850)
    norm = {"geopotential": {"mean": {str(p): float(mean[i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {str(p): float(mean[3 + i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(mean[6]), "std": float(std[6])}, "sea_surface_temperature": {"mean": float(mean[7]), "std": float(std[7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    latents = torch.randn(2, ENS, C_LAT, 1 + T, h, w_, generator=gen)
    save_latent_npy(latents, inits, str(tmp_path / "rollout"))
    truth = torch.randn(11, C, H + 1, W, generator=gen) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)  # with the south pole row
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H + 1, W))  # sparse: zeros
    clim.flush()
    del clim
    flags = ["--energy_group", "z_t", "geopotential_level500", "temperature_level850", "--energy_group", "surface", "6", "sea_surface_temperature", "1"]

    def run(extra, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", *map(str, lv), "--num_atm_vars", "2"] + extra
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, en = run([], "plain"), run(flags, "energy")
    per_channel = ["energy_score.npy", "energy_score_fair.npy", "energy_skill.npy", "energy_spread.npy", "energy_n_invalid.npy"]
    per_group = ["energy_group_score.npy", "energy_group_score_fair.npy", "energy_group_skill.npy", "energy_group_spread.npy"]
    assert sorted(p.name for p in en.iterdir()) == sorted([p.name for p in plain.iterdir()] + per_channel + per_group + ["energy.json"])
    for p in plain.iterdir():  # every other file bit for bit
        assert (en / p.name).read_bytes() == p.read_bytes(), p.name
    for k in per_channel:
        a = np.load(en / k)
        assert a.shape == (2, C, T) and a.dtype == (np.int32 if k == "energy_n_invalid.npy" else np.float64), k
    for k in per_group:
        a = np.load(en / k)
        assert a.shape == (2, 2, T) and a.dtype == np.float64 and np.isfinite(a).all(), k
    es, fair, skill, spread = (np.load(en / k) for k in per_channel[:4])
    assert np.isfinite(es).all() and (np.load(en / "energy_n_invalid.npy") == 0).all()
    assert np.array_equal(es, skill - 0.5 * spread) and (fair <= es).all() and (skill > 0).all() and (spread > 0).all()
    meta = json.loads((en / "energy.json").read_text())
    assert [(m["name"], m["channels"]) for m in meta["groups"]] == [("z_t", [1, 5]), ("surface", [6, 7, 1])]
    assert meta["groups"][0]["channel_names"] == ["geopotential_level500", "temperature_level850"]
    assert np.allclose(meta["groups"][1]["scales"], [float(std[6]), float(std[7]), float(std[1])], rtol=1e-6)
