"""The regional score kernel (csrc/regional.hip: ldc_rollout_regional) through the C ABI and `rollout_regional`, against the float64
oracle and the COUNTED bounds of tests/regional_refs.py (judged on the CPU by tests/test_regional_cpu.py):
  a. integer-valued cases (every fp32 point value and fp64 sum exact): 8 ensemble sizes x 3 grids x 3 region sets, bit for bit
  b. physical scale through the fused inverse normalisation, within the counted bounds
  c. both layouts, two leads with permuted slots, l_off > 0 in a wider L_total
  d. the NaN / inf table; poison at the points of no region
  e. independence of the other regions; two runs give the same bits
  f. consistency with ldc_ensemble_scores' point maps, ldc_rollout_scores and ldc_rollout_reliability
  g. guard bands around every buffer; refused arguments launch nothing
  h. the driver: score_latent_rollout(..., regions=...) on the tiny synthetic DC-AE, and the command line"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import regional_refs as R
from tests.redzone import U, UNWRITTEN32, UNWRITTEN64, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.regional as er

    return er


def run_one(E, c, **over):
    """a single-lead case of regional_refs on the device -> dict(sums (R, C, 10), counts (R, C, 3)) on the host"""
    c = dict(c, **over)
    kw = {}
    if c["norm"] is not None:
        kw = dict(mean=c["norm"][0].cuda(), std=c["norm"][1].cuda(), target_std=c["norm"][2])
    cl = None if c["cl"] is None else c["cl"].cuda()[:, None]
    d = E.rollout_regional(c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), np.asarray(c["mask"]), c["R"], clim=cl, **kw)
    C = c["v"].shape[1]
    assert d["regional_sums"].dtype == torch.float64 and d["regional_counts"].dtype == torch.int32
    assert d["regional_sums"].shape == (c["R"], C, 1, 10) and d["regional_counts"].shape == (c["R"], C, 1, 3)
    return dict(sums=d["regional_sums"][:, :, 0].cpu(), counts=d["regional_counts"][:, :, 0].cpu())


def ref_of(c):
    return R.regional_ref(c["x"], c["t"], c["w"], c["mask"], c["R"], c["cl"])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.contiguous().view(torch.int64) if b.dtype == torch.float64 else b)


# ---- a. integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W,Rn", R.INT_CASES)
def test_integers_are_exact(E, M, H, W, Rn):
    c = R.integer_case(M, H, W, Rn)
    got, ref = run_one(E, c), ref_of(c)
    assert torch.equal(got["counts"].long(), ref["counts"]), (got["counts"].long() != ref["counts"]).nonzero()[:4].tolist()
    bad = (got["sums"] != ref["sums"][0]).nonzero()
    assert bad.numel() == 0, f"M={M} {H}x{W} R={Rn}: sums differ at {bad[:4].tolist()}: {got['sums'][tuple(bad[0])]} vs {ref['sums'][0][tuple(bad[0])]}"
    assert int(ref["counts"][:, :, 1].sum()) == 0 and int(ref["counts"][0, 0, 0]) > 0
    if c["cl"] is not None:
        assert torch.equal(got["sums"][..., 6], got["sums"][..., 0])  # no NaN climatology: the ACC weight is the weight


def test_without_climatology_the_acc_sums_are_zero(E):
    c = R.integer_case(9, 5, 103, 32)
    got, ref = run_one(E, c, cl=None), R.regional_ref(c["x"], c["t"], c["w"], c["mask"], c["R"], None)
    assert R.exact(got, ref) and int(got["sums"][..., 6:].abs().sum()) == 0 and int(got["counts"][..., 2].sum()) == 0


# ---- b. physical scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M):
    c = R.physical_case(M)
    got, ref = run_one(E, c), ref_of(c)
    r = R.check(got, ref, f"M={M}")
    print(f"physical M={M}: worst err / bound {r:.4f}")
    plain = run_one(E, c, v=c["x"], norm=None)  # the same bits from fields de-normalised first
    assert same_bits(plain["sums"], got["sums"]) and torch.equal(plain["counts"], got["counts"])


# ---- c. layouts, slots, columns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
def test_two_leads_slots_and_columns(E, layout):
    M, C, L, H, W, _ = R.GUARD_CASES[1]
    c = R.guard_case(*R.GUARD_CASES[1])
    Rn = 32
    mask = R.case_mask(H, W, Rn, 101)
    xd = c["x"].cuda()
    kw = dict(clim=c["clim_table"].cuda(), clim_slots=c["c_slots"], truth_slot=c["t_slots"])
    assert c["t_slots"] != sorted(c["t_slots"]) and c["c_slots"] != c["t_slots"]
    if layout == "frame_major":
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    d = E.rollout_regional(xd, c["truth_table"].cuda(), c["w"].cuda(), mask.numpy(), Rn, **kw)
    assert d["regional_sums"].shape == (Rn, C, L, 10)
    for l in range(L):
        ref = R.regional_ref(c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], mask, Rn, c["clim_table"][c["c_slots"][l]])
        r = R.check(dict(sums=d["regional_sums"][:, :, l], counts=d["regional_counts"][:, :, l]), ref, f"{layout} lead {l}")
        print(f"{layout} lead {l}: worst err / bound {r:.4f}")
        assert int(ref["counts"][:, 0, 1].sum()) > 0  # the land points of the SST channel are counted as invalid
    out = E.empty_regional(Rn, C, L + 2, "cuda")
    for b in out._buffers:
        b.fill_(7)
    d2 = E.rollout_regional(xd, c["truth_table"].cuda(), c["w"].cuda(), mask.numpy(), Rn, out=out, l_off=1, **kw)
    for k in d:
        assert same_bits(d2[k][:, :, 1 : 1 + L].contiguous(), d[k].contiguous()), k
        assert bool((d2[k][:, :, 0] == 7).all()) and bool((d2[k][:, :, L + 1] == 7).all()), k


# ---- d. NaN / inf ----------------------------------------------------------------------------------------------------------------------
def test_nan_inf_table(E):
    c = R.nan_table_case()
    got, ref = run_one(E, c), ref_of(c)
    R.check(got, ref, "nan table")
    bits, kind = R.region_bits(c["mask"], c["R"]), c["kind"]
    for r in range(c["R"]):
        n = [int((bits[r] & (kind == k)).sum()) for k in range(len(R.PATTERNS))]
        assert got["counts"][r, 0].tolist() == [n[0] + n[3] + n[4], n[1] + n[2], n[0] + n[4]]  # NaN climatology only: valid, not ACC-valid
    assert bool(torch.isinf(got["sums"][..., 1]).all()) and bool(torch.isnan(got["sums"][..., 3]).all())  # +inf is a value: IEEE sums
    # NaN and inf at the points of no region - a whole tile among them - have no effect on any output
    clean = run_one(E, R.nan_table_case(poison=False))
    assert same_bits(clean["sums"], got["sums"]) and torch.equal(clean["counts"], got["counts"])


def test_inf_is_an_ordered_value(E):
    inf = float("inf")
    x = torch.tensor([[inf, 0.0, -inf], [1.0, 2.0, -inf], [0.0, 4.0, -inf]]).reshape(3, 1, 1, 1, 3).cuda()
    t = torch.tensor([0.0, inf, 0.0]).reshape(1, 1, 1, 3).cuda()
    d = E.rollout_regional(x, t, torch.ones(1).cuda(), np.array([[1, 2, 4]], dtype=np.uint32), 3)
    s, n = d["regional_sums"][:, 0, 0].cpu(), d["regional_counts"][:, 0, 0].cpu()
    assert n.tolist() == [[1, 0, 0]] * 3
    assert s[0, :6].tolist()[:3] == [1.0, inf, inf] and torch.isnan(s[0, 3]) and s[0, 4] == inf and s[0, 5] == inf  # a member +inf
    assert s[1, 1] == -inf and s[1, 2] == inf and s[1, 3] == 4.0 and s[1, 4] == inf and abs(float(s[1, 5]) - 2 / 6 * (-2 * 0 + 2 * 4)) < 1e-6  # truth +inf
    assert s[2, 1] == -inf and torch.isnan(s[2, 3]) and s[2, 4] == inf and torch.isnan(s[2, 5])  # all members -inf: inf - inf in the spread


# ---- e. independence, repeatability ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["physical", "two records"])
def test_one_region_alone_gives_the_bits_it_gives_among_31_others(E, case):
    c = R.physical_case(50) if case == "physical" else R.integer_case(9, 9, 257, 32)
    if case == "two records":  # general floats on the ten-tile grid: the grouping of the additions into records must not depend on R
        g = R.gen(103)
        x = torch.randn(*c["x"].shape, generator=g) * 3
        c = dict(c, v=x, x=x, t=torch.randn(*c["t"].shape, generator=g), cl=torch.randn(*c["cl"].shape, generator=g))
    full = run_one(E, c)
    m = torch.as_tensor(np.asarray(c["mask"]).astype(np.int64))
    alone = run_one(E, c, mask=((m >> 17) & 1).numpy(), R=1)
    assert int(alone["counts"][0, 0, 0]) > 50
    assert same_bits(alone["sums"][0], full["sums"][17]) and torch.equal(alone["counts"][0], full["counts"][17])
    few = run_one(E, c, mask=(m & 0x3FFFF).numpy(), R=18)  # and as the last of 18
    assert same_bits(few["sums"], full["sums"][:18]) and torch.equal(few["counts"], full["counts"][:18])


def test_two_runs_give_the_same_bits(E):
    for c in (R.physical_case(64), R.nan_table_case(), R.integer_case(9, 9, 257, 32)):
        a, b = run_one(E, c), run_one(E, c)
        assert same_bits(a["sums"], b["sums"]) and torch.equal(a["counts"], b["counts"])


# ---- f. consistency with the shipped kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [8, 24, 50])
def test_single_point_regions_hold_the_point_maps_of_ensemble_scores(E, M):
    """lat_weight all 1 and 32 single-point regions: S4 and S5 are one term each, the point's skill and spread - the values of
    ldc_ensemble_scores' skill_map / spread_map, on general floats.  S4 (sums, one division) is held bit for bit at every M.  S5 is held
    bit for bit where scoring.hip's contracted build fuses every multiply-add of the spread as regional.hip does explicitly (M > 8); its
    8-member arm leaves the first two products unfused (a packed multiply), so there S5 is held to the counted spread bound of
    tests/regional_refs.py against it instead.  S2 is the fp32 square of (mean - t), formed here from the same fp32 operations."""
    from ladcast_amd import hip

    H, W, C = 5, 103, 2
    g = R.gen(107 + M)
    x = (torch.randn(M, C, H, W, generator=g) * 3 + 1).cuda()
    t = torch.randn(C, H, W, generator=g).cuda()
    w = torch.ones(H).cuda()
    pts = torch.randperm(H * W, generator=g)[:32]
    mask = torch.zeros(H * W, dtype=torch.int64)
    mask[pts] = 1 << torch.arange(32)
    d = E.rollout_regional(x[:, :, None], t[:, None], w, mask.reshape(H, W).numpy(), 32)
    s = d["regional_sums"][:, :, 0].cpu()
    out, skill_map, spread_map = torch.empty(5, C, device="cuda"), torch.empty(C, H, W, device="cuda"), torch.empty(C, H, W, device="cuda")
    hip.ensemble_scores(x, t, None, w, out, M=M, C=C, H=H, W=W, member_stride=x.stride(0), channel_stride=x.stride(1), truth_channel_stride=t.stride(0),
                        skill_map=skill_map, spread_map=spread_map)
    sk, sp = skill_map.reshape(C, -1)[:, pts].T.cpu().double(), spread_map.reshape(C, -1)[:, pts].T.cpu().double()
    assert torch.equal(s[..., 0], torch.ones(32, C, dtype=torch.float64)) and torch.equal(d["regional_counts"][:, :, 0, 0].cpu(), torch.ones(32, C, dtype=torch.int32))
    assert torch.equal(s[..., 4], sk)
    if M > 8:
        assert torch.equal(s[..., 5], sp)
    else:
        xs = torch.sort(x.cpu().double().reshape(M, C, -1)[:, :, pts], dim=0).values
        wt = (2.0 * torch.arange(1, M + 1, dtype=torch.float64) - M - 1).view(-1, 1, 1)
        bound = 2 * (M + 1) * U * 2.0 / (M * (M - 1)) * (xs.abs() * wt.abs()).sum(0).T  # two fp32 evaluations, each within the counted bound
        assert bool(((s[..., 5] - sp).abs() <= bound).all()), float(((s[..., 5] - sp).abs() / bound).max())
    mean = torch.zeros(C, H * W)
    for i in range(M):
        mean = mean + x[i].cpu().reshape(C, -1)
    mean = mean / torch.tensor(float(M))
    e = (mean - t.cpu().reshape(C, -1))[:, pts].T
    assert torch.equal(s[..., 2], (e * e).double()) and torch.equal(s[..., 1], e.double())


@pytest.mark.parametrize("M", [8, 50])
def test_global_region_agrees_with_rollout_scores_and_reliability(E, M):
    """S2 / (H W), S4 / (H W), S5 / (H W) against ldc_rollout_scores' ens_mse, crps_skill, crps_spread and S3 / (H W) against
    ldc_rollout_reliability's ens_var.  The point values are the same fp32 numbers (the spread up to its fused multiply-adds: the counted
    (M + 1) U bound of regional_refs, twice); those kernels then round w * v to fp32 (1) and reduce in fp32: butterfly (6), the four wave
    totals pairwise (2), records per lane ceil(nblk / 64) (here 1), a second butterfly (6), the division by the count (1): 17 U on
    sum |w v| / (H W).  The fp64 sums of this kernel add (P + nrec) 2^-53, far below."""
    from ladcast_amd.evaluate import rollout_reliability, rollout_scores

    c = R.physical_case(M)
    H, W = R.PHYS_HW
    P = H * W
    xd, td, cd, wd = c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["cl"].cuda()[:, None], c["w"].cuda()
    kw = dict(mean=c["norm"][0].cuda(), std=c["norm"][1].cuda(), target_std=c["norm"][2])
    d = E.rollout_regional(xd, td, wd, np.ones((H, W), dtype=np.uint32), 1, clim=cd, **kw)
    s = d["regional_sums"][0, :, 0].cpu()
    sc = rollout_scores(xd, td, cd, wd, -1, **kw)
    rel = rollout_reliability(xd, td, wd, -1, **kw)
    pv, _, _ = R.point_values(c["x"], c["t"], c["cl"])
    wp = c["w"].double().reshape(H, 1).expand(H, W).reshape(P)
    n_tree = 1 + 6 + 2 + -(-(-(-P // 256)) // 64) + 6 + 1
    for k, name, other in ((2, "se", sc["ens_mse"]), (4, "skill", sc["crps_skill"]), (5, "spread", sc["crps_spread"]), (3, "var", rel["ens_var"])):
        v, b = pv[name]
        extra = 2 * (wp * b).sum(-1) / P if name == "spread" else 0.0
        bound = n_tree * U * (wp * v.abs()).sum(-1) / P + (P + 1) * 2.0 ** -53 * (wp * v.abs()).sum(-1) / P + extra
        err = (s[:, k] / P - other[:, 0].cpu().double()).abs()
        print(f"M={M} {name}: worst err / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), (name, err.tolist(), bound.tolist())


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

    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    Rn = 5
    mask = R.case_mask(H, W, 32, 109) & 0x1F
    HW, ld, FMAX = H * W, H * W + 8, R.FLT_MAX_BITS
    inp = dict(poison=FMAX, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(c["x"].reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(c["x"].permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gt = guarded(C, HW, ld, batch=R.N_TRUTH, batch_stride=C * ld + 16, **inp).fill(c["truth_table"].reshape(R.N_TRUTH, C, HW))
    gc = guarded(C, HW, ld, batch=R.N_CLIM, batch_stride=C * ld + 16, **inp).fill(c["clim_table"].reshape(R.N_CLIM, C, HW))
    gl = guarded(1, H, **inp).fill(c["w"])
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    gcs = guarded(1, L, dtype=torch.int32, poison=R.N_CLIM, unwritten=False).fill(torch.tensor(c["c_slots"]))
    gr = guarded(1, HW, dtype=torch.int32, poison=0x7FFFFFFF, unwritten=False).fill(mask.reshape(-1).to(torch.int32))  # a guard word read as a mask: every region
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    nbytes = int(hip.lib.ldc_rollout_regional_workspace_bytes(M, Rn, C, L, H, W))
    assert nbytes == R.workspace_bytes(C, L, HW)
    gw = guarded(1, nbytes // 4, unwritten=False)
    gsum, gcnt = guarded(Rn * C * Lt, 10, dtype=torch.float64), guarded(Rn * C * Lt, 3, dtype=torch.int32)
    assert hip.lib.ldc_rollout_regional(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gc.view), gc.bs, ld,
                                        _p(gcs.view), _p(gl.view), _p(gr.view), Rn, M, C, L, H, W, _p(gsum.view), _p(gcnt.view), Lt, 1, _p(gw.view),
                                        nbytes, stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, clim=gc, lat_weight=gl, truth_slot=gts, clim_slot=gcs, region_mask=gr, mean=gm, std=gs, workspace=gw,
                     sums=gsum, counts=gcnt).items():
        assert_untouched(g, k)
    sums, counts = gsum.payload()[0].reshape(Rn, C, Lt, 10), gcnt.payload()[0].reshape(Rn, C, Lt, 3)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(counts[:, :, col]) and _unwritten(sums[:, :, col])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    for l in range(L):
        ref = R.regional_ref(xp[:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], mask, Rn, c["clim_table"][c["c_slots"][l]])
        r = R.check(dict(sums=sums[:, :, 1 + l], counts=counts[:, :, 1 + l]), ref, f"{case} {layout} lead {l}")
        print(f"guard bands {case} {layout} lead {l}: worst err / bound {r:.4f}")
        assert bool(torch.isfinite(sums[:, :, 1 + l].cpu()).all()) and int(ref["counts"][:, sst, 1].sum()) > 0  # the land points of the SST channel


def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M0, C, L0, H0, W0, R0 = 5, 2, 1, 4, 8, 3
    x, t = torch.zeros(M0, C, L0, H0, W0, device="cuda"), torch.zeros(C, L0, H0, W0, device="cuda")
    cl, w, slot = torch.zeros(C, L0, H0, W0, device="cuda"), torch.ones(H0, device="cuda"), torch.zeros(L0, dtype=torch.int32, device="cuda")
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    mask = torch.full((H0, W0), 7, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)

    def call(M=M0, L=L0, H=H0, W=W0, Cn=C, Rn=R0, L_total=L0, l_off=0, nbytes=1 << 18, forecast=x, clim=cl, clim_slot=slot, mean=None, std=None, region=mask,
             ws_off=0):
        gs, gn = guarded(R0 * C * L0, 10, dtype=torch.float64), guarded(R0 * C * L0, 3, dtype=torch.int32)
        st = hip.lib.ldc_rollout_regional(None if forecast is None else _p(forecast), x.stride(0), x.stride(2), x.stride(1), None if mean is None else _p(mean),
                                          None if std is None else _p(std), 1.0, _p(t), t.stride(1), t.stride(0), _p(slot),
                                          None if clim is None else _p(clim), cl.stride(1), cl.stride(0), None if clim_slot is None else _p(clim_slot),
                                          _p(w), None if region is None else _p(region), Rn, M, Cn, L, H, W, _p(gs.view), _p(gn.view), L_total, l_off,
                                          ctypes.c_void_p(gw.view.data_ptr() + ws_off), nbytes, stream)
        torch.cuda.synchronize()
        untouched = _unwritten(gn.payload()) and _unwritten(gs.payload())
        for g in (gs, gn, gw):
            assert_untouched(g)
        return st, untouched

    ARG, UNSUPPORTED = (-1, True), (-3, True)
    need = int(hip.lib.ldc_rollout_regional_workspace_bytes(M0, R0, C, L0, H0, W0))
    assert need == C * L0 * 3072
    assert call(forecast=None) == ARG and call(region=None) == ARG
    for kw in (dict(M=0), dict(M=-3), dict(Cn=0), dict(L=0), dict(H=0), dict(W=0), dict(Rn=0), dict(Rn=-1), dict(L_total=0), dict(l_off=-1), dict(mean=mean),
               dict(clim_slot=None)):
        assert call(**kw) == ARG, kw
    assert call(L_total=1, l_off=1) == ARG and call(L_total=3, l_off=3) == ARG  # l_off + L > L_total
    assert call(nbytes=need - 4) == ARG
    assert call(M=65) == UNSUPPORTED and call(Rn=33) == UNSUPPORTED
    assert call(L=65536, L_total=65536, nbytes=1 << 40) == UNSUPPORTED and call(Cn=65536, nbytes=1 << 40) == UNSUPPORTED
    assert call(H=4097, W=4096, nbytes=1 << 40) == UNSUPPORTED
    assert call(ws_off=4)[1] and call(ws_off=4)[0] != 0  # fp64 records: a workspace that is not 8-byte aligned is refused
    # and the calls that are served
    assert call(nbytes=need) == (0, False)
    assert call(clim=None, clim_slot=None) == (0, False)
    assert call(mean=mean, std=std) == (0, False)
    # the wrappers
    with pytest.raises(ValueError):
        E.rollout_regional(torch.zeros(65, 1, 1, 2, 4, device="cuda"), torch.zeros(1, 1, 2, 4, device="cuda"), torch.ones(2, device="cuda"), np.ones((2, 4), dtype=np.uint32), 1)
    with pytest.raises(RuntimeError):
        E.rollout_regional(x.cpu(), t, w, np.ones((H0, W0), dtype=np.uint32), 1)  # device tensors only
    out = E.empty_regional(R0, C, L0, "cuda")
    with pytest.raises(RuntimeError, match="ldc_rollout_regional"):
        hip.rollout_regional(x, t, slot, None, None, w, mask, *out._buffers, R=33, M=M0, C=C, L=L0, H=H0, W=W0, member_stride=x.stride(0),
                             lead_stride=x.stride(2), channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0), L_total=L0)


# ---- h. the driver ---------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double()), torch.nan_to_num(b.double())) \
        and torch.equal(torch.isnan(a.double()), torch.isnan(b.double()))


def test_driver_regions():
    from ladcast_amd.evaluate import NAMED_REGIONS, Region, region_mask, regional_scores, rollout_regional
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.evaluate_encdec_model import equiangular_lat_weights
    from ladcast_amd.models import AutoencoderDC
    from tests.synth import make_dcae, tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 3, 8, 3, 6, 8, 8, 48, 64, 3
    cfg = tiny_dcae_config()
    model = AutoencoderDC.from_config(cfg)
    model.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(113)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    latents = torch.randn(ENS, C_LAT, 1 + T, h, w_, generator=gen)
    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = torch.randn(6, C, H, W, generator=gen) * scale + shift
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    clim = torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift
    t_slots, c_slots = [2, 5, 3], [2, 1, 4]
    lat_w = equiangular_lat_weights(H + 1, True)
    regions = [NAMED_REGIONS["global"], NAMED_REGIONS["tropics"], NAMED_REGIONS["europe"], Region("nowhere", 0.1, 0.2, 0, 360)]
    args = (latents, model, mean, std, truth.cuda(), t_slots, clim.cuda(), c_slots, lat_w)
    kw = dict(sst_channel=SST, crop_init=True)
    plain = EG.score_latent_rollout(*args, **kw)
    got = EG.score_latent_rollout(*args, regions=regions, **kw)
    assert set(got) == set(plain) | set(EG.REGIONAL_KEYS)
    for k in SCORES:  # the five scores are the bits of a call without regions
        assert _same(got[k], plain[k]), k
    Rn = len(regions)
    s, n = got["regional_sums"], got["regional_counts"]
    assert s.shape == (Rn, C, T, 10) and s.dtype == torch.float64 and s.device.type == "cpu" and n.shape == (Rn, C, T, 3) and n.dtype == torch.int32
    # a direct call on the same decoded batches
    mask = region_mask(regions, EG.row_latitudes(H), np.arange(W) * (360.0 / W))
    assert [int(((mask >> np.uint32(r)) & 1).sum()) > 0 for r in range(Rn)] == [True, True, True, False]
    frames = torch.stack([model.decode(latents[:, :, 1 + l].contiguous().cuda()).sample for l in range(T)])  # (T, ens, C, H, W), normalised
    direct = rollout_regional(frames, truth.cuda(), lat_w.cuda(), mask, Rn, clim=clim.cuda(), clim_slots=c_slots, truth_slot=t_slots, lead_dim=0,
                              mean=mean.cuda(), std=std.cuda())
    assert torch.equal(s.view(torch.int64), direct["regional_sums"].cpu().view(torch.int64)) and torch.equal(n, direct["regional_counts"].cpu())
    assert int(n[0, SST, :, 1].min()) > 0 and int(n[0, 0, :, 1].max()) == 0 and n[0, 0, 0].tolist() == [H * W, 0, H * W]  # land: the SST channel only
    assert int(n[3].abs().sum()) == 0 and float(s[3].abs().sum()) == 0.0
    # the same bits with the mask passed in
    given = EG.score_latent_rollout(*args, regions=Rn, region_mask=mask, **kw)
    for k in EG.REGIONAL_KEYS:
        assert _same(got[k], given[k]), k
    # Another decode batch size.  The DC-AE decoder itself is not batch-invariant: a frame decoded among 6 differs from the same frame
    # decoded among 3 in 69334 of 73728 values, by at most 1.3e-6 (fp32 sums taken in another order; measured on the MI355X with this
    # model), so no sum over decoded values can hold its bits across decode_batch_frames - the five scores do not either, and
    # tests/test_gpu_evaluate_ens.py compares them per frame batch for that reason.  What the driver owes: under every decode batch size
    # the sums are the bits of a direct call on the frames as that batching decodes them; and the two batchings agree as closely as
    # their decoded frames do - counts equal (the NaNs come from the truth), sums within 1e-4 of a bound on sum |w v|: a hundred times
    # the relative difference of the decoded values.
    other = EG.score_latent_rollout(*args, regions=regions, decode_batch_frames=2 * ENS, **kw)
    lat = latents[:, :, 1:]
    chunks = [model.decode(lat[:, :, s0 : s0 + 2].permute(2, 0, 1, 3, 4).reshape(-1, C_LAT, h, w_).contiguous().cuda()).sample for s0 in (0, 2)]
    frames2 = torch.cat(chunks).reshape(T, ENS, C, H, W)
    assert not torch.equal(frames2, frames)  # the premise: the decoder's bits depend on the batch
    direct2 = rollout_regional(frames2, truth.cuda(), lat_w.cuda(), mask, Rn, clim=clim.cuda(), clim_slots=c_slots, truth_slot=t_slots, lead_dim=0,
                               mean=mean.cuda(), std=std.cuda())
    assert torch.equal(other["regional_sums"].view(torch.int64), direct2["regional_sums"].cpu().view(torch.int64))
    assert torch.equal(other["regional_counts"], direct2["regional_counts"].cpu()) and torch.equal(other["regional_counts"], n)
    # sum |w v| of every one of the ten sums is at most S0 + S2 + 2 S3 + S8 + S9: |e| <= (1 + e^2) / 2, skill <= sqrt(se + var), spread <= sqrt(2 var),
    # |fa ta| <= (fa^2 + ta^2) / 2
    scale = (s[..., 0] + s[..., 2] + 2 * s[..., 3] + s[..., 8] + s[..., 9]).unsqueeze(-1)
    assert bool(((other["regional_sums"] - s).abs() <= 1e-4 * scale).all())
    wide = EG.score_latent_rollout(*args, regions=regions, total_num_steps=T + 2, **kw)
    for k in EG.REGIONAL_KEYS:
        assert _same(wide[k][:, :, :T].contiguous(), got[k]) and float(wide[k][:, :, T:].double().abs().sum()) == 0, k
    # the global region against the five scores (plain means: the channels without NaN)
    sc = regional_scores(s.numpy(), n.numpy(), ENS)
    wsum = float(lat_w.double().sum()) * W
    for c in (0, 5):
        assert np.allclose(sc["ens_mse"][0, c] * wsum / (H * W), plain["ens_mse"][c].numpy(), rtol=1e-5)
        assert np.allclose(sc["crps"][0, c] * wsum / (H * W), plain["crps"][c].numpy(), rtol=1e-5)
        assert np.allclose(sc["ens_acc"][0, c], plain["ens_acc"][c].numpy(), rtol=1e-4, atol=1e-6)
    assert np.isfinite(sc["rmse"][:3]).all() and np.isnan(sc["rmse"][3]).all() and np.isfinite(sc["bias"][0, SST]).all()


def test_command_line_region_flags(tmp_path):
    from ladcast_amd.evaluate import REGIONAL_SCORE_NAMES, regional_scores
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.pipelines.io import save_latent_npy
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]
    gen = torch.Generator().manual_seed(127)
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
    lsm = (torch.rand(H + 1, W, generator=gen) < 0.4).float().numpy()
    np.save(tmp_path / "lsm.npy", lsm)
    flags = ["--region", "tropics", "--region", "europe", "--region_box", "box", "-30", "30", "300", "60", "--region_surface", "box", "land",
             "--land_sea_mask_path", str(tmp_path / "lsm.npy"), "--region_per_init"]

    def run(extra, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", *map(str, lv), "--num_atm_vars", "2"] + extra
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, reg = run([], "plain"), run(flags, "regions")
    new = ["regional_sums.npy", "regional_counts.npy", "regional_sums_per_init.npy", "regions.json"] + [f"regional_{k}.npy" for k in REGIONAL_SCORE_NAMES]
    assert sorted(p.name for p in reg.iterdir()) == sorted([p.name for p in plain.iterdir()] + new)
    for p in plain.iterdir():  # the five scores (and the time stamps) bit for bit
        assert (reg / p.name).read_bytes() == p.read_bytes(), p.name
    s, n, per = np.load(reg / "regional_sums.npy"), np.load(reg / "regional_counts.npy"), np.load(reg / "regional_sums_per_init.npy")
    assert s.shape == (3, C, T, 10) and s.dtype == np.float64 and n.shape == (3, C, T, 3) and n.dtype == np.int64 and per.shape == (2, 3, C, T, 10)
    assert np.array_equal(per.sum(0), s)
    meta = json.loads((reg / "regions.json").read_text())
    assert [m["name"] for m in meta["regions"]] == ["tropics", "europe", "box"] and meta["members"] == ENS and meta["regions"][2]["surface"] == "land"
    lat, lon = EG.row_latitudes(H), np.arange(W) * (360.0 / W)
    box = ((lat >= -30) & (lat <= 30))[:, None] & ((lon >= 300) | (lon <= 60))[None, :] & (lsm[1:] >= 0.5)
    assert meta["regions"][2]["n_points"] == int(box.sum()) > 0 and meta["regions"][0]["n_points"] == int((np.abs(lat) <= 20).sum()) * W
    assert (n[..., 0] == 2 * np.array([m["n_points"] for m in meta["regions"]])[:, None, None]).all() and (n[..., 1] == 0).all()  # two initial times pooled
    lat_w = EG.lat_weights_for(H).double().numpy()
    assert np.allclose(s[2, :, :, 0], 2 * (lat_w[:, None] * box).sum(), rtol=1e-12)
    sc = regional_scores(s, n, ENS)
    for k in REGIONAL_SCORE_NAMES:
        f = np.load(reg / f"regional_{k}.npy")
        assert f.shape == (3, C, T) and np.array_equal(f, sc[k], equal_nan=True), k
    assert np.isfinite(np.load(reg / "regional_rmse.npy")).all() and np.isfinite(np.load(reg / "regional_ens_acc.npy")).all()
