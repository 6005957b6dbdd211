"""The neighbourhood verification kernel (csrc/fss.hip: ldc_rollout_fss) through the C ABI and `rollout_fss`, against the integer / float64
oracle and the COUNTED bound of tests/fss_refs.py (judged on the CPU by tests/test_fss_cpu.py):
  a. the case tables: integer-valued members (ties certain), M = 1 .. 130 x four grids, the seam and pole features, land, the special fields
  b. n_invalid and the r = 0 column against ldc_rollout_events on the same inputs
  c. the perfect forecast: s5 == 0.0 exactly
  d. two lead times, slots that are not 0 .. L - 1, both layouts, out / l_off
  e. physical scale through the fused inverse normalisation: the bits of de-normalising first
  f. guard bands around every buffer and the workspace
  g. refused arguments launch nothing
  h. the same call twice gives the same bits
  i. once at (M, E, S, L, H, W) = (50, 2, 4, 2, 120, 240)
  j. the driver: score_latent_rollout(..., events=, fss_radii=) on the tiny synthetic DC-AE, and the files `main` writes"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import events_refs as ER
from tests import fss_refs as R
from tests.redzone import UNWRITTEN32, UNWRITTEN64, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    return eu


def as_events(rows):
    from ladcast_amd.evaluate import Event

    return [Event(int(c), "gt" if d > 0 else "lt", float(thr), bool(a)) for c, d, thr, a in rows]


def column(d, l):
    """lead time l of a rollout_fss result as the dict fss_refs.check takes"""
    return dict(sums=d["event_fss_sums"][:, :, l], n_invalid=d["event_fss_n_invalid"][:, l])


def run_one(E, c, **over):
    """a single-lead case of fss_refs on the device -> its one column"""
    c = dict(c, **over)
    kw = {}
    if c["norm"] is not None:
        kw = dict(mean=c["norm"][0].cuda(), std=c["norm"][1].cuda(), target_std=c["norm"][2])
    d = E.rollout_fss(c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), as_events(c["events"]), c["radii"],
                      clim=c["cl"].cuda()[:, None], **kw)
    n_ev, S = len(c["events"]), len(c["radii"])
    assert d["event_fss_sums"].dtype == torch.float64 and d["event_fss_n_invalid"].dtype == torch.int32
    assert d["event_fss_sums"].shape == (n_ev, S, 1, 6) and d["event_fss_n_invalid"].shape == (n_ev, 1)
    return column(d, 0)


def ref_of(c):
    return R.fss_ref(c["x"], c["t"], c["w"], c["events"], c["radii"], c["cl"])


# ---- a. the case tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W", R.INT_CASES)
def test_integers(E, M, H, W):
    c = R.integer_case(M, H, W)
    got, ref = run_one(E, c), ref_of(c)
    r = R.check(got, ref, f"M={M} {H}x{W}")
    print(f"integers M={M} {H}x{W}: worst err / bound {r:.4f}")
    assert (got["sums"] >= 0).all()


@pytest.mark.parametrize("kind", R.SPECIAL_KINDS)
def test_special_fields(E, kind):
    from ladcast_amd.evaluate import fss_scores

    c = R.special_case(kind)
    got = run_one(E, c)
    R.check(got, ref_of(c), kind)
    s = got["sums"].cpu().numpy()
    fss = fss_scores(s)["fss"]
    if kind == "perfect":  # ---- c. s5 == 0.0 and fss == 1.0 exactly
        assert (s[..., 5] == 0.0).all() and (s[..., 3] > 0).any() and (fss[s[..., 3] > 0] == 1.0).all()
        assert np.array_equal(s[..., 1], s[..., 2]) and np.array_equal(s[..., 3], s[..., 4])
    elif kind == "all_event":
        assert (s[..., 5] == 0.0).all() and (fss == 1.0).all()
    else:
        assert (s[..., 1:] == 0.0).all() and np.isnan(fss).all()


# ---- b. against ldc_rollout_events -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W", [(9, 5, 7), (65, 17, 33)])
def test_radius_zero_is_the_brier_numerator_of_rollout_events(E, M, H, W):
    c = R.integer_case(M, H, W)
    ev = as_events(c["events"])
    args = (c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), ev)
    f = E.rollout_fss(*args, (0,), clim=c["cl"].cuda()[:, None])
    h = E.rollout_events(*args, clim=c["cl"].cuda()[:, None])
    assert torch.equal(f["event_fss_n_invalid"], h["event_n_invalid"]) and int(h["event_n_invalid"].sum()) > 0
    hw = h["event_hist_weighted"][:, 0].cpu().double().numpy()  # (E, M + 1, 2)
    p = (np.arange(M + 1) / M).reshape(1, M + 1)
    coef = np.stack([p ** 2, (p - 1.0) ** 2], -1)  # (1, M + 1, 2), both <= 1
    brier_num = (hw * coef).sum((-1, -2))
    # the histogram's counted fp32 bound per bin (events_refs), weighted by the coefficients, plus the counted float64 bound of s5 and a
    # few float64 roundings of the sum above
    b_hist = (ER.events_ref(c["x"], c["t"], c["w"], c["events"], c["cl"])["hist_w"][1].numpy() * coef).sum((-1, -2))
    s5 = f["event_fss_sums"][:, 0, 0, 5].cpu().numpy()
    tol = b_hist + R.bound(s5, H * W) + 2 * (M + 1) * 4 * R.U64 * brier_num
    print(f"M={M} {H}x{W}: |s5 - brier numerator| / tolerance {np.abs(s5 - brier_num) / np.maximum(tol, 1e-300)}")
    assert (np.abs(s5 - brier_num) <= tol).all() and (s5 > 0).all()
    s0 = f["event_fss_sums"][:, 0, 0, 0].cpu().numpy()
    assert (np.abs(s0 - hw.sum((-1, -2))) <= ER.events_ref(c["x"], c["t"], c["w"], c["events"], c["cl"])["hist_w"][1].numpy().sum((-1, -2))
            + R.bound(s0, H * W)).all()


# ---- d. two lead times, slots, layouts, out / l_off --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
def test_two_leads_slots_and_layouts(E, layout):
    c = R.mix_case()
    M, C, L, H, W = R.MIX_SHAPE
    S, n_ev = len(c["radii"]), len(c["events"])
    xd = c["x"].cuda()
    kw = dict(clim=c["clim_table"].cuda(), clim_slots=c["c_slots"], truth_slot=c["t_slots"])
    if layout == "frame_major":
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    d = E.rollout_fss(xd, c["truth_table"].cuda(), c["w"].cuda(), as_events(c["events"]), c["radii"], **kw)
    assert d["event_fss_sums"].shape == (n_ev, S, L, 6)
    for l in range(L):
        ref = R.fss_ref(c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], c["events"], c["radii"], c["clim_table"][c["c_slots"][l]])
        R.check(column(d, l), ref, f"{layout} lead {l}")
    assert not torch.equal(d["event_fss_sums"][:, :, 0], d["event_fss_sums"][:, :, 1])
    # filling an existing result: the columns outside l_off .. l_off + L - 1 keep what they held
    out = E.empty_fss(n_ev, S, L + 2, "cuda")
    for b in out._buffers:
        b.fill_(7)
    d2 = E.rollout_fss(xd, c["truth_table"].cuda(), c["w"].cuda(), as_events(c["events"]), c["radii"], out=out, l_off=1, **kw)
    assert torch.equal(d2["event_fss_sums"][:, :, 1 : 1 + L], d["event_fss_sums"]) and torch.equal(d2["event_fss_n_invalid"][:, 1 : 1 + L], d["event_fss_n_invalid"])
    assert bool((d2["event_fss_sums"][:, :, 0] == 7).all()) and bool((d2["event_fss_sums"][:, :, L + 1] == 7).all())
    assert bool((d2["event_fss_n_invalid"][:, 0] == 7).all()) and bool((d2["event_fss_n_invalid"][:, L + 1] == 7).all())


# ---- e. physical scale -------------------------------------------------------------------------------------------------------------------
def test_physical_scale_fused_equals_denormalised_first(E):
    c = dict(ER.physical_case(R.PHYS_M), radii=R.PHYS_RADII)
    got, ref = run_one(E, c), ref_of(c)
    r = R.check(got, ref, "physical")
    print(f"physical M={R.PHYS_M}: worst err / bound {r:.4f}")
    plain = run_one(E, c, v=c["x"], norm=None)
    for k in got:
        assert torch.equal(plain[k], got[k]), k
    assert (ref["sums"][0][:, :, 3] > 0).all() and (ref["sums"][0][:, :, 4] > 0).all()  # the thresholds cut the fields


# ---- f. guard bands ----------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    t = t.detach().cpu().contiguous()
    if t.element_size() == 8:
        return bool((t.view(torch.int64) == UNWRITTEN64).all())
    return bool((t.view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", ER.GUARD_CASES)
def test_guard_bands(case, layout):
    from ladcast_amd import hip

    M, C, L, H, W, sst = case
    c = ER.guard_case(*case)
    events = ER.guard_events(C)
    radii = (0, 1, (W - 1) // 2)
    n_ev, S = len(events), len(radii)
    HW, ld, FMAX = H * W, H * W + 8, ER.R.FLT_MAX_BITS
    inp = dict(poison=FMAX, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(c["x"].reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(c["x"].permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gt = guarded(C, HW, ld, batch=ER.N_TRUTH, batch_stride=C * ld + 16, **inp).fill(c["truth_table"].reshape(ER.N_TRUTH, C, HW))
    gc = guarded(C, HW, ld, batch=ER.N_CLIM, batch_stride=C * ld + 16, **inp).fill(c["clim_table"].reshape(ER.N_CLIM, C, HW))
    gl = guarded(1, H, **inp).fill(c["w"])
    assert gt.bs < 4096  # a slot read from a guard word points one entry past the table, into its poisoned back guard
    gts = guarded(1, L, dtype=torch.int32, poison=ER.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    gcs = guarded(1, L, dtype=torch.int32, poison=ER.N_CLIM, unwritten=False).fill(torch.tensor(c["c_slots"]))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    nbytes = int(hip.lib.ldc_rollout_fss_workspace_bytes(M, n_ev, S, L, H, W))
    assert nbytes == R.workspace_bytes(n_ev, S, L, H, W) and nbytes % 8 == 0
    gw = guarded(1, nbytes // 4, unwritten=False)
    gsum, gn = guarded(n_ev * S * Lt, 6, dtype=torch.float64), guarded(n_ev, Lt, dtype=torch.int32)
    desc = hip.events_desc(events)
    rad = (ctypes.c_int * S)(*radii)
    assert hip.lib.ldc_rollout_fss(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gc.view), gc.bs, ld,
                                   _p(gcs.view), _p(gl.view), M, C, L, H, W, ctypes.byref(desc), rad, S, _p(gsum.view), _p(gn.view), Lt, 1,
                                   _p(gw.view), nbytes, stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, clim=gc, lat_weight=gl, truth_slot=gts, clim_slot=gcs, mean=gm, std=gs, workspace=gw, fss_sums=gsum,
                     n_invalid=gn).items():
        assert_untouched(g, k)
    sums, ninv = gsum.payload()[0].reshape(n_ev, S, Lt, 6), gn.payload()[0].reshape(n_ev, Lt)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(ninv[:, col]) and _unwritten(sums[:, :, col])
    xp = ER.inv_norm_f32(c["x"], mean, std, ts)
    for l in range(L):
        ref = R.fss_ref(xp[:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], events, radii, c["clim_table"][c["c_slots"][l]])
        r = R.check(dict(sums=sums[:, :, 1 + l], n_invalid=ninv[:, 1 + l]), ref, f"{case} {layout} lead {l}")
        print(f"guard bands {case} {layout} lead {l}: worst err / bound {r:.4f}")
        if sst in (0, C - 1):
            assert int(ref["n_invalid"].sum()) > 0 and int(ref["reduced"].sum()) > 0  # the land points of the SST channel


# ---- g. arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M0, C, L0, H0, W0, S0 = 5, 2, 1, 4, 8, 2
    x, t = torch.zeros(M0, C, L0, H0, W0, device="cuda"), torch.zeros(C, L0, H0, W0, device="cuda")
    cl, w, slot = torch.zeros(C, L0, H0, W0, device="cuda"), torch.ones(H0, device="cuda"), torch.zeros(L0, dtype=torch.int32, device="cuda")
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)
    good = [(1, 1, 0.5, 0), (0, -1, 0.0, 1)]

    def call(M=M0, L=L0, H=H0, W=W0, Cn=C, L_total=L0, l_off=0, nbytes=1 << 18, events=good, forecast=x, clim=cl, clim_slot=slot, mean=None, std=None,
             raw=None, radii=(0, 3), S=None, null_radii=False, ws_shift=0, sums_shift=0):
        desc = hip.events_desc(events)
        if raw is not None:  # a field the host helper would refuse
            field, index, value = raw
            if field == "n_events":
                desc.n_events = value
            else:
                getattr(desc, field)[index] = value
        gsum, gn = guarded(2 * S0 * L0, 6, dtype=torch.float64), guarded(2, L0, dtype=torch.int32)
        rad = (ctypes.c_int * max(len(radii), 1))(*radii)
        st = hip.lib.ldc_rollout_fss(None if forecast is None else _p(forecast), x.stride(0), x.stride(2), x.stride(1), None if mean is None else _p(mean),
                                     None if std is None else _p(std), 1.0, _p(t), t.stride(1), t.stride(0), _p(slot),
                                     None if clim is None else _p(clim), cl.stride(1), cl.stride(0), None if clim_slot is None else _p(clim_slot),
                                     _p(w), M, Cn, L, H, W, ctypes.byref(desc), None if null_radii else rad, len(radii) if S is None else S,
                                     ctypes.c_void_p(gsum.view.data_ptr() + sums_shift), _p(gn.view), L_total, l_off,
                                     ctypes.c_void_p(gw.view.data_ptr() + ws_shift), nbytes, stream)
        torch.cuda.synchronize()
        untouched = all(_unwritten(g.payload()) for g in (gsum, gn))
        for g in (gsum, gn, gw):
            assert_untouched(g)
        return st, untouched

    ARG, ALIGN, UNSUPPORTED = (-1, True), (-2, True), (-3, True)
    need = int(hip.lib.ldc_rollout_fss_workspace_bytes(M0, 2, S0, L0, H0, W0))
    assert need == R.workspace_bytes(2, S0, L0, H0, W0)
    # LDC_ERR_ARG: everything ldc_rollout_events refuses
    assert call(forecast=None) == ARG
    for kw in (dict(M=0), dict(M=-3), dict(Cn=0), dict(L=0), dict(H=0), dict(W=0), dict(L_total=0), dict(l_off=-1), dict(mean=mean), dict(clim_slot=None)):
        assert call(**kw) == ARG, kw
    for raw in (("n_events", 0, 0), ("n_events", 0, 33), ("n_events", 0, -1), ("channel", 0, -1), ("channel", 1, C), ("dir", 0, 0), ("dir", 1, 2),
                ("anomaly", 0, 2), ("anomaly", 1, -1), ("thr", 0, float("nan"))):
        assert call(raw=raw) == ARG, raw
    assert call(clim=None, clim_slot=None) == ARG  # an anomaly event without a climatology
    assert call(L_total=1, l_off=1) == ARG and call(L_total=3, l_off=3) == ARG  # l_off + L > L_total
    assert call(nbytes=need - 8) == ARG
    # ... and the radii: none, too many, negative, a window wider than a row
    assert call(null_radii=True) == ARG and call(radii=(), S=0) == ARG and call(radii=tuple(range(4)) * 4 + (0,), W=64) == ARG
    assert call(radii=(0, -1)) == ARG and call(radii=(4,)) == ARG  # 2 r + 1 = 9 > W = 8
    # LDC_ERR_UNSUPPORTED
    assert call(M=1025) == UNSUPPORTED
    assert call(L=65536, L_total=65536, nbytes=1 << 40) == UNSUPPORTED
    assert call(H=4097, W=4096, nbytes=1 << 40) == UNSUPPORTED
    assert call(M=1024, H=2048, W=2048, nbytes=1 << 40) == UNSUPPORTED  # M H W = 2^32: Sn would not fit uint32
    # LDC_ERR_ALIGN
    assert call(ws_shift=4) == ALIGN and call(sums_shift=4) == ALIGN
    # and the calls that are served
    assert call(nbytes=need) == (0, False)
    assert call(radii=(3,)) == (0, False)  # 2 r + 1 = 7 >= H = 4: every row
    assert call(clim=None, clim_slot=None, events=[(1, 1, 0.5, 0)]) == (0, False)
    assert call(mean=mean, std=std) == (0, False)
    # the wrappers
    with pytest.raises(RuntimeError):
        E.rollout_fss(x.cpu(), t, w, as_events([(0, 1, 0.5, 0)]), (0,))  # device tensors only
    bad = hip.events_desc([(0, 1, 0.5, 0)])
    bad.channel[0] = C
    out = E.empty_fss(1, 1, L0, "cuda")
    with pytest.raises(RuntimeError, match="ldc_rollout_fss"):
        hip.rollout_fss(x, t, slot, None, None, w, bad, (0,), *out._buffers, M=M0, C=C, L=L0, H=H0, W=W0, member_stride=x.stride(0), lead_stride=x.stride(2),
                        channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0), L_total=L0)


# ---- h. repeatability --------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(E):
    for c in (R.integer_case(65, 17, 33), R.integer_case(130, 3, 50)):
        a, b = run_one(E, c), run_one(E, c)
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- i. one large case -------------------------------------------------------------------------------------------------------------------
def test_production_grid_once(E):
    from ladcast_amd.evaluate import fss_scores

    M, n_ev, S, L, H, W = R.BIG_SHAPE
    c = R.big_case()
    d = E.rollout_fss(c["x"].cuda(), c["truth_table"].cuda(), c["w"].cuda(), as_events(c["events"]), c["radii"], truth_slot=list(range(L)))
    assert d["event_fss_sums"].shape == (n_ev, S, L, 6)
    for l in range(L):
        ref = R.fss_ref(c["x"][:, :, l], c["truth_table"][l], c["w"], c["events"], c["radii"])
        r = R.check(column(d, l), ref, f"lead {l}")
        print(f"production grid lead {l}: worst err / bound {r:.4f}")
        assert int(ref["n_invalid"][1]) > 1000 and int(ref["n_invalid"][0]) == 0 and (ref["reduced"][1, 1:] > 0).all()
    fss = fss_scores(d["event_fss_sums"].cpu().numpy())["fss"]
    assert np.isfinite(fss).all() and (fss[:, 1] > fss[:, 0]).all()  # the truth's features lie 3 columns off: a wider window sees them


# ---- j. the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_fss():
    from ladcast_amd.evaluate import Event, rollout_fss
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.evaluate_encdec_model import equiangular_lat_weights
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D
    from tests.synth import make_dcae, tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 3, 8, 3, 6, 8, 8, 48, 64, 3
    cfg = tiny_dcae_config()
    model = AutoencoderDC.from_config(cfg)
    model.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(61)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    latents = torch.randn(ENS, C_LAT, 1 + T, h, w_, generator=gen)
    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = torch.randn(6, C, H, W, generator=gen) * scale + shift
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    clim = torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift
    t_slots, c_slots = [2, 5, 3], [2, 1, 4]
    lat_w = equiangular_lat_weights(H + 1, True)
    fields = []
    for l in range(T):
        y = model.decode(latents[:, :, 1 + l].contiguous().cuda()).sample
        fields.append(inverse_normalize_transform_3D(y.reshape(ENS, C, 1, H, W), mean, std).reshape(ENS, C, H, W))
    phys = torch.stack(fields, 2)  # (ens, C, T, H, W)
    med = [round(float(phys[:, c].median()), 2) for c in range(C)]
    events = [Event(1, "gt", med[1]), Event(6, "gt", 0.1, True), Event(SST, "lt", med[SST])]
    radii = [0, 2, 31]
    args = (latents, model, mean, std, truth.cuda(), t_slots, clim.cuda(), c_slots, lat_w)
    kw = dict(sst_channel=SST, crop_init=True)
    plain = EG.score_latent_rollout(*args, events=events, **kw)
    got = EG.score_latent_rollout(*args, events=events, fss_radii=radii, **kw)
    assert set(got) == set(plain) | set(EG.FSS_KEYS)
    for k in plain:  # every other output is the bits of a call without the radii
        assert torch.equal(torch.nan_to_num(got[k].double()), torch.nan_to_num(plain[k].double())), k
    assert got["event_fss_sums"].shape == (3, 3, T, 6) and got["event_fss_sums"].dtype == torch.float64 and got["event_fss_sums"].device.type == "cpu"
    assert torch.equal(got["event_fss_n_invalid"], got["event_n_invalid"]) and int(got["event_n_invalid"][2].sum()) > 0
    direct = rollout_fss(phys, truth.cuda(), lat_w.cuda(), events, radii, clim=clim.cuda(), clim_slots=c_slots, truth_slot=t_slots)
    for k in EG.FSS_KEYS:
        assert torch.equal(got[k], direct[k].cpu()), k
    rows = [(e.channel, 1 if e.direction == "gt" else -1, e.threshold, int(e.anomaly)) for e in events]
    for l in range(T):
        ref = R.fss_ref(phys[:, :, l].cpu(), truth[t_slots[l]], lat_w, rows, radii, clim[c_slots[l]])
        R.check(dict(sums=got["event_fss_sums"][:, :, l], n_invalid=got["event_fss_n_invalid"][:, l]), ref, f"lead {l}")
    other = EG.score_latent_rollout(*args, events=events, fss_radii=radii, decode_batch_frames=2 * ENS, total_num_steps=T + 1, **kw)
    for k in EG.FSS_KEYS:  # another decode batch size; the column past the last lead time stays zero
        assert torch.equal(other[k][..., :T, :] if k == "event_fss_sums" else other[k][:, :T], got[k]), k
    assert float(other["event_fss_sums"][:, :, T].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="fss_radii needs events"):
        EG.score_latent_rollout(*args, fss_radii=radii, **kw)
    with pytest.raises(ValueError, match="wider"):
        EG.score_latent_rollout(*args, events=events, fss_radii=[32], **kw)  # 65 > W = 64


def test_command_line_fss_scales(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate import fss_scores
    from ladcast_amd.pipelines.io import save_latent_npy
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]
    gen = torch.Generator().manual_seed(67)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    lv = (300, 500, 850)
    norm = {"geopotential": {"mean": {str(p): float(mean[i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {str(p): float(mean[3 + i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(mean[6]), "std": float(std[6])}, "sea_surface_temperature": {"mean": float(mean[7]), "std": float(std[7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    save_latent_npy(torch.randn(2, ENS, C_LAT, 1 + T, h, w_, generator=gen), inits, str(tmp_path / "rollout"))
    truth = torch.randn(11, C, H, W, generator=gen) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H, W))  # sparse: zeros
    clim.flush()
    del clim
    thr = round(float(mean[6]), 3)
    flags = ["--event", "2m_temperature", "gt", str(thr), "--event_anomaly", "geopotential_level500", "lt", str(round(float(mean[1]) - 0.1, 3))]

    def run(extra, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", *map(str, lv), "--num_atm_vars", "2"] + extra
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            out = EG.main(argv)
        return tmp_path / name, out

    (ev, _), (fs, out) = run(flags, "events"), run(flags + ["--fss_scales", "0", "3", "12"], "fss")
    files = ("event_fss_sums", "event_fss_n_invalid", "event_fss", "event_fss_target", "event_fss_obs_fraction", "event_fss_freq_bias",
             "event_fss_useful_scale")
    assert sorted(p.name for p in fs.iterdir()) == sorted([p.name for p in ev.iterdir()] + [f"{k}.npy" for k in files])
    for p in ev.iterdir():  # everything a run without the flag writes, bit for bit - events.json aside, which gains two entries
        if p.name != "events.json":
            assert (fs / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(fs / f"{k}.npy") for k in files}
    assert a["event_fss_sums"].shape == (2, 3, T, 6) and a["event_fss_sums"].dtype == np.float64 and (a["event_fss_sums"] >= 0).all()
    assert np.array_equal(a["event_fss_n_invalid"], np.load(fs / "event_n_invalid.npy"))
    sc = fss_scores(a["event_fss_sums"], [0, 3, 12])
    for f, k in (("event_fss", "fss"), ("event_fss_target", "fss_target"), ("event_fss_obs_fraction", "obs_fraction"), ("event_fss_freq_bias", "freq_bias")):
        assert a[f].shape == (2, 3, T) and np.array_equal(a[f], sc[k]) and np.isfinite(a[f]).all(), f
    assert a["event_fss_useful_scale"].shape == (2, T) and np.array_equal(a["event_fss_useful_scale"], sc["useful_scale"])
    # r = 0 pooled over the two initial times: the Brier score of the pooled histogram.  Its numerator and its total weight are fp32 sums
    # of at most H W weights per bin and 12 records (events_refs: (n_b + nrec) 2^-24 each), so the quotient is within twice that
    brier = np.load(fs / "event_brier.npy")
    s = a["event_fss_sums"][:, 0]
    assert np.allclose(s[..., 5] / s[..., 0], brier, rtol=2 * (H * W + 12 + 4) * 2.0 ** -24, atol=0)
    meta = json.loads((fs / "events.json").read_text())
    assert meta["fss_radii"] == [0, 3, 12] and meta["fss_width_deg"] == [(2 * r + 1) * 360.0 / W for r in (0, 3, 12)]
    assert meta["events"] == json.loads((ev / "events.json").read_text())["events"]
