"""The threshold-event kernel (csrc/events.hip: ldc_rollout_events) through the C ABI and `rollout_events`, against the integer / float64
oracle and the COUNTED bound of tests/events_refs.py (judged on the CPU by tests/test_events_cpu.py):
  a. integer-valued members and thresholds (ties certain), M = 1 .. 1024 x three grids: every register arm and its boundary, the streaming
     arm, 256 bins, the second and the partial ninth bin slot per thread; hist_count and n_invalid bit-exact
  b. the event mix: two events on one channel, one anomaly event on another, two lead times, slots that are not 0 .. L - 1, both layouts
  c. physical scale through the fused inverse normalisation, thresholds on values that members take exactly
  d. the finish loop: 65 and 129 records
  e. the NaN / inf table
  f. guard bands around every buffer, the columns outside l_off .. l_off + L - 1 left alone
  g. refused arguments launch nothing
  h. consistency with ldc_rollout_products' exceedance planes; repeatability
  i. the driver: score_latent_rollout(..., events=...) on the tiny synthetic DC-AE"""
import ctypes

import numpy as np
import pytest
import torch

from tests import events_refs as R
from tests.redzone import UNWRITTEN32, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    return eu


def as_events(rows):
    from ladcast_amd.evaluate import Event

    return [Event(int(c), "gt" if d > 0 else "lt", float(thr), bool(a)) for c, d, thr, a in rows]


def column(d, l):
    """lead time l of a rollout_events result as the dict events_refs.check takes"""
    return dict(hist=d["event_hist"][:, l], hist_w=d["event_hist_weighted"][:, l], n_invalid=d["event_n_invalid"][:, l])


def run_one(E, c, **over):
    """a single-lead case of events_refs on the device -> its one column"""
    c = dict(c, **over)
    kw = {}
    if c["norm"] is not None:
        kw = dict(mean=c["norm"][0].cuda(), std=c["norm"][1].cuda(), target_std=c["norm"][2])
    d = E.rollout_events(c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), as_events(c["events"]), clim=c["cl"].cuda()[:, None], **kw)
    M, n_ev = c["v"].shape[0], len(c["events"])
    assert d["event_hist"].dtype == torch.int32 and d["event_n_invalid"].dtype == torch.int32 and d["event_hist_weighted"].dtype == torch.float32
    assert d["event_hist"].shape == d["event_hist_weighted"].shape == (n_ev, 1, M + 1, 2) and d["event_n_invalid"].shape == (n_ev, 1)
    return column(d, 0)


def ref_of(c):
    return R.events_ref(c["x"], c["t"], c["w"], c["events"], c["cl"])


# ---- a. integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,H,W", R.INT_CASES)
def test_integers(E, M, H, W):
    c = R.integer_case(M, H, W)
    got, ref = run_one(E, c), ref_of(c)
    r = R.check(got, ref, f"M={M} {H}x{W}")
    print(f"integers M={M} {H}x{W}: worst err / bound {r:.4f}")
    P = H * W
    assert got["n_invalid"].cpu().tolist() == [0] * len(c["events"])
    assert got["hist"].sum((-1, -2)).cpu().tolist() == [P - int(n) for n in got["n_invalid"]]
    assert int(ref["hist"][0, M].sum()) > 0 and int(ref["hist"][0, 0].sum()) > 0  # the two end bins are in use


# ---- b. the event mix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
def test_event_mix_two_leads_and_slots(E, layout):
    c = R.mix_case()
    M, C, L, H, W = R.MIX_SHAPE
    xd = c["x"].cuda()
    kw = dict(clim=c["clim_table"].cuda(), clim_slots=c["c_slots"], truth_slot=c["t_slots"])
    if layout == "frame_major":
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    d = E.rollout_events(xd, c["truth_table"].cuda(), c["w"].cuda(), as_events(c["events"]), **kw)
    assert d["event_hist"].shape == (3, L, M + 1, 2)
    for l in range(L):
        ref = R.events_ref(c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], c["events"], c["clim_table"][c["c_slots"][l]])
        R.check(column(d, l), ref, f"{layout} lead {l}")
    # filling an existing result: the columns outside l_off .. l_off + L - 1 keep what they held
    out = E.empty_events(M, 3, L + 2, "cuda")
    for b in out._buffers:
        b.fill_(7)
    d2 = E.rollout_events(xd, c["truth_table"].cuda(), c["w"].cuda(), as_events(c["events"]), out=out, l_off=1, **kw)
    for k in d:
        assert torch.equal(d2[k][:, 1 : 1 + L], d[k]), k
        assert bool((d2[k][:, 0] == 7).all()) and bool((d2[k][:, L + 1] == 7).all()), k


# ---- c. physical scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M):
    c = R.physical_case(M)
    got, ref = run_one(E, c), ref_of(c)
    r = R.check(got, ref, f"M={M}")
    print(f"physical M={M}: worst err / bound {r:.4f}")
    # the same bits from fields de-normalised first, and from the decoder's frame-major layout
    plain = run_one(E, c, v=c["x"], norm=None)
    mean, std, ts = c["norm"]
    frames = c["v"].cuda()[None].contiguous()  # (L = 1, ens, C, H, W)
    fm = E.rollout_events(frames, c["t"].cuda()[:, None], c["w"].cuda(), as_events(c["events"]), clim=c["cl"].cuda()[:, None], lead_dim=0,
                          mean=mean.cuda(), std=std.cuda(), target_std=ts)
    for k, v in column(fm, 0).items():
        assert torch.equal(v, got[k]) and torch.equal(plain[k], got[k]), k


# ---- d. the finish loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.FINISH_SHAPES)
def test_finish_loop(E, H, W):
    c = R.finish_case(H, W)
    assert R.n_records(H * W, c["v"].shape[0]) == -(-H * W // 256) > 64
    got = run_one(E, c)
    r = R.check(got, ref_of(c), f"{H}x{W}")
    print(f"finish loop {H}x{W}: worst err / bound {r:.4f}")
    again = run_one(E, c)  # repeatability: no float atomics, so the same bits
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---- e. NaN / inf table ----------------------------------------------------------------------------------------------------------------
def test_nan_inf_table(E):
    c = R.nan_table_case()
    got, ref = run_one(E, c), ref_of(c)
    R.check(got, ref, "nan table")
    P = c["v"].shape[2] * c["v"].shape[3]
    invalid = R.nan_table_invalid(c["kind"])
    assert got["n_invalid"].cpu().tolist() == invalid and invalid[2] > invalid[3] > 0  # the NaN climatology: the anomaly event only
    assert got["hist"].sum((-1, -2)).cpu().tolist() == [P - n for n in invalid]
    # channel 2 is NaN everywhere and no event reads it: replacing it changes nothing
    v2 = c["v"].clone()
    v2[:, 2] = 0.0
    t2 = c["t"].clone()
    t2[2] = float("nan")
    other = run_one(E, c, v=v2, t=t2)
    for k in got:
        assert torch.equal(got[k], other[k]), k


def test_inf_is_an_ordered_value(E):
    inf = float("inf")
    x = torch.tensor([[inf, 0.0, -inf], [0.0, 0.0, -inf]]).reshape(2, 1, 1, 1, 3).cuda()  # members (inf, 0), (0, 0), (-inf, -inf)
    t = torch.tensor([-inf, inf, 0.0]).reshape(1, 1, 1, 3).cuda()
    d = E.rollout_events(x, t, torch.ones(1).cuda(), as_events([(0, 1, 1e30, 0), (0, -1, -1e30, 0)]))
    h = d["event_hist"][:, 0].cpu()
    assert h[0].nonzero().tolist() == [[0, 0], [0, 1], [1, 0]]  # gt 1e30: n = 1, 0, 0 and o = 0, 1, 0
    assert h[0, 0].tolist() == [1, 1] and h[0, 1].tolist() == [1, 0]
    assert h[1, 0].tolist() == [1, 1] and h[1, 2].tolist() == [1, 0]  # lt -1e30: n = 0, 0, 2 and o = 1, 0, 0
    assert d["event_n_invalid"].cpu().tolist() == [[0], [0]] and d["event_hist_weighted"][:, 0].cpu().tolist() == h.float().tolist()


# ---- f. guard bands --------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", R.GUARD_CASES)
def test_guard_bands(case, layout):
    from ladcast_amd import hip

    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    events = R.guard_events(C)
    n_ev = len(events)
    HW, ld, FMAX = H * W, H * W + 8, R.R.FLT_MAX_BITS
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
    assert gt.bs < 4096  # a slot read from a guard word points one entry past the table, into its poisoned back guard
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    gcs = guarded(1, L, dtype=torch.int32, poison=R.N_CLIM, unwritten=False).fill(torch.tensor(c["c_slots"]))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt, NB = L + 2, 2 * (M + 1)
    nbytes = int(hip.lib.ldc_rollout_events_workspace_bytes(M, n_ev, L, H, W))
    assert nbytes == R.workspace_bytes(M, n_ev, L, HW)
    gw = guarded(1, nbytes // 4, unwritten=False)
    gh, ghw, gn = guarded(n_ev * Lt, NB, dtype=torch.int32), guarded(n_ev * Lt, NB), guarded(n_ev, Lt, dtype=torch.int32)
    desc = hip.events_desc(events)
    assert hip.lib.ldc_rollout_events(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gc.view), gc.bs, ld,
                                      _p(gcs.view), _p(gl.view), M, C, L, H, W, ctypes.byref(desc), _p(gh.view), _p(ghw.view), _p(gn.view), Lt, 1,
                                      _p(gw.view), nbytes, stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, clim=gc, lat_weight=gl, truth_slot=gts, clim_slot=gcs, mean=gm, std=gs, workspace=gw, hist_count=gh,
                     hist_weight=ghw, n_invalid=gn).items():
        assert_untouched(g, k)
    hist, hist_w = gh.payload()[0].reshape(n_ev, Lt, M + 1, 2), ghw.payload()[0].reshape(n_ev, Lt, M + 1, 2)
    ninv = gn.payload()[0].reshape(n_ev, Lt)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(ninv[:, col]) and _unwritten(hist[:, col]) and _unwritten(hist_w[:, col])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    for l in range(L):
        ref = R.events_ref(xp[:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], events, c["clim_table"][c["c_slots"][l]])
        got = dict(hist=hist[:, 1 + l], hist_w=hist_w[:, 1 + l], n_invalid=ninv[:, 1 + l])
        r = R.check(got, ref, f"{case} {layout} lead {l}")
        print(f"guard bands {case} {layout} lead {l}: worst err / bound {r:.4f}")
        assert bool(torch.isfinite(got["hist_w"]).all())
        if sst in (0, C - 1):
            assert int(ref["n_invalid"].sum()) > 0  # the land points of the SST channel


# ---- g. arguments ----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M0, C, L0, H0, W0 = 5, 2, 1, 4, 8
    x, t = torch.zeros(M0, C, L0, H0, W0, device="cuda"), torch.zeros(C, L0, H0, W0, device="cuda")
    cl, w, slot = torch.zeros(C, L0, H0, W0, device="cuda"), torch.ones(H0, device="cuda"), torch.zeros(L0, dtype=torch.int32, device="cuda")
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)
    good = [(1, 1, 0.5, 0), (0, -1, 0.0, 1)]

    def call(M=M0, L=L0, H=H0, W=W0, Cn=C, L_total=L0, l_off=0, nbytes=1 << 18, events=good, forecast=x, clim=cl, clim_slot=slot, mean=None, std=None,
             raw=None):
        desc = hip.events_desc(events)
        if raw is not None:  # a field the host helper would refuse
            field, index, value = raw
            if field == "n_events":
                desc.n_events = value
            else:
                getattr(desc, field)[index] = value
        gh, ghw, gn = guarded(2 * L0, 2 * (M0 + 1), dtype=torch.int32), guarded(2 * L0, 2 * (M0 + 1)), guarded(2, L0, dtype=torch.int32)
        st = hip.lib.ldc_rollout_events(None if forecast is None else _p(forecast), x.stride(0), x.stride(2), x.stride(1), None if mean is None else _p(mean),
                                        None if std is None else _p(std), 1.0, _p(t), t.stride(1), t.stride(0), _p(slot),
                                        None if clim is None else _p(clim), cl.stride(1), cl.stride(0), None if clim_slot is None else _p(clim_slot),
                                        _p(w), M, Cn, L, H, W, ctypes.byref(desc), _p(gh.view), _p(ghw.view), _p(gn.view), L_total, l_off, _p(gw.view),
                                        nbytes, stream)
        torch.cuda.synchronize()
        untouched = all(_unwritten(g.payload()) for g in (gh, ghw, gn))
        for g in (gh, ghw, gn, gw):
            assert_untouched(g)
        return st, untouched

    ARG, UNSUPPORTED = (-1, True), (-3, True)
    need = int(hip.lib.ldc_rollout_events_workspace_bytes(M0, 2, L0, H0, W0))
    assert need == 4 * 2 * (4 + 4 * (M0 + 1))
    # LDC_ERR_ARG: null or non-positive arguments
    assert call(forecast=None) == ARG
    for kw in (dict(M=0), dict(M=-3), dict(Cn=0), dict(L=0), dict(H=0), dict(W=0), dict(L_total=0), dict(l_off=-1), dict(mean=mean), dict(clim_slot=None)):
        assert call(**kw) == ARG, kw
    # the descriptor
    for raw in (("n_events", 0, 0), ("n_events", 0, 33), ("n_events", 0, -1), ("channel", 0, -1), ("channel", 1, C), ("dir", 0, 0), ("dir", 1, 2),
                ("anomaly", 0, 2), ("anomaly", 1, -1), ("thr", 0, float("nan"))):
        assert call(raw=raw) == ARG, raw
    assert call(clim=None, clim_slot=None) == ARG  # an anomaly event without a climatology
    assert call(L_total=1, l_off=1) == ARG and call(L_total=3, l_off=3) == ARG  # l_off + L > L_total
    assert call(nbytes=need - 4) == ARG
    # LDC_ERR_UNSUPPORTED
    assert call(M=1025) == UNSUPPORTED
    assert call(L=65536, L_total=65536, nbytes=1 << 40) == UNSUPPORTED
    assert call(H=4097, W=4096, nbytes=1 << 40) == UNSUPPORTED
    # and the calls that are served
    assert call(nbytes=need) == (0, False)
    assert call(clim=None, clim_slot=None, events=[(1, 1, 0.5, 0)]) == (0, False)
    assert call(mean=mean, std=std) == (0, False)
    # the wrappers
    big = torch.zeros(1025, 1, 1, 2, 4, device="cuda")
    with pytest.raises(ValueError):
        E.rollout_events(big, torch.zeros(1, 1, 2, 4, device="cuda"), torch.ones(2, device="cuda"), as_events([(0, 1, 0.5, 0)]))
    with pytest.raises(RuntimeError):
        E.rollout_events(x.cpu(), t, w, as_events([(0, 1, 0.5, 0)]))  # device tensors only
    bad = hip.events_desc([(0, 1, 0.5, 0)])
    bad.channel[0] = C
    out = E.empty_events(M0, 1, L0, "cuda")
    with pytest.raises(RuntimeError, match="ldc_rollout_events"):
        hip.rollout_events(x, t, slot, None, None, w, bad, *out._buffers, M=M0, C=C, L=L0, H=H0, W=W0, member_stride=x.stride(0), lead_stride=x.stride(2),
                           channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0), L_total=L0)


# ---- h. consistency with the shipped kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 9, 64])
def test_consistent_with_the_exceedance_products(E, M):
    """sum_n n (count_n0 + count_n1) is the number of (member, point) pairs that show the event: M times the sum of ldc_rollout_products'
    exceedance plane #{x_i > thr} / M for the same threshold and direction - an identity on integers, on inputs without NaN"""
    H, W = 3, 50
    c = R.integer_case(M, H, W)
    events = [ev for ev in c["events"] if not ev[3]]
    d = E.rollout_events(c["v"].cuda()[:, :, None], c["t"].cuda()[:, None], c["w"].cuda(), as_events(events))
    n = torch.arange(M + 1).view(1, M + 1, 1)
    pairs = (d["event_hist"][:, 0].cpu().long() * n).sum((-1, -2))
    assert d["event_n_invalid"].cpu().tolist() == [[0]] * len(events)
    for e, (ch, direction, thr, _) in enumerate(events):
        p = E.rollout_products(c["v"].cuda()[:, :, None], thresholds=torch.tensor([[thr]]), threshold_dirs=[direction], channels=[ch], stats=False)
        plane = p["exceed"][0, 0, 0].cpu().double()
        assert int(torch.round(plane * M).sum()) == int(pairs[e]), (e, ch, direction, thr)
        mean_n = float(pairs[e]) / M / (H * W)
        assert abs(float(plane.mean()) - mean_n) <= 1e-6 * max(mean_n, 1e-30)  # fp32 quotients n / M averaged in float64


def test_two_runs_give_the_same_bits(E):
    for c in (R.physical_case(65), R.integer_case(1024, 1, 257)):
        a, b = run_one(E, c), run_one(E, c)
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- i. the driver ---------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
REL = ("ens_var", "ssr", "rank_hist", "rank_hist_weighted", "n_invalid")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double()), torch.nan_to_num(b.double())) \
        and torch.equal(torch.isnan(a.double()), torch.isnan(b.double()))


def test_driver_events():
    from ladcast_amd.evaluate import Event, event_scores, rollout_events
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
    gen = torch.Generator().manual_seed(53)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    latents = torch.randn(ENS, C_LAT, 1 + T, h, w_, generator=gen)
    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = torch.randn(6, C, H, W, generator=gen) * scale + shift
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    clim = torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift
    t_slots, c_slots = [2, 5, 3], [2, 1, 4]
    lat_w = equiangular_lat_weights(H + 1, True)
    # the fields the decoder returns for one lead time's members per call, de-normalised: what the default driver run scores
    fields = []
    for l in range(T):
        y = model.decode(latents[:, :, 1 + l].contiguous().cuda()).sample
        fields.append(inverse_normalize_transform_3D(y.reshape(ENS, C, 1, H, W), mean, std).reshape(ENS, C, H, W))
    phys = torch.stack(fields, 2)  # (ens, C, T, H, W)
    med = [round(float(phys[:, c].median()), 2) for c in range(C)]
    events = [Event(1, "gt", med[1]), Event(1, "lt", med[1] - 0.25), Event(6, "gt", 0.1, True), Event(SST, "gt", med[SST])]
    args = (latents, model, mean, std, truth.cuda(), t_slots, clim.cuda(), c_slots, lat_w)
    kw = dict(sst_channel=SST, crop_init=True, reliability=True)
    plain = EG.score_latent_rollout(*args, **kw)
    got = EG.score_latent_rollout(*args, events=events, **kw)
    assert set(got) == set(plain) | set(EG.EVENTS_KEYS)
    for k in SCORES + REL:  # the scores and the reliability outputs are the bits of a call without events
        assert _same_bits(got[k], plain[k]), k
    assert got["event_hist"].shape == (4, T, ENS + 1, 2) and got["event_hist"].dtype == torch.int32 and got["event_hist"].device.type == "cpu"
    assert got["event_hist_weighted"].dtype == torch.float32 and got["event_n_invalid"].shape == (4, T) and got["event_n_invalid"].dtype == torch.int32
    # the event outputs equal rollout_events on the separately decoded, de-normalised fields, and the oracle on them
    direct = rollout_events(phys, truth.cuda(), lat_w.cuda(), events, clim=clim.cuda(), clim_slots=c_slots, truth_slot=t_slots)
    for k in EG.EVENTS_KEYS:
        assert torch.equal(got[k], direct[k].cpu()), k
    rows = [(e.channel, 1 if e.direction == "gt" else -1, e.threshold, int(e.anomaly)) for e in events]
    for l in range(T):
        ref = R.events_ref(phys[:, :, l].cpu(), truth[t_slots[l]], lat_w, rows, clim[c_slots[l]])
        R.check(dict(hist=got["event_hist"][:, l], hist_w=got["event_hist_weighted"][:, l], n_invalid=got["event_n_invalid"][:, l]), ref, f"lead {l}")
        assert int(ref["n_invalid"][3]) > 0 and int(ref["n_invalid"][0]) == 0  # land: the SST event only
        assert all(0 < int(ref["hist"][e, :, 1].sum()) < H * W for e in range(3))  # both classes occur: the thresholds cut the fields
    # the same result under another decode batch size
    other = EG.score_latent_rollout(*args, events=events, decode_batch_frames=2 * ENS, **kw)
    for k in EG.EVENTS_KEYS:
        assert torch.equal(got[k], other[k]), k
    # columns past the last lead time stay empty; an anomaly event needs the climatology
    wide = EG.score_latent_rollout(*args, events=events, total_num_steps=T + 2, **kw)
    for k in EG.EVENTS_KEYS:
        assert torch.equal(wide[k][:, :T], got[k]) and int(wide[k][:, T:].abs().sum()) == 0, k
    with pytest.raises(ValueError, match="climatology"):
        EG.score_latent_rollout(latents, model, mean, std, truth.cuda(), t_slots, None, None, lat_w, events=events, **kw)
    sc = event_scores(got["event_hist_weighted"].numpy())
    assert sc["brier"].shape == (4, T) and np.isfinite(sc["brier"]).all() and np.isfinite(sc["roc_area"]).all()


def test_command_line_event_flags(tmp_path):
    import json

    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate import event_scores
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.io import save_latent_npy
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]  # frames from 2020-02-27 00 h, 6 h apart: frames 6 and 7; their leads are frames 7 .. 9 and 8 .. 10
    gen = torch.Generator().manual_seed(59)
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
    truth = torch.randn(11, C, H, W, generator=gen) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H, W))  # sparse: zeros
    clim.flush()
    del clim
    thr_t2m, thr_z = round(float(mean[6]), 3), round(float(mean[1]) - 0.1, 3)
    flags = ["--event", "2m_temperature", "gt", str(thr_t2m), "--event_anomaly", "geopotential_level500", "lt", str(thr_z), "--event", "6", "lt", str(thr_t2m)]

    def run(extra, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", *map(str, lv), "--num_atm_vars", "2"] + extra
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, ev = run([], "plain"), run(flags, "events")
    files = ("event_hist", "event_hist_weighted", "event_n_invalid", "event_brier", "event_bss", "event_reliability", "event_resolution",
             "event_uncertainty", "event_roc_area")
    assert sorted(p.name for p in ev.iterdir()) == sorted([p.name for p in plain.iterdir()] + [f"{k}.npy" for k in files] + ["events.json"])
    for p in plain.iterdir():  # the five scores (and the time stamps) bit for bit
        assert (ev / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(ev / f"{k}.npy") for k in files}
    assert a["event_hist"].shape == a["event_hist_weighted"].shape == (3, T, ENS + 1, 2) and a["event_n_invalid"].shape == (2, 3, T)
    assert a["event_hist"].dtype == np.int64 and a["event_hist_weighted"].dtype == np.float64 and a["event_n_invalid"].dtype == np.int32
    meta = json.loads((ev / "events.json").read_text())["events"]
    assert [(m["channel"], m["channel_index"], m["direction"], m["anomaly"]) for m in meta] == [
        ("2m_temperature", 6, "gt", False), ("2m_temperature", 6, "lt", False), ("geopotential_level500", 1, "lt", True)]
    # the oracle on the fields the product decoder returns for the same frame batches, pooled over the two initial times
    rows = [(6, 1, thr_t2m, 0), (6, -1, thr_t2m, 0), (1, -1, thr_z, 1)]
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in mean]), torch.tensor([float(v) for v in std])
    lat_w = EG.lat_weights_for(H)
    shape = (3, T, ENS + 1, 2)
    hist, hist_w, hist_b = torch.zeros(shape, dtype=torch.int64), torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64)
    for n in range(2):
        for l in range(T):
            y = model.decode(latents[n, :, :, 1 + l].contiguous().cuda()).sample
            phys = inverse_normalize_transform_3D(y.reshape(ENS, C, 1, H, W), mean32, std32).reshape(ENS, C, H, W).cpu()
            ref = R.events_ref(phys, truth[6 + n + 1 + l], lat_w, rows, torch.zeros(C, H, W))
            assert a["event_n_invalid"][n, :, l].tolist() == ref["n_invalid"].tolist() == [0, 0, 0]
            hist[:, l] += ref["hist"]
            hist_w[:, l] += ref["hist_w"][0]
            hist_b[:, l] += ref["hist_w"][1]
    assert np.array_equal(a["event_hist"], hist.numpy()) and int(hist.sum()) == 2 * 3 * T * H * W
    R.judge(torch.from_numpy(a["event_hist_weighted"]), (hist_w, hist_b), "event_hist_weighted")
    sc = event_scores(a["event_hist_weighted"])
    for k in ("brier", "bss", "reliability", "resolution", "uncertainty", "roc_area"):
        assert a[f"event_{k}"].shape == (3, T) and a[f"event_{k}"].dtype == np.float64 and np.array_equal(a[f"event_{k}"], sc[k]), k
    assert np.isfinite(a["event_brier"]).all() and np.isfinite(a["event_roc_area"]).all()
