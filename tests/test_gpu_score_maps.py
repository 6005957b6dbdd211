"""The score-map kernel (csrc/score_maps.hip: ldc_rollout_score_maps) through the C ABI and `rollout_score_maps`, against the float64
oracle and the COUNTED bound of tests/score_map_refs.py (judged on the CPU by tests/test_score_maps_cpu.py):
  a. integer-valued tables (every fp32 point value and fp64 sum exact): 8 ensemble sizes x 3 grids, three calls into one buffer, bit for bit
  b. the tie to the shipped kernel: maps of one call, pooled over a region in ldc_rollout_regional's order, give its sums bit for bit
  c. physical scale through the fused inverse normalisation, within the counted bound
  d. the NaN / inf table; without a climatology terms 5 .. 7 and count 2 keep a sentinel pattern
  e. independence of the batching, of the other channels, of the run; the ascending order of the leads of a shared plane
  f. guard bands around both buffers and every input; refused arguments launch nothing
  g. the driver: score_latent_rollout(..., score_maps=...) on the tiny synthetic DC-AE, and the command line"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import regional_refs as R
from tests import score_map_refs as S
from tests.redzone import UNWRITTEN32, UNWRITTEN64, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.score_maps as sm

    return sm


def add_call(E, acc, call, *, frame_major=False, plain=False, l_off=0, leads=None):
    """one CALL of score_map_refs through the wrapper; `plain`: the fields de-normalised first; `leads`: these leads only"""
    sl = slice(None) if leads is None else leads
    kw = {}
    v = call["x"] if plain else call["v"]
    if call["norm"] is not None and not plain:
        kw = dict(mean=call["norm"][0].cuda(), std=call["norm"][1].cuda(), target_std=call["norm"][2])
    xd = v[:, :, sl].cuda()
    if frame_major:
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    cl = None if call["cl"] is None else call["cl"][sl].permute(1, 0, 2, 3).cuda()
    E.rollout_score_maps(xd, call["t"][sl].permute(1, 0, 2, 3).cuda(), acc, clim=cl, l_off=l_off, **kw)


def run_table(E, tab, **kw):
    acc = E.ScoreMaps(tab["channel_idx"], tab["plane_of_lead"], tab["P"])
    for call in tab["calls"]:
        add_call(E, acc, call, **kw)
    return host(acc)


def host(acc):
    sums, counts = acc.download()
    Cm, P = len(acc.channels), acc.n_planes
    assert sums.dtype == np.float64 and counts.dtype == np.int32 and sums.shape == (Cm, P, 8, *acc.grid) and counts.shape == (Cm, P, 3, *acc.grid)
    return dict(sums=torch.from_numpy(sums).reshape(Cm, P, 8, -1), counts=torch.from_numpy(counts).reshape(Cm, P, 3, -1))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64) if a.dtype == torch.float64 else a,
                                                                     b.contiguous().view(torch.int64) if b.dtype == torch.float64 else b)


def same(a, b):
    return same_bits(a["sums"], b["sums"]) and torch.equal(a["counts"], b["counts"])


# ---- a. integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", S.INT_GRIDS)
@pytest.mark.parametrize("M", S.INT_M)
def test_integers_are_exact(E, M, H, W):
    tab = S.integer_table(M, H, W)
    assert tab["channel_idx"] == [1, 0] and tab["plane_of_lead"] == [1, -1, 0, 1] and len(tab["calls"]) == 3
    got, ref = run_table(E, tab), S.maps_ref(tab)
    assert torch.equal(got["counts"].long(), ref["counts"]), (got["counts"].long() != ref["counts"]).nonzero()[:4].tolist()
    bad = (got["sums"] != ref["sums"][0]).nonzero()
    assert bad.numel() == 0, f"M={M} {H}x{W}: sums differ at {bad[:4].tolist()}: {got['sums'][tuple(bad[0])]} vs {ref['sums'][0][tuple(bad[0])]}"
    assert int(ref["counts"][:, 0, 0].min()) == 3 and int(ref["counts"][:, 1, 0].min()) == 6 and int(ref["counts"][:, :, 1].sum()) == 0


# ---- b. the tie to ldc_rollout_regional --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("inv_norm", [True, False])
@pytest.mark.parametrize("M", S.PHYS_M)
def test_maps_pooled_in_regional_order_are_the_regional_sums(E, M, inv_norm, layout):
    """After one call into zeroed maps with one lead per plane every map entry is double(v) of the regional kernel's fp32 point value v
    (0 + v is exact), and w v is exact in fp64: the region's valid points summed in the regional kernel's order - one sequential sum per
    2048-point record, then the records in order (regional_refs._seq_sum) - give ldc_rollout_regional's sums and counts bit for bit."""
    from ladcast_amd.evaluate.regional import rollout_regional

    c = R.physical_case(M)
    tab = S.physical_table(M)
    call, Rn, mask = tab["calls"][1], c["R"], c["mask"]
    fm = layout == "frame_major"
    acc = E.ScoreMaps([0, 1], [0, 1], 2)
    add_call(E, acc, call, frame_major=fm, plain=not inv_norm)
    got = host(acc)
    kw = dict(mean=call["norm"][0].cuda(), std=call["norm"][1].cuda(), target_std=call["norm"][2]) if inv_norm else {}
    xd = (call["v"] if inv_norm else call["x"]).cuda()
    if fm:
        xd, kw["lead_dim"] = xd.permute(2, 0, 1, 3, 4).contiguous(), 0
    d = rollout_regional(xd, call["t"].permute(1, 0, 2, 3).cuda(), c["w"].cuda(), np.asarray(mask), Rn, clim=call["cl"].permute(1, 0, 2, 3).cuda(), **kw)
    rs, rn = d["regional_sums"].cpu(), d["regional_counts"].cpu()
    H, W = c["x"].shape[-2:]
    wp = c["w"].float()[torch.arange(H * W) // W].double().numpy()
    bits = R.region_bits(mask, Rn).numpy()
    sums, counts = got["sums"].numpy(), got["counts"].numpy()
    assert counts.max() == 1 and int(counts[:, :, 1].sum()) == 0
    want_s, want_n = np.zeros((Rn, 2, 2, 10)), np.zeros((Rn, 2, 2, 3), dtype=np.int64)
    for r in range(Rn):
        for ch in range(2):
            for l in range(2):
                ok, ok_a = bits[r] & (counts[ch, l, 0] == 1), bits[r] & (counts[ch, l, 2] == 1)
                want_n[r, ch, l] = [ok.sum(), (bits[r] & (counts[ch, l, 1] == 1)).sum(), ok_a.sum()]
                terms = [np.ones(H * W)] + [sums[ch, l, k] for k in range(5)] + [np.ones(H * W)] + [sums[ch, l, k] for k in range(5, 8)]
                want_s[r, ch, l] = [R._seq_sum(wp * t, ok if k < 6 else ok_a) for k, t in enumerate(terms)]
    assert torch.equal(rn.long(), torch.from_numpy(want_n))
    assert same_bits(rs, torch.from_numpy(want_s)), (rs != torch.from_numpy(want_s)).nonzero()[:4].tolist()
    assert int(want_n[:, :, :, 0].max()) > 100 and float(np.abs(want_s[..., 7]).max()) > 0


# ---- c. physical scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("M", S.PHYS_M)
def test_physical_scale(E, M, shared):
    tab = S.physical_table(M, shared)
    got = run_table(E, tab)
    r = S.check(got, S.maps_ref(tab), f"M={M}")
    print(f"physical M={M} {'one plane' if shared else 'a plane per lead'}: worst err / bound {r:.4f}")
    assert same(run_table(E, tab, plain=True), got)  # the same bits from fields de-normalised first
    assert same(run_table(E, tab, frame_major=True), got)


# ---- d. NaN / inf ----------------------------------------------------------------------------------------------------------------------
def test_nan_inf_table(E):
    tab = S.nan_table()
    got, ref = run_table(E, tab), S.maps_ref(tab)
    r = S.check(got, ref, "nan table")
    print(f"nan table: worst err / bound {r:.4f}")
    n = got["counts"]
    assert bool((n[:, :, 0] + n[:, :, 1] == 4).all()) and int(n[:, :, 1].sum()) > 0 and bool((n[:, :, 2] <= n[:, :, 0]).all()) and bool((n[:, :, 2] < n[:, :, 0]).any())
    assert bool(torch.isinf(got["sums"][:, :, 0]).any()) and bool(torch.isnan(got["sums"][:, :, 2]).any())  # +inf is a value: IEEE sums
    never = n[:, :, 0] == 0
    assert bool(never.any()) and float(got["sums"][:, :, :5].permute(0, 1, 3, 2)[never].abs().sum()) == 0.0  # an invalid sample adds nothing


def test_without_a_climatology_the_acc_terms_keep_their_bits(E):
    tab = S.no_clim_table()
    acc = E.ScoreMaps(tab["channel_idx"], tab["plane_of_lead"], tab["P"])
    add_call(E, acc, tab["calls"][0])
    acc.sums[:, :, 5:].view(torch.int64).fill_(UNWRITTEN64)
    acc.counts[:, :, 2].fill_(UNWRITTEN32)
    add_call(E, acc, tab["calls"][1])
    got = host(acc)
    assert bool((got["sums"][:, :, 5:].contiguous().view(torch.int64) == UNWRITTEN64).all()) and bool((got["counts"][:, :, 2] == UNWRITTEN32).all())
    ref = S.maps_ref(dict(tab, init=None))
    assert torch.equal(got["counts"][:, :, :2].long(), ref["counts"][:, :, :2])
    R.judge(got["sums"][:, :, :5], (ref["sums"][0][:, :, :5], ref["sums"][1][:, :, :5]), "no climatology")


# ---- e. independence, order, repeatability ---------------------------------------------------------------------------------------------
def test_a_plane_holds_the_same_bits_however_the_leads_are_batched(E):
    c = R.physical_case(50)
    call = S.make_call([S.rolled(c, 5 * l) for l in range(4)])
    pol = [1, 0, 1, 1]
    one = E.ScoreMaps([1, 0], pol, 2)
    add_call(E, one, call)
    four = E.ScoreMaps([1, 0], pol, 2)
    for l in range(4):
        add_call(E, four, call, leads=slice(l, l + 1), l_off=l)
    split = E.ScoreMaps([1, 0], pol, 2)
    add_call(E, split, call, leads=slice(0, 3), frame_major=True)
    add_call(E, split, call, leads=slice(3, 4), l_off=3)
    a = host(one)
    assert same(host(four), a) and same(host(split), a) and int(a["counts"][:, 1, 0].min()) == 3


def test_a_channel_alone_gives_the_bits_it_gives_among_others(E):
    c = R.physical_case(24)
    three = {k: torch.cat([c[k], S.rolled(c, 9)[k][..., :1, :, :]], -3) for k in ("x", "t", "cl")}  # a third channel
    call = S.make_call([dict(v=three["x"], x=three["x"], t=three["t"], cl=three["cl"], norm=None)] * 2)
    among = E.ScoreMaps([2, 0, 1], [0, 2], 3)
    add_call(E, among, call)
    alone = E.ScoreMaps([0], [0, 0], 1)
    add_call(E, alone, call, leads=slice(0, 1))
    a, b = host(among), host(alone)
    assert same_bits(a["sums"][1, 0], b["sums"][0, 0]) and torch.equal(a["counts"][1, 0], b["counts"][0, 0])
    assert same_bits(a["sums"][1, 0], a["sums"][1, 2]) and float(a["sums"][:, 1].abs().sum()) == 0.0 and int(a["counts"][:, 1].sum()) == 0


def test_two_runs_give_the_same_bits_and_the_leads_of_a_plane_are_added_in_ascending_order(E):
    for tab in (S.physical_table(64, True), S.nan_table(), S.integer_table(9, 1, 257)):
        assert same(run_table(E, tab), run_table(E, tab))
    assert S.order_ok(run_table(E, S.order_table()))


# ---- f. guard bands, arguments ---------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    t = t.detach().cpu().contiguous()
    return bool((t.view(torch.int64) == UNWRITTEN64).all()) if t.dtype == torch.float64 else bool((t.view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", S.GUARD_CASES)
def test_guard_bands(case, layout):
    from ladcast_amd import hip

    M, C, L, H, W, sst = case
    c = S.guard_case(*case)
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
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    gcs = guarded(1, L, dtype=torch.int32, poison=R.N_CLIM, unwritten=False).fill(torch.tensor(c["c_slots"]))
    chan = [C - 1, sst]  # any order; the SST channel with its land NaNs among them
    pol = [2, 0, 2][:L]  # plane 1 is named by no lead
    Cm, P = len(chan), 3
    gch = guarded(1, Cm, dtype=torch.int32, poison=C, unwritten=False).fill(torch.tensor(chan))
    gpl = guarded(1, L, dtype=torch.int32, poison=P, unwritten=False).fill(torch.tensor(pol))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    gsum, gcnt = guarded(Cm * P * 8, HW, dtype=torch.float64), guarded(Cm * P * 3, HW, dtype=torch.int32)
    sv, nv = gsum.view.view(Cm, P, 8, HW), gcnt.view.view(Cm, P, 3, HW)
    for pl in (0, 2):  # the caller zeroes what it addresses; plane 1 keeps the first bits
        sv[:, pl] = 0
        nv[:, pl] = 0
    assert int(hip.lib.ldc_score_maps_bytes(Cm, P, H, W)) == Cm * P * HW * 76 == gsum.view.numel() * 8 + gcnt.view.numel() * 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert hip.lib.ldc_rollout_score_maps(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gc.view), gc.bs, ld,
                                          _p(gcs.view), _p(gch.view), Cm, _p(gpl.view), P, M, C, L, H, W, _p(gsum.view), _p(gcnt.view), stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, clim=gc, truth_slot=gts, clim_slot=gcs, channel_idx=gch, plane_of_lead=gpl, mean=gm, std=gs, sums=gsum,
                     counts=gcnt).items():
        assert_untouched(g, k)
    sums, counts = gsum.payload().reshape(Cm, P, 8, HW), gcnt.payload().reshape(Cm, P, 3, HW)
    assert _unwritten(sums[:, 1]) and _unwritten(counts[:, 1])
    xp = S.inv_norm_f32(c["x"], mean, std, ts)
    call = dict(v=xp, x=xp, norm=None, t=torch.stack([c["truth_table"][s] for s in c["t_slots"]]), cl=torch.stack([c["clim_table"][s] for s in c["c_slots"]]))
    ref = S.maps_ref(dict(calls=[call], channel_idx=chan, plane_of_lead=pol, P=P, init=None))
    keep = [0, 2]
    r = S.check(dict(sums=sums[:, keep], counts=counts[:, keep]), dict(sums=(ref["sums"][0][:, keep], ref["sums"][1][:, keep]), counts=ref["counts"][:, keep]),
                f"{case} {layout}")
    print(f"guard bands {case} {layout}: worst err / bound {r:.4f}")
    assert int(ref["counts"][chan.index(sst), :, 1].sum()) > 0  # the land points of the SST channel are counted as invalid


def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M0, C, L0, H0, W0, Cm0, P0 = 5, 2, 2, 4, 8, 2, 2
    x, t = torch.zeros(M0, C, L0, H0, W0, device="cuda"), torch.zeros(C, L0, H0, W0, device="cuda")
    cl = torch.zeros(C, L0, H0, W0, device="cuda")
    slot = torch.arange(L0, dtype=torch.int32, device="cuda")
    chan, pol = torch.tensor([1, 0], dtype=torch.int32, device="cuda"), torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    mean, std = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(M=M0, L=L0, H=H0, W=W0, Cn=C, Cm=Cm0, P=P0, forecast=x, truth=t, truth_slot=slot, clim=cl, clim_slot=slot, mean=None, std=None, channel_idx=chan,
             plane_of_lead=pol, sums=True, counts=True, sums_off=0):
        gs, gn = guarded(Cm0 * P0 * 8, H0 * W0, dtype=torch.float64), guarded(Cm0 * P0 * 3, H0 * W0, dtype=torch.int32)
        q = lambda v: None if v is None else _p(v)  # noqa: E731
        st = hip.lib.ldc_rollout_score_maps(q(forecast), x.stride(0), x.stride(2), x.stride(1), q(mean), q(std), 1.0, q(truth), t.stride(1), t.stride(0),
                                            q(truth_slot), q(clim), cl.stride(1), cl.stride(0), q(clim_slot), q(channel_idx), Cm, q(plane_of_lead), P, M, Cn, L, H,
                                            W, ctypes.c_void_p(gs.view.data_ptr() + sums_off) if sums else None, _p(gn.view) if counts else None, stream)
        torch.cuda.synchronize()
        untouched = _unwritten(gn.payload()) and _unwritten(gs.payload())
        for g in (gs, gn):
            assert_untouched(g)
        return st, untouched

    ARG, UNSUPPORTED, ALIGN = (-1, True), (-3, True), (-2, True)
    for kw in (dict(forecast=None), dict(truth=None), dict(truth_slot=None), dict(channel_idx=None), dict(plane_of_lead=None), dict(sums=False), dict(counts=False),
               dict(M=0), dict(M=-3), dict(Cn=0), dict(L=0), dict(H=0), dict(W=0), dict(Cm=0), dict(Cm=-1), dict(P=0), dict(P=-2), dict(mean=mean), dict(clim_slot=None)):
        assert call(**kw) == ARG, kw
    for kw in (dict(M=65), dict(Cm=65536), dict(P=65536), dict(H=4097, W=4096)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(sums_off=4) == ALIGN  # fp64 sums that are not 8-byte aligned
    # and the calls that are served: they write (an UNWRITTEN NaN plus a value stays a NaN, but no longer that pattern's payload in the counts)
    assert call()[0] == 0 and not call()[1]
    assert call(clim=None, clim_slot=None)[0] == 0 and call(mean=mean, std=std)[0] == 0
    # the wrapper checks what the kernel leaves to the caller, on the host
    acc = E.ScoreMaps([0, 2], [0, 1], 2)
    with pytest.raises(ValueError, match="channels"):
        E.rollout_score_maps(x, t, acc)
    acc = E.ScoreMaps([0], [0], 1)
    with pytest.raises(ValueError, match="plane_of_lead"):
        E.rollout_score_maps(x, t, acc)  # two leads, one entry
    with pytest.raises(ValueError):
        E.rollout_score_maps(torch.zeros(65, 1, 1, 2, 4, device="cuda"), torch.zeros(1, 1, 2, 4, device="cuda"), acc)
    with pytest.raises(RuntimeError):
        E.rollout_score_maps(x.cpu(), t, E.ScoreMaps([0], [0, 0], 1))  # device tensors only
    assert acc.sums is None
    acc = E.ScoreMaps([0], [0, 0], 1)
    E.rollout_score_maps(x, t, acc)
    with pytest.raises(ValueError, match="members"):
        E.rollout_score_maps(x[:3], t, acc)  # one accumulator, one ensemble size
    with pytest.raises(RuntimeError, match="ldc_rollout_score_maps"):
        hip.rollout_score_maps(x, t, slot, None, None, chan, pol, acc.sums, acc.counts, Cm=65536, P=1, M=M0, C=C, L=L0, H=H0, W=W0, member_stride=x.stride(0),
                               lead_stride=x.stride(2), channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0))


# ---- g. the driver ---------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.double()), torch.nan_to_num(b.double())) \
        and torch.equal(torch.isnan(a.double()), torch.isnan(b.double()))


def test_driver_score_maps(E):
    from ladcast_amd.evaluate import NAMED_REGIONS, region_mask
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.evaluate_encdec_model import equiangular_lat_weights
    from ladcast_amd.models import AutoencoderDC
    from tests.synth import make_dcae, tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 3, 8, 3, 6, 8, 8, 48, 64, 3
    cfg = tiny_dcae_config()
    model = AutoencoderDC.from_config(cfg)
    model.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    model = model.cuda().eval()
    gen = torch.Generator().manual_seed(131)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    inits = [torch.randn(ENS, C_LAT, 1 + T, h, w_, generator=gen) for _ in range(2)]
    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = (torch.randn(7, C, H, W, generator=gen) * scale + shift)
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    truth, clim = truth.cuda(), (torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift).cuda()
    slots = [([2, 5, 3], [2, 1, 4]), ([3, 6, 4], [0, 3, 1])]
    lat_w = equiangular_lat_weights(H + 1, True)
    chans, pol = [5, SST, 0], [0, 1, 2]
    regions = [NAMED_REGIONS["global"], NAMED_REGIONS["tropics"], NAMED_REGIONS["europe"]]
    kw = dict(sst_channel=SST, crop_init=True, regions=regions)
    pooled = {}
    for dbf in (3, 6):
        acc, direct = E.ScoreMaps(chans, pol, 3), E.ScoreMaps(chans, pol, 3)
        per = dbf // ENS
        for lat, (ts, cs) in zip(inits, slots):
            args = (lat, model, mean, std, truth, ts, clim, cs, lat_w)
            plain = EG.score_latent_rollout(*args, decode_batch_frames=dbf, **kw)
            got = EG.score_latent_rollout(*args, decode_batch_frames=dbf, score_maps=acc, **kw)
            assert set(got) == set(plain)  # the result gains no key
            for k in plain:  # and every other output is the bits of the call without maps
                assert _same(got[k], plain[k]), k
            for s0 in range(0, T, per):  # direct calls on the frames as this batching decodes them
                nl = min(per, T - s0)
                x = lat[:, :, 1 + s0 : 1 + s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ENS, C_LAT, h, w_).contiguous().cuda()
                y = model.decode(x).sample.reshape(nl, ENS, C, H, W)
                E.rollout_score_maps(y, truth, direct, clim=clim, clim_slots=cs[s0 : s0 + nl], truth_slot=ts[s0 : s0 + nl], lead_dim=0, mean=mean.cuda(), std=std.cuda(),
                                     l_off=s0)
            for k in EG.REGIONAL_KEYS:
                pooled[(dbf, k)] = pooled.get((dbf, k), 0) + got[k].double().numpy()
        assert acc.n_init == 2 and acc.members == ENS and direct.n_init == 0
        a, b = host(acc), host(direct)
        assert same(a, b)
        n = a["counts"]
        assert bool((n[0, :, 0] == 2).all()) and int(n[1, :, 1].min()) in (0, 2) and int(n[1, :, 1].sum()) > 0 and bool((n[:, :, 0] + n[:, :, 1] == 2).all())
        # regional_from_maps against the pooled regional sums of the same calls: both sides sum the same exact products w v, in another
        # grouping.  Additions: the kernel's per call (points of the region + its records), the host's one per call; on the map side two per
        # point and the points of the region.  sum |w v| of every sum is at most S0 + S2 + 2 S3 + S8 + S9 (tests/test_gpu_regional.py).
        mask = region_mask(regions, EG.row_latitudes(H), np.arange(W) * (360.0 / W))
        sums, counts = acc.download()
        rs, rn = E.regional_from_maps(sums, counts, lat_w, mask, len(regions))
        assert rs.shape == (3, 3, 3, 10) and rn.shape == (3, 3, 3, 3)
        ps, pn = pooled[(dbf, "regional_sums")][:, chans], pooled[(dbf, "regional_counts")][:, chans]
        assert np.array_equal(rn, pn.astype(np.int64))
        n_add = 2 * (H * W + R.n_records(H * W) + 1) + 3 * H * W
        bound = n_add * 2.0 ** -53 * (ps[..., 0] + ps[..., 2] + 2 * ps[..., 3] + ps[..., 8] + ps[..., 9])[..., None]
        err = np.abs(rs - ps)
        print(f"decode_batch_frames={dbf}: regional_from_maps worst err / bound {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert bool((err <= bound).all())
    assert acc.grid == (H, W)


def test_command_line_map_flags(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.score_maps import MAP_COUNT_NAMES, SCORE_MAP_NAMES, TERM_NAMES, score_maps
    from ladcast_amd.evaluate.validate_AR import column_names
    from ladcast_amd.pipelines.io import save_latent_npy
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]
    gen = torch.Generator().manual_seed(137)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    lv = (300, 500, 850)
    norm = {"geopotential": {"mean": {str(p): float(mean[i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {str(p): float(mean[3 + i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(mean[6]), "std": float(std[6])}, "sea_surface_temperature": {"mean": float(mean[7]), "std": float(std[7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    save_latent_npy(torch.randn(2, ENS, C_LAT, 1 + T, h, w_, generator=gen), inits, str(tmp_path / "rollout"))
    truth = torch.randn(11, C, H + 1, W, generator=gen) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)  # with the south pole row
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H + 1, W))  # sparse: zeros
    clim.flush()
    del clim
    chan_names = column_names(names, list(lv), 2)
    flags = ["--map", chan_names[7], "0", "--map_lead_bins", "6-12", "18-18"]

    def run(extra, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", *map(str, lv), "--num_atm_vars", "2"] + extra
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, maps = run([], "plain"), run(flags, "maps")
    new = ["score_map_sums.npy", "score_map_counts.npy", "score_maps.json"] + [f"score_map_{k}.npy" for k in SCORE_MAP_NAMES]
    assert not [p.name for p in plain.iterdir() if p.name.startswith("score_map")]  # a run without --map writes none of them
    assert sorted(p.name for p in maps.iterdir()) == sorted([p.name for p in plain.iterdir()] + new)
    for p in plain.iterdir():  # every other file bit for bit
        assert (maps / p.name).read_bytes() == p.read_bytes(), p.name
    s, n = np.load(maps / "score_map_sums.npy"), np.load(maps / "score_map_counts.npy")
    assert s.shape == (2, 2, 8, H, W) and s.dtype == np.float64 and n.shape == (2, 2, 3, H, W) and n.dtype == np.int32
    assert (n[:, 0, 0] == 4).all() and (n[:, 1, 0] == 2).all() and (n[:, :, 1] == 0).all()  # two initial times; plane 0 pools two leads
    sc = score_maps(s, n, ENS)
    for k in SCORE_MAP_NAMES:
        f = np.load(maps / f"score_map_{k}.npy")
        assert f.shape == (2, 2, H, W) and np.array_equal(f, sc[k], equal_nan=True), k
    assert np.isfinite(np.load(maps / "score_map_rmse.npy")).all() and np.isfinite(np.load(maps / "score_map_ens_acc.npy")).all()
    meta = json.loads((maps / "score_maps.json").read_text())
    assert meta["channels"] == [chan_names[7], chan_names[0]] and meta["channel_indices"] == [7, 0] and meta["members"] == ENS and meta["n_init"] == 2
    assert [p["lead_hours"] for p in meta["planes"]] == [[6, 12], [18]] and meta["plane_of_lead"] == [0, 0, 1]
    assert meta["terms"] == list(TERM_NAMES) and meta["counts"] == list(MAP_COUNT_NAMES)
    with pytest.raises(ValueError, match="map_max_gib"):  # the guard refuses before anything is decoded
        run(flags + ["--map_max_gib", "0.0001"], "refused")
