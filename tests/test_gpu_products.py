"""The ensemble-products kernel (csrc/products.hip: ldc_rollout_products) through the C ABI and `rollout_products`, against the float64
oracle and the COUNTED bounds of tests/products_refs.py (judged on the CPU by tests/test_products_cpu.py).  Common shapes: C = 3, L = 2
written at l_off = 1 of L_total = 4; (H, W) = (3, 70), one partial workgroup, and (3, 86), two workgroups with a ragged tail.
  a. small integers, M at both ends of every register arm: mean / min / max / exceed / t == 0 quantiles exact, the rest within the bound
  b. the streaming arm, M = 65, 100, 1024, without quantiles; with quantiles: refused, buffers untouched
  c. order and ties: duplicates, -0 / +0, +-inf members
  d. physical scale through the fused inverse normalisation: target_std, both layouts, strided members and channels, channels = [2, 0]
  e. the NaN table
  f. guard bands around every buffer, columns outside l_off .. l_off + L - 1 untouched, outputs passed as None
  g. refused arguments launch nothing
  h. the driver on the tiny synthetic DC-AE"""
import ctypes

import pytest
import torch

from tests import products_refs as R
from tests.redzone import UNWRITTEN32, assert_untouched, guarded
from tests.score_edge_refs import FLT_MAX_BITS

pytestmark = pytest.mark.gpu
C, L, L_OFF, LT = R.C, R.L, R.L_OFF, R.L_TOTAL


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    return eu


def run(E, x, quantiles=(), thr=None, dirs=None, *, channels=None, what="", **kw):
    """x (M, C, L, H, W) on the host (or a device view with `lead_dim` in kw) -> the result written at l_off = 1 of L_total = 4, with the
    columns outside checked to be the NaN of a fresh result"""
    xd = x if x.is_cuda else x.cuda()
    H, W = xd.shape[-2:]
    Cs = C if channels is None else len(channels)
    out = E.empty_products(Cs, LT, H, W, "cuda", n_quantiles=len(quantiles), n_thresholds=0 if thr is None else thr.shape[0])
    d = E.rollout_products(xd, quantiles=quantiles, thresholds=thr, threshold_dirs=dirs, channels=channels, out=out, l_off=L_OFF, **kw)
    assert isinstance(d, E.ProductsDict) and all(v.dtype == torch.float32 and v.is_cuda for v in d.values())
    for k, v in d.items():
        lead_axis = 1 if k in R.STAT_NAMES else 2
        assert v.shape[lead_axis] == LT and v.shape[lead_axis - 1] == Cs
        for col in (0, LT - 1):
            assert bool(torch.isnan(v.select(lead_axis, col)).all()), f"{what}: column {col} of {k} was written"
    return d


def check_leads(d, x, quantiles, thr, dirs, what, channels=None):
    worst = 0.0
    for l in range(L):
        worst = max(worst, R.check(R.column(d, L_OFF + l), R.ref_of(x, l, quantiles, thr, dirs, channels), f"{what} lead {l}"))
    return worst


def exact_mean(d, x, what):
    for l in range(L):
        want = R.ref_of(x, l, (), None, ())["mean"][0].float()
        assert R.same_value_bits(d["mean"][:, L_OFF + l], want), f"{what} lead {l}: the mean is not the float64 value rounded once"


# ---- a. small integers, the register arms ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.REGISTER_M)
def test_integers_register_arms(E, M):
    for H, W in R.SHAPES:
        c = R.integer_case(M, H, W)
        what = f"M={M} {H}x{W}"
        d = run(E, c["x"], R.QUANTILES, c["thr"], c["dirs"], what=what)
        r = check_leads(d, c["x"], R.QUANTILES, c["thr"], c["dirs"], what)
        print(f"integers {what}: worst err / bound {r:.4f}")
        exact_mean(d, c["x"], what)
        assert bool(torch.isnan(d["std"][:, L_OFF:L_OFF + L]).all()) == (M == 1)
        assert bool(torch.isfinite(d["mean"][:, L_OFF:L_OFF + L]).all())


# ---- b. the streaming arm ------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("M", R.STREAM_M)
def test_streaming_arm(E, M):
    from ladcast_amd import hip

    for H, W in R.SHAPES:
        c = R.integer_case(M, H, W)
        what = f"M={M} {H}x{W}"
        d = run(E, c["x"], (), c["thr"], c["dirs"], what=what)
        assert "quantiles" not in d
        r = check_leads(d, c["x"], (), c["thr"], c["dirs"], what)
        print(f"streaming {what}: worst err / bound {r:.4f}")
        exact_mean(d, c["x"], what)
    # with quantiles: refused by the host and by the library, nothing written
    xd = c["x"].cuda()
    with pytest.raises(ValueError):
        E.rollout_products(xd, quantiles=[0.5])
    HW = H * W
    gs, gq, ge = guarded(4 * C * L, HW), guarded(1 * C * L, HW), guarded(3 * C * L, HW)
    desc = hip.products_desc([0.5], 64, c["dirs"])  # a descriptor that is valid on its own
    thr_d = c["thr"].cuda()
    st = hip.lib.ldc_rollout_products(_p(xd), xd.stride(0), xd.stride(2), xd.stride(1), None, None, 1.0, None, M, C, C, L, H, W, ctypes.byref(desc),
                                      _p(thr_d), _p(gs.view), _p(gq.view), _p(ge.view), L, 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == -3  # LDC_ERR_UNSUPPORTED
    for g in (gs, gq, ge):
        assert_untouched(g)
        assert _unwritten(g.payload())


# ---- c. order and ties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("M", [4, 9, 64])
def test_order_and_ties(E, M, with_inf):
    H, W = R.SHAPES[1]
    c = R.ties_case(M, H, W, with_inf)
    x, thr, dirs = c["x"], c["thr"], c["dirs"]
    what = f"ties M={M} inf={with_inf}"
    d = run(E, x, R.QUANTILES, thr, dirs, what=what)
    check_leads(d, x, R.QUANTILES, thr, dirs, what)
    sl = slice(L_OFF, L_OFF + L)
    q, ex = d["quantiles"][:, :, sl].cpu(), d["exceed"][:, :, sl].cpu()
    # q = 0 and q = 1 are the bits of min and max
    assert torch.equal(q[0].view(torch.int32), d["min"][:, sl].cpu().view(torch.int32))
    assert torch.equal(q[-1].view(torch.int32), d["max"][:, sl].cpu().view(torch.int32))
    # non-decreasing in q (where both are numbers: an interpolation between -inf and a number, or between two +inf, is NaN by IEEE)
    for a, b in zip(q[:-1], q[1:]):
        ok = ~torch.isnan(a) & ~torch.isnan(b)
        assert bool((a[ok] <= b[ok]).all())
    if not with_inf:
        assert not bool(torch.isnan(q).any())
    # exceed(>) + exceed(<) + ties / M == 1 for the thresholds 0.25 / 0 / 2 (planes 0 and 1 hold the same table), stated in counts:
    # k / M is not a binary fraction for every M, so the three fp32 quotients are turned back into the integers they were formed from
    xs = x.float()
    ties = (xs == thr[0].view(1, C, 1, 1, 1)).sum(0)
    above, below = (ex[0] * M).round().long(), (ex[1] * M).round().long()
    assert R.equal_by_value(ex[0], above.float() / M) and R.equal_by_value(ex[1], below.float() / M)
    assert torch.equal(above + below + ties, torch.full_like(ties, M))
    # a threshold of -inf gives 1 (no member is -inf where it is counted) and of +inf gives 0
    no_minf = ~(xs == float("-inf")).any(0)
    assert bool((ex[2][no_minf] == 1.0).all()) and bool((ex[3] == 0.0).all())
    if with_inf:
        assert bool((ex[2][~no_minf] == (M - 1) / M).all()) and bool(torch.isinf(d["min"][:, sl]).any()) and bool(torch.isinf(d["max"][:, sl]).any())
    # -0 / +0 are one value: the median of a point whose members are all zeros of either sign is a zero
    z = torch.where(torch.rand(M, C, L, H, W, generator=R.gen(3)) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    dz = run(E, z, (0.0, 0.5, 1.0), what="zeros")
    for k in ("mean", "min", "max"):
        assert bool((dz[k][:, sl] == 0).all())
    assert bool((dz["quantiles"][:, :, sl] == 0).all()) and bool((dz["std"][:, sl] == 0).all())


# ---- d. physical scale ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target_std", [1.0, 0.5])
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M, target_std):
    H, W = R.SHAPES[1]
    c = R.physical_case(M, H, W)
    v, mean, std = c["v"], c["mean"], c["std"]
    x = R.inv_norm_f32(v, mean, std, target_std)
    md, sd = mean.cuda(), std.cuda()
    kw = dict(mean=md, std=sd, target_std=target_std)
    results = {}
    for channels in (None, [2, 0]):
        thr, dirs = R.phys_thresholds(channels or (0, 1, 2))
        what = f"physical M={M} target_std={target_std} channels={channels}"
        d = run(E, v, R.QUANTILES, thr, dirs, channels=channels, what=what, **kw)
        r = check_leads(d, x, R.QUANTILES, thr, dirs, what, channels)
        print(f"{what}: worst err / bound {r:.4f}")
        # the decoder's frame-major layout, and a forecast with strided members and channels: the same bits
        frames = v.cuda().permute(2, 0, 1, 3, 4).contiguous()
        wide = torch.full((2 * M, C + 2, L, H, W), float("nan"), device="cuda")
        wide[::2, 1:C + 1] = v.cuda()
        strided = wide[::2, 1:C + 1]
        assert not strided.is_contiguous() and strided.stride(0) == 2 * (C + 2) * L * H * W
        for other, okw in ((frames, dict(lead_dim=0)), (strided, {})):
            d2 = run(E, other, R.QUANTILES, thr, dirs, channels=channels, what=what, **kw, **okw)
            for k in d:
                assert R.same_value_bits(d[k], d2[k]), (what, k, okw)
        results[str(channels)] = d
    # channels = [2, 0]: the subset, in list order, with mean / std / thr of the right channel
    full, sub = results["None"], results["[2, 0]"]
    for k in R.STAT_NAMES:
        assert R.same_value_bits(sub[k], full[k][[2, 0]]), k
    assert R.same_value_bits(sub["quantiles"], full["quantiles"][:, [2, 0]])
    sl = slice(L_OFF, L_OFF + L)
    assert R.same_value_bits(sub["exceed"][0, 1], full["exceed"][0, 0]) and bool(torch.isnan(sub["exceed"][0, 0]).all())  # 303.15 K on channel 0
    assert bool(torch.isnan(sub["exceed"][1]).all())  # the pressure threshold's channel is not selected
    assert bool(torch.isfinite(full["exceed"][1, 1][sl]).all()) and bool(torch.isnan(full["exceed"][1, 0]).all())


# ---- e. the NaN table ----------------------------------------------------------------------------------------------------------------------------
def test_nan_table(E):
    for H, W in R.SHAPES:
        c = R.nan_case(H, W)
        d = run(E, c["x"], R.QUANTILES, c["thr"], c["dirs"], what="NaN table")
        check_leads(d, c["x"], R.QUANTILES, c["thr"], c["dirs"], f"NaN table {H}x{W}")
        h, w = c["point"]
        sl = slice(L_OFF, L_OFF + L)
        for k in R.STAT_NAMES:
            nan = torch.isnan(d[k][:, sl])
            assert int(nan.sum()) == C * L and bool(nan[:, :, h, w].all()), k
        nan = torch.isnan(d["quantiles"][:, :, sl])
        assert int(nan.sum()) == len(R.QUANTILES) * C * L and bool(nan[..., h, w].all())
        p, ch = c["nan_thr"]
        nan = torch.isnan(d["exceed"][:, :, sl])
        assert bool(nan[p, ch].all()) and bool(nan[..., h, w].all()) and int(nan.sum()) == L * (H * W + len(c["dirs"]) * C - 1)


# ---- f. guard bands ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", ["all", "no_stats", "only_stats", "only_exceed"])
@pytest.mark.parametrize("M,layout", [(9, "ens_C_L_H_W"), (50, "frame_major"), (100, "ens_C_L_H_W")])
def test_guard_bands(M, layout, outputs):
    from ladcast_amd import hip

    H, W = R.SHAPES[1]
    HW, ld = H * W, H * W + 8
    c = R.physical_case(M, H, W)
    v = c["v"]
    chans = [2, 0]
    Cs = len(chans)
    quantiles = R.QUANTILES if M <= 64 else ()
    Q = len(quantiles)
    thr, dirs = R.phys_thresholds(chans)
    P = len(dirs)
    inp = dict(poison=FLT_MAX_BITS, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(v.reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(v.permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gm, gsd = guarded(1, C, **inp).fill(c["mean"]), guarded(1, C, **inp).fill(c["std"])
    gc = guarded(1, Cs, dtype=torch.int32, poison=0, unwritten=False).fill(torch.tensor(chans))
    gt = guarded(P, Cs, **inp).fill(thr)
    want_s, want_q, want_e = outputs in ("all", "only_stats"), outputs in ("all", "no_stats") and Q > 0, outputs in ("all", "no_stats", "only_exceed")
    assert want_s or want_e  # every case asks for an output that every ensemble size serves
    gs, gq, ge = guarded(4 * Cs * LT, HW), guarded(max(Q, 1) * Cs * LT, HW), guarded(P * Cs * LT, HW)
    desc = hip.products_desc(quantiles, M, dirs)
    st = hip.lib.ldc_rollout_products(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gsd.view), 0.5, _p(gc.view), M, C, Cs, L, H, W, ctypes.byref(desc),
                                      _p(gt.view), _p(gs.view) if want_s else None, _p(gq.view) if want_q else None, _p(ge.view) if want_e else None,
                                      LT, L_OFF, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    for k, g in dict(forecast=gf, mean=gm, std=gsd, channels=gc, thr=gt, stats=gs, quant=gq, exceed=ge).items():
        assert_untouched(g, k)
    stats, quant, exceed = gs.payload()[0].reshape(4, Cs, LT, H, W), gq.payload()[0].reshape(max(Q, 1), Cs, LT, H, W), ge.payload()[0].reshape(P, Cs, LT, H, W)
    for buf, want in ((stats, want_s), (quant, want_q), (exceed, want_e)):
        if not want:
            assert _unwritten(buf)  # an output that was not asked for is not written
            continue
        for col in (0, LT - 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
            assert _unwritten(buf[:, :, col])
        assert not bool((buf[:, :, L_OFF:L_OFF + L].contiguous().view(torch.int32) == UNWRITTEN32).any())
    x = R.inv_norm_f32(v, c["mean"], c["std"], 0.5)
    for l in range(L):
        got = {}
        if want_s:
            got.update({k: stats[i, :, L_OFF + l] for i, k in enumerate(R.STAT_NAMES)})
        ref = R.ref_of(x, l, quantiles if want_q else (), thr if want_e else None, dirs if want_e else (), chans)
        if want_q:
            got["quantiles"] = quant[:, :, L_OFF + l]
        if want_e:
            got["exceed"] = exceed[:, :, L_OFF + l]
        R.check(got, ref, f"guard bands M={M} {layout} {outputs} lead {l}")


def test_stats_false_and_missing_outputs(E):
    H, W = R.SHAPES[0]
    c = R.integer_case(17, H, W)
    full = run(E, c["x"], R.QUANTILES, c["thr"], c["dirs"])
    d = E.rollout_products(c["x"].cuda(), quantiles=R.QUANTILES, thresholds=c["thr"], threshold_dirs=c["dirs"], stats=False, l_off=L_OFF)
    assert sorted(d) == ["exceed", "quantiles"] and d["quantiles"].shape == (len(R.QUANTILES), C, L_OFF + L, H, W)
    assert bool(torch.isnan(d["quantiles"][:, :, 0]).all())  # a fresh result is NaN where nothing was written
    for k in d:
        assert R.same_value_bits(d[k][:, :, L_OFF:], full[k][:, :, L_OFF:L_OFF + L]), k
    d = E.rollout_products(c["x"].cuda(), thresholds=c["thr"], threshold_dirs=c["dirs"], stats=False)
    assert sorted(d) == ["exceed"] and R.same_value_bits(d["exceed"], full["exceed"][:, :, L_OFF:L_OFF + L])
    d = E.rollout_products(c["x"].cuda())
    assert sorted(d) == sorted(R.STAT_NAMES) and all(R.same_value_bits(d[k], full[k][:, L_OFF:L_OFF + L]) for k in d)


# ---- g. refused arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    M, H, W = 5, 4, 8
    HW = H * W
    x = torch.zeros(M, C, L, H, W, device="cuda")
    thr = torch.zeros(8, C, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def desc(Q=2, P=2, direction=1, lo=None, t=None):
        d = hip.ProductsDesc()
        d.n_quant, d.n_thr = Q, P
        for k in range(16):
            d.q_lo[k], d.q_t[k] = (k % M if lo is None else lo), (0.5 if t is None else t)
        for k in range(8):
            d.thr_dir[k] = direction
        return d

    def call(d, M=M, forecast=x, L_total=LT, l_off=L_OFF, Cs=C, channels=None, thr=thr, outputs=True):
        gs, gq, ge = guarded(4 * C * LT, HW), guarded(16 * C * LT, HW), guarded(8 * C * LT, HW)
        st = hip.lib.ldc_rollout_products(_p(forecast), x.stride(0), x.stride(2), x.stride(1), None, None, 1.0, _p(channels), M, C, Cs, L, H, W,
                                          None if d is None else ctypes.byref(d), _p(thr), _p(gs.view) if outputs else None,
                                          _p(gq.view) if outputs else None, _p(ge.view) if outputs else None, L_total, l_off, stream)
        torch.cuda.synchronize()
        untouched = all(_unwritten(g.payload()) for g in (gs, gq, ge))
        for g in (gs, gq, ge):
            assert_untouched(g)
        return st, untouched

    assert call(desc()) == (0, False)
    assert call(desc(), M=0) == (-1, True)  # LDC_ERR_ARG
    assert call(desc(), M=-2) == (-1, True)
    assert call(desc(Q=17)) == (-1, True)
    assert call(desc(P=9)) == (-1, True)
    assert call(desc(Q=-1)) == (-1, True)
    assert call(desc(), l_off=LT - L + 1) == (-1, True)  # l_off + L > L_total
    assert call(desc(), l_off=-1) == (-1, True)
    assert call(desc(direction=0)) == (-1, True)
    assert call(desc(direction=2)) == (-1, True)
    assert call(desc(), forecast=None) == (-1, True)
    assert call(None) == (-1, True)
    assert call(desc(lo=M)) == (-1, True)  # an order statistic that does not exist
    assert call(desc(t=float("nan"))) == (-1, True)
    assert call(desc(t=1.5)) == (-1, True)
    assert call(desc(), Cs=2) == (-1, True)  # all channels, yet not C of them
    assert call(desc(), thr=None) == (-1, True)
    assert call(desc(), outputs=False) == (-1, True)  # nothing to compute
    assert call(desc(), M=1025) == (-3, True)  # LDC_ERR_UNSUPPORTED
    assert call(desc(lo=0), M=65) == (-3, True)
    with pytest.raises(RuntimeError, match="ldc_rollout_products"):
        hip.rollout_products(x, desc(P=9), M=M, C=C, L=L, H=H, W=W, member_stride=x.stride(0), lead_stride=x.stride(2), channel_stride=x.stride(1),
                             stats=torch.empty(4, C, L, H, W, device="cuda"), L_total=L)
    with pytest.raises(RuntimeError):
        E.rollout_products(x.cpu())  # device tensors only


# ---- h. the driver -------------------------------------------------------------------------------------------------------------------------------
ENS, C_LAT, T, CHANS, DRIVER_Q, DRIVER_DIRS = 6, 8, 3, [5, 0, 3], (0.1, 0.5, 0.9), (1, -1)


@pytest.fixture(scope="module")
def driver():
    """the tiny synthetic DC-AE, latents with the initial condition in slot 0, and the products of the default decode batch (one lead time
    per decode batch) and of one decode batch for all lead times"""
    from ladcast_amd.evaluate.products import products_of_latent_rollout
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.utils import decode_latent_ens
    from tests.synth import tiny_dcae_config

    gen = torch.Generator().manual_seed(53)
    torch.manual_seed(4321)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    latents = torch.randn(ENS, C_LAT, 1 + T, 6, 8, generator=gen)
    mean, std = torch.randn(8, generator=gen) * 50 + 200, torch.rand(8, generator=gen) * 20 + 5
    # the fields of every slot, each lead time's members decoded by one decoder call as the driver's default batch decodes them
    fields = torch.cat([decode_latent_ens(model, latents[:, :, l:l + 1], mean, std).cpu() for l in range(1 + T)], dim=2)  # (ENS, C', 1 + T, H, W)
    thr = torch.full((2, len(CHANS)), float("nan"))
    thr[0, 0], thr[1, 2] = float(fields[:, 5].median()), float(fields[:, 3].median())
    kw = dict(quantiles=DRIVER_Q, thresholds=thr, threshold_dirs=DRIVER_DIRS, channels=CHANS)
    one = products_of_latent_rollout(latents, model, mean, std, total_num_steps=T + 1, crop_init=True, **kw)
    every = products_of_latent_rollout(latents, model, mean, std, total_num_steps=T + 1, crop_init=True, decode_batch_frames=T * ENS, **kw)
    return dict(model=model, latents=latents, mean=mean, std=std, fields=fields, thr=thr, kw=kw, one=one, every=every)


def test_driver_on_the_synthetic_dcae(driver):
    from ladcast_amd.evaluate.products import products_of_latent_rollout
    from ladcast_amd.pipelines.utils import decode_latent_ens

    s = driver
    one, every, fields, thr = s["one"], s["every"], s["fields"], s["thr"]
    H, W = fields.shape[-2:]
    for res in (one, every):
        assert sorted(res) == ["exceed", "max", "mean", "min", "quantiles", "std"] and all(not v.is_cuda and v.dtype == torch.float32 for v in res.values())
        assert res["mean"].shape == (3, T + 1, H, W) and res["quantiles"].shape == (3, 3, T + 1, H, W) and res["exceed"].shape == (2, 3, T + 1, H, W)
        for k in res:
            assert bool(torch.isnan(res[k].select(1 if k in R.STAT_NAMES else 2, T)).all())  # the column past the last lead time stays NaN
    # the default decode batch against the oracle on decode_latent_ens' output (crop_init: slot 0 is left out)
    for l in range(T):
        r = R.check(R.column(one, l), R.ref_of(fields[:, :, 1:], l, DRIVER_Q, thr, DRIVER_DIRS, CHANS), f"driver lead {l}")
        print(f"driver lead {l}: worst err / bound {r:.4f}")
    assert 0.0 < float(one["exceed"][0, 0, :T].mean()) < 1.0
    # all lead times in one decode batch: every lead time still has a decoder call of its own, so the same oracle holds
    for l in range(T):
        R.check(R.column(every, l), R.ref_of(fields[:, :, 1:], l, DRIVER_Q, thr, DRIVER_DIRS, CHANS), f"driver, one decode batch, lead {l}")
    two = products_of_latent_rollout(s["latents"], s["model"], s["mean"], s["std"], total_num_steps=T + 1, crop_init=True, decode_batch_frames=2 * ENS,
                                     **s["kw"])  # batches of two lead times and a last one of one
    for k in one:
        assert R.same_value_bits(one[k], two[k]), k
    # crop_init off: the initial condition is lead 0; force_ens_size: the first members only
    full = products_of_latent_rollout(s["latents"], s["model"], s["mean"], s["std"], force_ens_size=4, **s["kw"])
    assert full["mean"].shape == (3, T + 1, H, W)
    for l in (0, T):  # the decoder's schedule follows the launch size: the oracle's fields come from a decoder call of the same 4 frames
        sub = decode_latent_ens(s["model"], s["latents"][:4, :, l:l + 1], s["mean"], s["std"]).cpu()
        R.check(R.column(full, l), R.ref_of(sub, 0, DRIVER_Q, thr, DRIVER_DIRS, CHANS), f"driver force_ens_size lead {l}")
    with pytest.raises(ValueError):
        products_of_latent_rollout(s["latents"], s["model"], s["mean"], s["std"], total_num_steps=T, **s["kw"])


def test_driver_decode_batch_size_same_bits(driver):
    """`decode_batch_frames` of one lead time and of all lead times give the same bits."""
    one, every = driver["one"], driver["every"]
    worst = {}
    for k in one:
        a, b = one[k], every[k]
        ok = ~torch.isnan(a) & ~torch.isnan(b)
        worst[k] = (int((a[ok] != b[ok]).sum()), int(ok.sum()), float((a[ok] - b[ok]).abs().max()))
        print(f"decode batch of one lead time vs of all lead times: {k}: {worst[k][0]} of {worst[k][1]} values differ, max abs diff {worst[k][2]:.3e}")
    for k in one:
        assert R.same_value_bits(one[k], every[k]), f"{k}: the decode batch size changed the bits: {worst[k]}"


def test_lead_times_per_launch_do_not_change_a_bit(E):
    """the kernel is pointwise: L lead times in one launch, and one launch per lead time into the same buffers, give the same bits"""
    H, W = R.SHAPES[1]
    c = R.physical_case(10, H, W)
    thr, dirs = R.phys_thresholds((0, 1, 2))
    kw = dict(quantiles=R.QUANTILES, thresholds=thr, threshold_dirs=dirs, mean=c["mean"].cuda(), std=c["std"].cuda(), target_std=0.5)
    v = c["v"].cuda()
    a = E.rollout_products(v, **kw)
    b = E.empty_products(C, L, H, W, "cuda", n_quantiles=len(R.QUANTILES), n_thresholds=2)
    for l in range(L):
        res = E.rollout_products(v[:, :, l:l + 1], out=b, l_off=l, **kw)
        assert all(x is y for x, y in zip(res._buffers, b._buffers))  # `out` is filled in place
    for k in a:
        assert R.same_value_bits(a[k], b[k]), k
