"""Derived fields on the device: `ldc_derive_fields` through `derive_forecast` / `derive_table` against the host reference
(tests/derived_refs.py), and the two drivers (`score_latent_rollout`, `products_of_latent_rollout`) with `derived=` on the tiny DC-AE of
tests/test_gpu_evaluate_ens.py.

Bounds.  `diff` is one fp32 subtraction of inputs that hold the reference's bits: bit-equal.  `speed` / `shear`: the squares are exact
in double, the sum and the root are each correctly rounded in the reference; a device root that is only faithful (within one double
ulp) can, after the one rounding to fp32, differ from the reference only where the double result lies at an fp32 rounding boundary:
at most 1 fp32 ulp, and on almost no element.  The tests print the number of elements that differ at all.  +0 and -0 compare equal."""
import json
import math

import numpy as np
import pytest
import torch

from oracle import scoring as S
from tests import derived_refs as R
from tests.redzone import assert_untouched, guarded
from tests.synth import tiny_dcae_config
from tests.test_gpu_evaluate_ens import C, C_LAT, ENS, H, INIT, KEYS, SST, T, TRUTH_SLOTS, W, _close, _same_bits, _tables, h, setup, w  # noqa: F401

pytestmark = pytest.mark.gpu

FIELDS = [("speed", "speed", (0, 1)), ("thick", "diff", (2, 4)), ("shear", "shear", (0, 1, 5, 6))]
D = len(FIELDS)


def _check(got, want, fields, what):
    """diff fields bit-equal (NaN pattern included), speed / shear within 1 ulp; channels on axis -3 of both"""
    got, want = got.detach().cpu().numpy(), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, want.shape)
    for k, f in enumerate(fields):
        d = R.ulp_distance(got[..., k, :, :], want[..., k, :, :])
        n = int((d != 0).sum())
        if f[1] != "diff" and n:
            print(f"{what}: field {k} ({f[1]}): {n} of {d.size} elements differ from the reference, by at most {int(d.max())} ulp")
        assert int(d.max()) <= (0 if f[1] == "diff" else 1), (what, k, f, int(d.max()))


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead_dim", [0, 2])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("hw", [(3, 5), (4, 8)])  # odd HW: the scalar path; HW % 4 == 0: the 16-byte path
def test_derive_forecast_shapes_and_strides(hw, M, L, lead_dim):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), Cc = hw, 5
    g = torch.Generator().manual_seed(3 + 7 * M + L)
    # a slice of a larger tensor: member, lead and channel strides all differ from the dense ones
    big = torch.randn((M + 1, Cc + 2, L + 1, Hh, Ww) if lead_dim == 2 else (L + 1, M + 1, Cc + 2, Hh, Ww), generator=g).cuda()
    view = big[1:, 1 : 1 + Cc, :L] if lead_dim == 2 else big[:L, 1:, 1 : 1 + Cc]
    mean, std = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    fields = [("s", "speed", (0, 1)), ("d", "diff", (2, 0)), ("sh", "shear", (0, 1, 3, 4)), ("twice", "speed", (1, 1)), ("dd", "diff", (4, 4))]
    for target_std in (1.0, 0.5):
        got = derive_forecast(view, fields, lead_dim=lead_dim, mean=mean.cuda(), std=std.cuda(), target_std=target_std)
        assert got.shape == ((M, len(fields), L, Hh, Ww) if lead_dim == 2 else (L, M, len(fields), Hh, Ww)) and got.is_contiguous()
        want = R.derive(view.cpu().numpy(), fields, 1 if lead_dim == 2 else 2, mean.numpy(), std.numpy(), target_std)
        if lead_dim == 2:  # channels to axis -3 for the comparison
            _check(got.permute(0, 2, 1, 3, 4), want.transpose(0, 2, 1, 3, 4), fields, f"{hw} M={M} L={L}")
        else:
            _check(got, want, fields, f"{hw} M={M} L={L} lead-major")
    phys = derive_forecast(view, fields[:2], lead_dim=lead_dim)  # no mean: the source is physical, its bits are taken as they are
    want = R.derive(view.cpu().numpy(), fields[:2], 1 if lead_dim == 2 else 2)
    _check(phys.movedim(1 if lead_dim == 2 else 2, -3), np.moveaxis(want, 1 if lead_dim == 2 else 2, -3), fields[:2], "physical")


@pytest.mark.parametrize("n_fields", [1, 16])
@pytest.mark.parametrize("offset", [0, 1, 3])  # elements: 1 and 3 leave every plane base off the 16-byte grid while HW % 4 == 0
def test_odd_storage_offset_and_field_counts(offset, n_fields):
    from ladcast_amd.evaluate import derive_forecast

    M, Cc, L, Hh, Ww = 2, 40, 2, 4, 8
    g = torch.Generator().manual_seed(17 + offset)
    flat = torch.randn(offset + M * Cc * L * Hh * Ww, generator=g).cuda()
    view = flat[offset:].view(M, Cc, L, Hh, Ww)
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    kinds = ("speed", "diff", "shear")
    # 16 fields over 40 channels: more than 16 distinct source channels, so more than one launch; channel 0 feeds several fields
    fields = [(f"f{k}", kinds[k % 3], tuple((0, 2 * k + 1, 2 * k + 2, 39 - k)[: R.KIND_CHANNELS[kinds[k % 3]]])) for k in range(n_fields)]
    got = derive_forecast(view, fields)
    _check(got.permute(0, 2, 1, 3, 4), R.derive(view.cpu().numpy(), fields, 1).transpose(0, 2, 1, 3, 4), fields, f"offset {offset}, {n_fields} fields")


# ---- 2. values -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])  # the 16-byte path and the scalar path
def test_special_values(offset):
    from ladcast_amd.evaluate import derive_forecast

    nan, inf = float("nan"), float("inf")
    vals = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1e-45, inf, -inf, nan, 1e30, -1e30, 1e-30, -1e-30, 1.5, -2.25, 3.0e38, 17.2], dtype=torch.float32)
    n = vals.numel()  # every pair (a, b) on an n x n plane; c, d: the same grid rolled, so every value meets every other in the shear too
    a, b = vals.view(n, 1).expand(n, n), vals.view(1, n).expand(n, n)
    planes = torch.stack([a, b, b.roll(3, 1), a.roll(5, 0)]).reshape(1, 4, 1, n, n)
    flat = torch.empty(offset + planes.numel()).cuda()
    view = flat[offset:].view(planes.shape)
    view.copy_(planes)
    fields = [("s", "speed", (0, 1)), ("d", "diff", (0, 1)), ("sh", "shear", (0, 1, 2, 3))]
    got = derive_forecast(view, fields)[0, :, 0].cpu()
    want = R.derive(planes.numpy(), fields, 1)[0, :, 0]
    _check(got.unsqueeze(0), want[None], fields, "special values")
    s, d = got[0], got[1]
    isn = torch.isnan(vals)
    assert bool(torch.isnan(s[isn]).all()) and bool(torch.isnan(s[:, isn]).all()) and bool(torch.isnan(d[isn]).all())  # NaN in one input, the other, both
    i30, j30 = vals.tolist().index(float(np.float32(1e30))), vals.tolist().index(float(np.float32(-1e30)))
    assert math.isfinite(float(s[i30, j30])) and abs(float(s[i30, j30]) / 1e30 - math.sqrt(2.0)) < 1e-6  # fp32 squares would be inf
    t30 = vals.tolist().index(float(np.float32(1e-30)))
    assert float(s[t30, t30]) > 1.4e-30  # fp32 squares would be 0
    den = vals.tolist().index(float(np.float32(1e-40)))
    assert float(s[den, 0]) == float(np.float32(1e-40)) and float(d[den, 0]) == float(np.float32(1e-40))  # denormals are not flushed
    assert float(s[0, 1]) == 0.0 and float(s[5, 6]) == inf and math.isnan(float(d[5, 5]))  # +-0; inf, inf; inf - inf


# ---- 3. tables -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 5), (4, 8)])
def test_derive_table(hw):
    from ladcast_amd.evaluate import derive_table

    (Hh, Ww), N, Cc = hw, 5, 7
    g = torch.Generator().manual_seed(23)
    table = (torch.randn(N, Cc, Hh, Ww, generator=g) * 30.0).cuda()
    fields = [("s", "speed", (0, 1)), ("d", "diff", (2, 4)), ("sh", "shear", (0, 1, 5, 6))]
    slots = [3, 0, 3, 1]  # out of order and repeated
    got = derive_table(table, slots, fields)
    assert got.shape == (4, 3, Hh, Ww)
    _check(got, R.derive(table.cpu().numpy()[slots], fields, 1), fields, "slots")
    _check(derive_table(table, torch.tensor(slots), fields), R.derive(table.cpu().numpy()[slots], fields, 1), fields, "tensor slots")
    for bad in ([0, 5], [-1], []):
        with pytest.raises(ValueError):
            derive_table(table, bad, fields)
    clt = table.permute(1, 0, 2, 3).contiguous()  # (C, L, H, W), no slots
    _check(derive_table(clt, None, fields), R.derive(table.cpu().numpy(), fields, 1), fields, "no slots")
    _check(derive_table(table.permute(1, 0, 2, 3), None, fields), R.derive(table.cpu().numpy(), fields, 1), fields, "no slots, a permuted view")


# ---- 4. writes stay where they belong --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("hw", [(3, 5), (4, 8)])
def test_out_as_tail_channels_keeps_head_and_guards(hw, offset):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), L, M, Cc = hw, 2, 3, 6
    fields = FIELDS[:2] + [("sh", "shear", (0, 1, 5, 3))]
    n = L * M * (Cc + 3) * Hh * Ww
    buf = guarded(1, offset + n)
    flat = buf.view[0, 0]
    flat[:offset] = 123.0
    ext = flat[offset:].view(L, M, Cc + 3, Hh, Ww)  # lead-major, as the drivers' buffer
    g = torch.Generator().manual_seed(29)
    head = torch.randn(L, M, Cc, Hh, Ww, generator=g)
    ext[:, :, :Cc] = head.cuda()
    mean, std = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    out = derive_forecast(ext[:, :, :Cc], fields, lead_dim=0, mean=mean.cuda(), std=std.cuda(), out=ext[:, :, Cc:])
    assert out.data_ptr() == ext[:, :, Cc:].data_ptr()
    assert_untouched(buf, f"derive_forecast {hw} offset {offset}")
    assert torch.equal(ext[:, :, :Cc].cpu(), head) and bool((flat[:offset].cpu() == 123.0).all())
    _check(ext[:, :, Cc:], R.derive(head.numpy(), fields, 2, mean.numpy(), std.numpy()), fields, "tail")


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    import ctypes

    from ladcast_amd import hip
    from ladcast_amd.evaluate import derive_forecast, derive_table

    x = torch.randn(2, 4, 1, 4, 8)
    with pytest.raises(RuntimeError):
        derive_forecast(x, FIELDS[:1])  # host tensors
    with pytest.raises(RuntimeError):
        derive_table(x[0], None, FIELDS[:1])
    with pytest.raises(RuntimeError):
        derive_forecast(x.cuda(), FIELDS[:1], mean=torch.zeros(4), std=torch.ones(4))
    with pytest.raises(NotImplementedError):
        derive_forecast(x.cuda().half(), FIELDS[:1])
    with pytest.raises(NotImplementedError):
        derive_table(x[0].cuda().half(), None, FIELDS[:1])
    for bad in ([("s", "speed", (0, 1))] * 17, [("s", "speed", (0, 4))], [("s", "speed", (-1, 0))], [("s", "hypot", (0, 1))], [("s", "shear", (0, 1))], []):
        with pytest.raises(ValueError):
            derive_forecast(x.cuda(), bad)
    for bad_out in (torch.empty(2, 1, 1, 4, 8), torch.empty(2, 2, 1, 4, 8).cuda(), torch.empty(2, 1, 1, 8, 4).cuda().transpose(3, 4)):
        with pytest.raises((ValueError, RuntimeError)):
            derive_forecast(x.cuda(), FIELDS[:1], out=bad_out)
    with pytest.raises(ValueError):
        derive_forecast(x.cuda(), FIELDS[:1], lead_dim=1)
    # the C ABI itself: a wrong kind, a channel out of range, D outside 1 .. 16
    xd, out = x.cuda(), torch.empty(2, 1, 1, 4, 8).cuda()
    keep = out.clone()

    def call(desc, n):
        return hip.lib.ldc_derive_fields(xd.data_ptr(), 128, 32, 32, None, None, None, 1.0, 2, 1, 4, 32, desc, n, out.data_ptr(), 32, 32, 32, None)

    one = (hip.DeriveDesc * 1)()
    one[0].kind, one[0].ch[0], one[0].ch[1] = 7, 0, 1
    assert call(one, 1) == -1  # LDC_ERR_ARG
    one[0].kind, one[0].ch[1] = hip.DERIVE_DIFF, 4
    assert call(one, 1) == -1
    many = (hip.DeriveDesc * 17)()
    assert call(many, 17) == -1 and call(many, 0) == -1
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), keep.view(torch.int32))  # nothing was launched
    one[0].ch[1] = 3
    assert call(one, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, 0].cpu(), x[:, 0] - x[:, 3])
    assert ctypes.sizeof(hip.DeriveDesc) == hip.lib.ldc_sizeof_derive_desc() == 20


# ---- 6 .. 9. the drivers ---------------------------------------------------------------------------------------------------------------------
def _decode(s, s0, nl):
    lat = s["latents"][:, :, 1:]
    x = lat[:, :, s0 : s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ENS, C_LAT, h, w).contiguous().cuda()
    return s["g"].decode(x).sample.reshape(nl, ENS, C, H, W)  # normalised, lead-major


def _extended(s, y, t_slots, c_slots):
    """the extended batch by hand, from the public derive_* functions: forecast, truth, clim with the derived fields as tail channels"""
    from ladcast_amd.evaluate import derive_forecast, derive_table

    md, sd, td, cd = s["mean"].cuda(), s["std"].cuda(), s["truth"].cuda(), s["clim"].cuda()
    ext = torch.cat([y, derive_forecast(y, FIELDS, lead_dim=0, mean=md, std=sd)], dim=2)
    truth = torch.cat([td[t_slots], derive_table(td, t_slots, FIELDS)], dim=1)
    clim = torch.cat([cd[c_slots], derive_table(cd, c_slots, FIELDS)], dim=1)
    for k, f in enumerate(FIELDS):
        if f[1] != "diff":
            clim[:, C + k] = float("nan")
    return ext, truth, clim


def _scales(s):
    st = [float(v) for v in s["std"]]
    return torch.tensor(st + [math.sqrt(st[0] ** 2 + st[1] ** 2), math.sqrt(st[2] ** 2 + st[4] ** 2), math.sqrt(sum(st[c] ** 2 for c in (0, 1, 5, 6)))], dtype=torch.float64)


def _options(s):
    from ladcast_amd.evaluate.energy import EnergyGroup
    from ladcast_amd.evaluate.regional import Region
    from ladcast_amd.evaluate.utils import Event

    events = [Event(0, "gt", float(s["mean"][0])), Event(C, "gt", 1.1 * float(s["std"][0])), Event(C + 1, "lt", 0.0, True)]  # decoded; the speed field; the diff's anomaly
    return dict(reliability=True, spectrum=True, events=events, fss_radii=(0, 2), regions=[Region("box", -20.0, 20.0, 30.0, 120.0)], energy=True,
                energy_groups=[EnergyGroup("mixed", (2, C)), EnergyGroup("decoded", (0, 1))])  # a decoded and a derived channel together


CHANNEL_AXIS = dict(regional_sums=1, regional_counts=1)  # the axis of length C of a result; None: no channel axis
NO_CHANNEL = ("event_hist", "event_hist_weighted", "event_n_invalid", "event_fss_sums", "event_fss_n_invalid", "energy_group_score", "energy_group_score_fair",
              "energy_group_skill", "energy_group_spread", "energy_group_weight", "energy_group_n_invalid")


def _rows(k, v, lo, hi):
    return v if k in NO_CHANNEL or k.startswith("energy_group") else v.narrow(CHANNEL_AXIS.get(k, 0), lo, hi - lo)


@pytest.mark.parametrize("dbf", [3, 6])
def test_score_latent_rollout_with_derived(setup, dbf):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.rollout_metrics import METRICS, Batch
    from ladcast_amd.evaluate.utils import rollout_scores
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D

    s = setup
    args = (s["latents"], s["g"], s["mean"], s["std"], s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"])
    kw = dict(sst_channel=SST, crop_init=True, decode_batch_frames=dbf)
    opts = _options(s)
    got = EG.score_latent_rollout(*args, derived=FIELDS, **opts, **kw)
    decoded_opts = dict(opts, events=opts["events"][:1], energy_groups=opts["energy_groups"][1:])
    plain = EG.score_latent_rollout(*args, **decoded_opts, **kw)
    assert all(got[k].shape == (C + D, T) for k in KEYS)
    # a. rows 0 .. C - 1: the bits of the call without derived fields, for the five scores and every optional metric
    for k, v in plain.items():
        if k in NO_CHANNEL or k.startswith("energy_group"):
            continue  # events and groups are compared below, entry by entry
        assert _same_bits(_rows(k, got[k], 0, C).double(), v.double()) and got[k].dtype == v.dtype, k
    for k in ("event_hist", "event_hist_weighted", "event_n_invalid", "event_fss_sums", "event_fss_n_invalid"):
        assert _same_bits(got[k][:1].double(), plain[k].double()), k  # the decoded channel's event
    for k in got:
        if k.startswith("energy_group"):
            assert _same_bits(got[k][1:].double(), plain[k].double()), k  # the decoded group
    # b. rows C ..: the bits of the scorers run on an extended batch built by hand
    per = max(1, dbf // ENS)
    dev = "cuda"
    scores = torch.full((5, C + D, T), float("nan"), device=dev)
    o = dict(opts, spectrum_row_weight=None, region_mask=None, energy_scales=_scales(s), clim=s["clim"], std_tensor=None)
    metrics = [m for m in (cls.for_rollout(o) for cls in METRICS) if m is not None]
    lat_w = s["lat_w"].cuda()
    for m in metrics:
        m.start(lat_w)
    mean_e = torch.cat([s["mean"], torch.zeros(D)]).cuda()
    std_e = torch.cat([s["std"], torch.ones(D)]).cuda()
    fields64 = []
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        y = _decode(s, s0, nl)
        ext, truth, clim = _extended(s, y, TRUTH_SLOTS[s0 : s0 + nl], s["clim_slots"][s0 : s0 + nl])
        b = Batch(ext, truth, lat_w, SST, T, dict(lead_dim=0, mean=mean_e, std=std_e, truth_slot=list(range(nl)), l_off=s0),
                  dict(clim=clim, clim_slots=list(range(nl))))
        rollout_scores(ext, truth, clim, lat_w, SST, lead_dim=0, mean=mean_e, std=std_e, truth_slots=list(range(nl)), clim_slots=list(range(nl)),
                       out=scores, lead_offset=s0)
        for m in metrics:
            m.run(b)
        fields64.append(inverse_normalize_transform_3D(y.reshape(nl * ENS, C, 1, H, W), s["mean"], s["std"]).reshape(nl, ENS, C, H, W).cpu().double())
    hand = {k: scores[i].cpu() for i, k in enumerate(KEYS)}
    for m in metrics:
        hand.update(m.result())
    assert set(hand) == set(got)
    for k, v in hand.items():
        assert _same_bits(got[k].double(), v.double()) and got[k].dtype == v.dtype, k  # every row, the derived ones among them
    # c. rows C ..: the oracle on fields derived in float64 from the de-normalised decoder output
    f64 = torch.cat(fields64)  # (T, ens, C, H, W)

    def derive64(x, ax):  # x: float64, channels on axis `ax`
        ch = lambda c: x.select(ax, c)  # noqa: E731
        return torch.stack([torch.sqrt(ch(0) ** 2 + ch(1) ** 2), ch(2) - ch(4), torch.sqrt((ch(0) - ch(5)) ** 2 + (ch(1) - ch(6)) ** 2)], dim=ax)

    for l in range(T):
        clim64 = derive64(s["clim"][s["clim_slots"][l]].double(), 0)
        clim64[0] = clim64[2] = float("nan")
        want = S.ensemble_scores(derive64(f64[l], 1), derive64(s["truth"][TRUTH_SLOTS[l]].double(), 0), clim64, s["lat_w"].double(), sst_channel=1)  # nanmean on the diff, which holds no NaN
        for k in KEYS:
            _close(got[k][C:, l], want[k], 1e-5)
    acc = got["ens_acc"][C:]
    assert bool(torch.isnan(acc[0]).all()) and bool(torch.isnan(acc[2]).all()) and bool(torch.isfinite(acc[1]).all())
    assert all(bool(torch.isfinite(got[k][C:]).all()) for k in KEYS[1:])
    # d. host-resident tables: the same bits
    host = EG.score_latent_rollout(*args[:4], s["truth"].numpy(), TRUTH_SLOTS, s["clim"], s["clim_slots"], s["lat_w"], derived=FIELDS, **opts, **kw)
    assert set(host) == set(got)
    for k in got:
        assert _same_bits(host[k].double(), got[k].double()), k


def test_score_latent_rollout_derived_refusals(setup):
    from ladcast_amd.evaluate import Derived, score_latent_rollout
    from ladcast_amd.evaluate.utils import Event

    s = setup
    args = (s["latents"], s["g"], s["mean"], s["std"], s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"])
    kw = dict(sst_channel=SST, crop_init=True)
    with pytest.raises(ValueError, match="SST"):
        score_latent_rollout(*args, derived=[Derived("d", "diff", (SST, 0))], **kw)
    with pytest.raises(ValueError, match="anomaly"):
        score_latent_rollout(*args, derived=FIELDS, events=[Event(C, "gt", 1.0, True)], **kw)
    with pytest.raises(ValueError):
        score_latent_rollout(*args, derived=[Derived("s", "speed", (0, C))], **kw)
    with pytest.raises(ValueError):
        score_latent_rollout(*args, derived=[], **kw)


def test_cli_round_trip_with_derive(setup, tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.io import save_latent_npy

    s = setup
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    lv = (300, 500, 850)
    norm = {"geopotential": {"mean": {str(p): float(s["mean"][i]) for i, p in enumerate(lv)}, "std": {str(p): float(s["std"][i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {str(p): float(s["mean"][3 + i]) for i, p in enumerate(lv)}, "std": {str(p): float(s["std"][3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(s["mean"][6]), "std": float(s["std"][6])},
            "sea_surface_temperature": {"mean": float(s["mean"][7]), "std": float(s["std"][7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    gen = torch.Generator().manual_seed(43)
    save_latent_npy(torch.randn(1, ENS, C_LAT, 1 + T, h, w, generator=gen), [INIT], str(tmp_path / "rollout"))
    truth, full_slots, planes = _tables(gen, s["mean"], s["std"], 10)  # frames from 2020-02-27 00 h: INIT's leads are frames 7, 8, 9
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H, W))
    for i, slot in enumerate(full_slots):
        clim[slot // 4, slot % 4] = planes[i].numpy()
    clim.flush()
    del clim
    out_dir = tmp_path / "scores"
    argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
            "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
            "--end_date", "2020-02-29T12", "--output", str(out_dir), "--total_lead_time_hour", "18", "--crop_init", "--force_ens_size", "2",
            "--decode_batch_frames", "4", "--sst_channel_idx", str(SST), "--variable_names", *names, "--levels", "300", "500", "850", "--num_atm_vars", "2",
            "--derive", "speed", "speed", "geopotential_level300", "geopotential_level500", "--derive", "thick", "diff", "geopotential_level850", "4",
            "--derive", "shear", "shear", "0", "1", "temperature_level850", "2m_temperature", "--event", "speed", "gt", "1.0"]
    torch.manual_seed(1234)
    with pytest.warns(UserWarning):
        res = EG.main(argv)
    ts = str(INIT)
    for k in KEYS:
        assert np.load(out_dir / f"{ts}_{k}.npy").shape == (C + D, T) and np.load(out_dir / f"{k}.npy").shape == (1, C + D, T)
    meta = json.loads((out_dir / "derived.json").read_text())
    st = [float(np.float32(float(v))) for v in s["std"]]
    assert meta["decoded_channels"] == C and [(m["name"], m["kind"], m["channels"], m["index"]) for m in meta["derived"]] == [
        ("speed", "speed", [0, 1], C), ("thick", "diff", [2, 4], C + 1), ("shear", "shear", [0, 1, 5, 6], C + 2)]
    assert meta["derived"][0]["channel_names"] == ["geopotential_level300", "geopotential_level500"]
    assert abs(meta["derived"][0]["scale"] - math.sqrt(st[0] ** 2 + st[1] ** 2)) < 1e-12
    assert json.loads((out_dir / "events.json").read_text())["events"][0]["channel_index"] == C
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in s["mean"]]), torch.tensor([float(v) for v in s["std"]])
    want = EG.score_latent_rollout(str(tmp_path / "rollout" / f"latent_{ts}.npy"), model, mean32, std32, truth, [7, 8, 9], planes, [0, 1, 2],
                                   EG.lat_weights_for(H), sst_channel=SST, crop_init=True, force_ens_size=2, decode_batch_frames=4, derived=FIELDS)
    for k in KEYS:
        assert _same_bits(torch.from_numpy(res[k][0]), want[k]), k


@pytest.mark.parametrize("dbf", [3, 6])
def test_products_with_derived(setup, dbf):
    from ladcast_amd.evaluate import products_of_latent_rollout, rollout_products

    s = setup
    # the hand-built batch: one decoder call per lead time, always ENS frames, as the driver decodes
    ys = torch.cat([_decode(s, l, 1) for l in range(T)])
    ref = R.derive(ys.cpu().numpy(), FIELDS[:1], 2, s["mean"].numpy(), s["std"].numpy())[:, :, 0]  # the reference speed, (T, ens, H, W)
    thr = float(np.float32(np.median(ref) * (1.0 + 2.0 ** -12)))  # about half the members above it, and off the data's own values
    table = torch.full((1, C + D), float("nan"))
    table[0, C] = thr
    args = (s["latents"], s["g"], s["mean"], s["std"])
    kw = dict(crop_init=True, decode_batch_frames=dbf)
    got = products_of_latent_rollout(*args, thresholds=table, derived=FIELDS, **kw)
    plain = products_of_latent_rollout(*args, **kw)
    for k in ("mean", "std", "min", "max"):
        assert got[k].shape == (C + D, T, H, W) and _same_bits(got[k][:C], plain[k]), k  # the decoded channels keep their bits
    assert got["exceed"].shape == (1, C + D, T, H, W) and bool(torch.isnan(got["exceed"][0, :C]).all())
    mean_e, std_e = torch.cat([s["mean"], torch.zeros(D)]).cuda(), torch.cat([s["std"], torch.ones(D)]).cuda()
    ext, _, _ = _extended(s, ys, TRUTH_SLOTS, s["clim_slots"])
    hand = rollout_products(ext, thresholds=table, lead_dim=0, mean=mean_e, std=std_e)
    for k in ("mean", "std", "min", "max", "exceed"):
        assert _same_bits(got[k].narrow(-4, C, D), hand[k].cpu().narrow(-4, C, D)), k
    # the exceedance plane against the reference field: the member count above thr over M, wherever no member is within 1 ulp of thr
    near = (R.ulp_distance(ref, np.full_like(ref, np.float32(thr))) <= 1).any(axis=1)
    print(f"exceedance of speed > {thr:.6g}: {near.mean():.3%} of the points have a member within 1 ulp of the threshold and are left out")
    assert near.mean() < 0.01
    want = (ref > np.float32(thr)).sum(axis=1).astype(np.float32) / np.float32(ENS)
    ex = got["exceed"][0, C].numpy()
    assert 0.05 < want.mean() < 0.95 and np.array_equal(ex[~near], want[~near])
