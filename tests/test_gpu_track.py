"""The cyclone tracker on the MI355X (ladcast_amd/evaluate/track.py; track.hip): the search and whole tracks bit for bit against the
fixture made by the reference's own tracking code (tests/golden/make_track_golden.py), random cases against the numpy restatement
tests/track_oracle.py, the mean and gather kernels against numpy / decode_latent_ens, and the --latent_path flow end to end."""
import os
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

from tests import track_oracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_ref.npz")
T0 = datetime(2018, 10, 1, 0)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def _latlon(track):
    return np.array([(la, lo) for _, la, lo in track], dtype=np.float64)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_query_kernel_equals_fixture_bit_for_bit(gold):
    from ladcast_amd.evaluate.track import find_local_minima

    fields = _dev(gold["q_fields"])
    res = find_local_minima(fields, [tuple(c) for c in gold["q_center"]], gold["q_inner"].tolist(), gold["q_field_idx"].tolist())
    for q, r in enumerate(res):
        if gold["q_found"][q]:
            assert r is not None, q
            assert (r[0], r[1]) == tuple(gold["q_latlon"][q]), q
            assert np.float32(r[2]).tobytes() == gold["q_value"][q].tobytes(), q
        else:
            assert r is None, q


def test_tracks_equal_fixture(gold):
    import warnings

    from ladcast_amd.evaluate.track import track_first_n_steps

    for i in range(int(gold["n_tracks"])):
        em = bool(gold[f"t{i}_enforce_msl"])
        mslp = gold[f"t{i}_mslp"]
        kw = {} if em else dict(z700=_dev(gold[f"t{i}_z700"]), land_sea_mask=_dev(gold[f"t{i}_lsm"]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            trk, codes = track_first_n_steps(T0, *gold[f"t{i}_start"], _dev(mslp), n_steps=mslp.shape[0] - 1,
                                             inner_box_sizes=gold[f"t{i}_boxes"].tolist(), enforce_msl=em, return_codes=True, **kw)
        assert np.array_equal(_latlon(trk), gold[f"t{i}_track"]), i
        assert [t for t, _, _ in trk] == [T0 + timedelta(hours=6 * k) for k in range(mslp.shape[0])]
        _, want_codes = O.track_first_n_steps(T0, *gold[f"t{i}_start"], mslp, mslp.shape[0] - 1, list(gold[f"t{i}_boxes"]), em,
                                             gold.get(f"t{i}_z700"), gold.get(f"t{i}_lsm"), return_codes=True)
        assert list(codes) == want_codes, i
    # the ensemble: every member and the mean of the members (taken on the device) in one launch each
    from ladcast_amd import hip

    mem = _dev(gold["ens_members"])
    E, T = mem.shape[:2]
    mean = torch.empty_like(mem[0])
    hip.track_nanmean(mem, mean, member_stride=mem[0].numel(), E=E, n=mean.numel())
    assert np.array_equal(mean.cpu().numpy(), gold["ens_mean_field"], equal_nan=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        tracks = track_first_n_steps(T0, *gold["ens_start"], torch.cat([mem, mean[None]]), n_steps=T - 1)
    for e in range(E):
        assert np.array_equal(_latlon(tracks[e]), gold["ens_tracks"][e]), e
    assert np.array_equal(_latlon(tracks[E]), gold["ens_mean_track"])


def _random_case(rng, T):
    """background + 1..3 Gaussian lows anywhere (poles and the 0/360 seam included), noise, optional plateaus and NaN patches"""
    lat, lon = O.grid()
    la, lo = lat[:, None], lon[None, :]
    f = np.full((T, lat.size, lon.size), 1000.0)
    n_lows = rng.integers(1, 4)
    c_la, c_lo = rng.uniform(-90, 90, n_lows), rng.uniform(0, 360, n_lows)
    v_la, v_lo = rng.uniform(-2, 2, n_lows), rng.uniform(-4, 4, n_lows)
    depth, rad = rng.uniform(5, 60, n_lows), rng.uniform(1.5, 5, n_lows)
    for t in range(T):
        for k in range(n_lows):
            d2 = ((la - (c_la[k] + v_la[k] * t)) ** 2 + ((lo - c_lo[k] - v_lo[k] * t + 180) % 360 - 180) ** 2) / rad[k] ** 2
            f[t] -= depth[k] * np.exp(-0.5 * d2)
    kind = rng.integers(0, 4)
    if kind == 0:
        f += rng.standard_normal(f.shape) * rng.uniform(0.01, 2)
    elif kind == 1:
        f = np.round(f / rng.choice([1.0, 5.0, 20.0]))  # plateaus of equal values
    else:
        f = f + rng.standard_normal(f.shape) * 0.05
    f = f.astype(np.float32)
    if rng.random() < 0.3:
        r0, c0 = rng.integers(0, 115), rng.integers(0, 235)
        f[rng.integers(0, T):, r0 : r0 + rng.integers(1, 6), c0 : c0 + rng.integers(1, 6)] = np.nan
    start = (float(c_la[0] + rng.uniform(-3, 3)), float((c_lo[0] + rng.uniform(-3, 3)) % 360 if rng.random() < 0.8 else rng.uniform(-1, 361)))
    if rng.random() < 0.15:
        start = (float(rng.choice([-90.0, -89.0, -88.5, 88.0, 89.9, 90.0])), start[1])
    return f, start


def test_random_cases_equal_oracle():
    """>= 200 seeded random cases vs tests/track_oracle.py: each box set, both enforce_msl settings, one launch per group"""
    from ladcast_amd.evaluate.track import _track_launch, round_to_grid

    rng = np.random.default_rng(7)
    T = 5
    groups = [([7, 4, 1], True), ([7, 5, 1], True), ([6, 3, 0], True), ([0], True), ([12, 2], True), ([30, 9, 0], True),
              ([7, 4, 1], False), ([6, 3, 0], False)]
    per = 26
    n = 0
    for boxes, em in groups:
        cases = [_random_case(rng, T) for _ in range(per)]
        z = [_random_case(rng, T)[0] for _ in range(per)] if not em else None
        lsm = (rng.random((120, 240)) < 0.4).astype(np.float32)
        stack = [np.stack([c[0], zz], axis=1) for c, zz in zip(cases, z)] if not em else [c[0][:, None] for c in cases]
        buf = _dev(np.stack(stack))  # (per, T, nc, H, W)
        nc = buf.shape[2]
        starts = [(round_to_grid(s[0]), round_to_grid(s[1])) for _, s in cases]
        lats, lons, codes = _track_launch(buf, track_stride=T * nc * 28800, frame_stride=nc * 28800, mslp_off=0, z_off=None if em else 28800,
                                          lsm=None if em else _dev(lsm), n_tracks=per, n_frames=T, n_steps=T - 1, lat0=[s[0] for s in starts],
                                          lon0=[s[1] for s in starts], inner_box_sizes=boxes, enforce_msl=em, lat=None, lon=None)
        for i, (f, s) in enumerate(cases):
            want, wcodes = O.track_first_n_steps(T0, s[0], s[1], f, T - 1, boxes, em, None if em else z[i], None if em else lsm,
                                                 return_codes=True)
            assert np.array_equal(np.stack([lats[i], lons[i]], 1), _latlon(want)), (boxes, em, i, s)
            assert list(codes[i]) == wcodes, (boxes, em, i)
            n += 1
    assert n >= 200


def test_nanmean_kernel_equals_numpy():
    from ladcast_amd import hip

    rng = np.random.default_rng(3)
    for E in (1, 2, 7, 50):
        x = (rng.standard_normal((E, 3, 257)) * 1000 + 101325).astype(np.float32)
        x[rng.random(x.shape) < 0.2] = np.nan
        x[:, 0, :5] = np.nan
        x[0, 1, 0] = -0.0
        d = _dev(x)
        out = torch.empty(3, 257, device=DEV)
        hip.track_nanmean(d, out, member_stride=3 * 257, E=E, n=3 * 257)
        want = torch.from_numpy(O.nanmean_members(x))
        assert torch.equal(out.cpu().nan_to_num(7.0), want.nan_to_num(7.0)), E
        assert torch.equal(out.cpu().isnan(), want.isnan())


def _small_dcae():
    from ladcast_amd.models import AutoencoderDC
    from oracle.dcae import CONFIG_DCAE_84
    from tests.synth import make_dcae

    ae_cfg = dict(CONFIG_DCAE_84, encoder_block_out_channels=(84, 84, 84, 168), decoder_block_out_channels=(84, 84, 84, 168),
                  encoder_layers_per_block=(1, 1, 1, 1), decoder_layers_per_block=(1, 1, 1, 1))
    gae = AutoencoderDC.from_config(ae_cfg)
    gae.load_state_dict(make_dcae(ae_cfg).state_dict(), strict=True)
    return gae.cuda().eval()


def _stats():
    g = torch.Generator().manual_seed(5)
    mean, std = torch.randn(84, generator=g) * 10, torch.rand(84, generator=g) * 3 + 0.5
    mean[81], std[81] = 101325.0, 1200.0
    mean[9], std[9] = 30000.0, 500.0
    return mean, std


@pytest.mark.parametrize("mode", ["fp32", "bf16x3", "bf16"])
def test_gather_equals_decode_latent_ens(mode):
    from ladcast_amd import hip
    from ladcast_amd.pipelines.utils import _device_vector, inverse_normalize_transform_3D

    gae = _small_dcae().set_gemm_precision(mode)
    mean, std = _stats()
    z = torch.randn(2, 84, 3, 15, 30, generator=torch.Generator().manual_seed(11))
    x = z.to(DEV).permute(0, 2, 1, 3, 4).reshape(6, 84, 15, 30).contiguous()
    y = gae.decode(x).sample  # (B*T, C, H, W), the frame-major output the flow gathers from
    dec = inverse_normalize_transform_3D(y.reshape(2, 3, 84, 120, 240).permute(0, 2, 1, 3, 4).contiguous(), mean, std)  # decode_latent_ens
    ch = [81, 9]
    out = torch.full((2, 5, 2, 120, 240), float("nan"), device=DEV)
    md, sd = _device_vector(mean, DEV), _device_vector(std, DEV)
    hip.track_gather(y, out, ch, md, sd, sb=3 * 84 * 28800, st=84 * 28800, sc=28800, B=2, T=3, HW=28800, T_total=5, t_off=1)
    for k, c in enumerate(ch):
        assert torch.equal(out[:, 1:4, k], dec[:, c]), (mode, c)
    assert out[:, 0].isnan().all() and out[:, 4].isnan().all()  # only the frames at t_off .. t_off + T were written
    # the (B, C, T, H, W) layout of decode_latent_ens's own output gives the same values
    raw = y.reshape(2, 3, 84, 120, 240).permute(0, 2, 1, 3, 4).contiguous()
    out2 = torch.empty(2, 3, 2, 120, 240, device=DEV)
    hip.track_gather(raw, out2, ch, md, sd, sb=84 * 3 * 28800, st=28800, sc=3 * 28800, B=2, T=3, HW=28800, T_total=3, t_off=0)
    assert torch.equal(out2, out[:, 1:4])


def test_track_latent_ensemble_end_to_end(tmp_path):
    """a latent_YYYYMMDDHH.npy written by save_latent_npy -> track_latent_ensemble: the member tracks and the mean track equal
    tests/track_oracle.py on decode_latent_ens output, under every decode_batch_frames; two launches are bitwise equal"""
    import warnings

    from ladcast_amd.evaluate.track import track_latent_ensemble
    from ladcast_amd.pipelines.io import save_latent_npy
    from ladcast_amd.pipelines.utils import decode_latent_ens

    gae = _small_dcae()
    mean, std = _stats()
    n_steps, ens = 8, 3
    lat_ = torch.randn(1, ens, 84, n_steps + 2, 15, 30, generator=torch.Generator().manual_seed(21))
    (path,) = save_latent_npy(lat_, [2018100100], str(tmp_path))
    members = [0, 2]
    want_fields = [decode_latent_ens(gae, lat_[0, m : m + 1], mean.to(DEV), std.to(DEV), extract_first=n_steps + 1)[0, 81].cpu().numpy()
                   for m in members]
    start = (15.2, 140.3)
    t0 = datetime(2018, 10, 1, 0)
    want = {f"M{m}": _latlon(O.track_first_n_steps(t0, *start, f, n_steps)) for m, f in zip(members, want_fields)}
    want_mean = _latlon(O.track_first_n_steps(t0, *start, O.nanmean_members(np.stack(want_fields)), n_steps))
    results = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        for dbf in (None, 1, 7, None):
            ens_tracks, mean_track, buf = track_latent_ensemble(path, gae, mean, std, *start, n_steps, ens_member_idx=members,
                                                                decode_batch_frames=dbf, return_fields=True)
            results.append((ens_tracks, mean_track, buf))
            assert set(ens_tracks) == set(want)
            for k in want:
                assert np.array_equal(_latlon(ens_tracks[k]), want[k]), (dbf, k)
                assert ens_tracks[k][0][0] == t0 and ens_tracks[k][-1][0] == t0 + timedelta(hours=6 * n_steps)
            assert np.array_equal(_latlon(mean_track), want_mean), dbf
    # decode_batch_frames=None is the reference's decode call: fields bit-equal to decode_latent_ens, mean bit-equal to np.nanmean
    buf = results[0][2]
    for i in range(len(members)):
        assert np.array_equal(buf[i, :, 0].cpu().numpy(), want_fields[i])
    assert np.array_equal(buf[len(members), :, 0].cpu().numpy(), O.nanmean_members(np.stack(want_fields)))
    assert torch.equal(results[0][2], results[3][2]) and results[0][:2] == results[3][:2]  # two runs, bitwise equal


def test_two_launches_bitwise_equal_and_refusals(gold):
    import warnings

    from ladcast_amd import hip
    from ladcast_amd.evaluate.track import find_local_minima, track_first_n_steps

    mem = _dev(gold["ens_members"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        a = track_first_n_steps(T0, 18.2, 139.9, mem, n_steps=6, return_codes=True)
        b = track_first_n_steps(T0, 18.2, 139.9, mem, n_steps=6, return_codes=True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    with pytest.raises(RuntimeError):
        track_first_n_steps(T0, 18.2, 139.9, mem.cpu(), n_steps=6)
    with pytest.raises(ValueError):
        track_first_n_steps(T0, 18.2, 139.9, mem, n_steps=6, inner_box_sizes=[31])
    with pytest.raises(ValueError):
        track_first_n_steps(T0, 18.2, 139.9, mem, n_steps=6, inner_box_sizes=[1] * 9)
    with pytest.raises(ValueError):
        track_first_n_steps(T0, 18.2, 139.9, mem, n_steps=7)  # 7 frames hold 6 steps
    with pytest.raises(ValueError):
        find_local_minima(mem[0], [(18.0, 140.0)], [31])
    # the C ABI refuses over-cap box lists before launch
    f64 = torch.zeros(1, dtype=torch.float64, device=DEV)
    lat, lon = _dev(gold["lat"]), _dev(gold["lon"])
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    code = torch.zeros(1, dtype=torch.int32, device=DEV)
    for boxes in ([31], [1] * 9):
        with pytest.raises(RuntimeError, match="status -3"):
            hip.track_storms(mem, lat, lon, f64, f64, out, out, code, track_stride=0, frame_stride=28800, mslp_off=0, z_off=-1, lsm=None,
                             H=120, W=240, n_tracks=1, n_steps=1, inner_box_sizes=boxes, enforce_msl=True)
