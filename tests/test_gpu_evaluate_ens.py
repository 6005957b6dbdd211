"""`score_latent_rollout` and the evaluate_ens_gpu command line on the tiny synthetic DC-AE (tests/synth.py).

The driver is held bit for bit to the composition of the public pieces it replaces - the same decoder calls on the same frame batches,
`inverse_normalize_transform_3D`, `ensemble_scores` per lead time - and to the pinned oracle (oracle/scoring.py) fed those same
GPU-decoded, un-normalised fields: the decoder's own accuracy is held by the DC-AE tests and stays out of the scoring check, so the
project's 1e-5 (`_close` of tests/test_gpu_scoring.py) applies unchanged."""
import json

import numpy as np
import pytest
import torch

from oracle import scoring as S
from tests.synth import make_dcae, tiny_dcae_config

pytestmark = pytest.mark.gpu

KEYS = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
SST = 3
ENS, C_LAT, T, h, w = 3, 8, 3, 6, 8
C, H, W = 8, 48, 64
INIT = 2020022812  # leads: 02-28 18 h, 02-29 00 h, 02-29 06 h
TRUTH_SLOTS = [2, 5, 3]


def _close(a, b, tol):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    assert bool((nan_a == nan_b).all()), "NaN pattern differs"
    a, b = a[~nan_a], b[~nan_b]
    if a.numel() == 0:
        return
    assert ((a - b).abs() <= tol * (b.abs() + b.abs().mean())).all(), float(((a - b).abs() / (b.abs() + b.abs().mean())).max())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _tables(gen, mean, std, n_truth):
    """truth frames and the climatology planes of INIT's lead times in physical units, land NaNs in the truth's SST channel"""
    from ladcast_amd.evaluate import climatology_slots

    scale, shift = std.view(1, C, 1, 1), mean.view(1, C, 1, 1)
    truth = torch.randn(n_truth, C, H, W, generator=gen) * scale + shift
    land = torch.rand(H, W, generator=gen) < 0.3
    truth[:, SST][:, land] = float("nan")
    full_slots = climatology_slots(INIT, 6 * T)
    assert full_slots == [58 * 4 + 3, 59 * 4 + 0, 59 * 4 + 1]  # 28 February 18 h, then 29 February = day 60
    planes = torch.randn(5, C, H, W, generator=gen) * 0.3 * scale + shift
    return truth, full_slots, planes


@pytest.fixture(scope="module")
def setup():
    from ladcast_amd.evaluate.evaluate_encdec_model import equiangular_lat_weights
    from ladcast_amd.models import AutoencoderDC

    cfg = tiny_dcae_config()  # 8 fields + 5 static channels, 8 latent channels, 8 x compression
    g = AutoencoderDC.from_config(cfg)
    g.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    g = g.cuda().eval()
    gen = torch.Generator().manual_seed(41)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    latents = torch.randn(ENS, C_LAT, 1 + T, h, w, generator=gen)  # slot 0: the initial condition, cropped
    truth, full_slots, planes = _tables(gen, mean, std, 6)
    # the (366 * 4)-slot climatology cut down to the three slots used plus two decoys, renumbered
    clim, clim_slots = planes, [2, 1, 4]
    return dict(g=g, mean=mean, std=std, latents=latents, truth=truth, clim=clim, clim_slots=clim_slots, lat_w=equiangular_lat_weights(H + 1, True))


def _composition(s, per):
    """the public pieces that exist without the driver, on the same frame batches -> ({key: (C, T)} on the host, physical fields (T, ens, C, H, W))"""
    from ladcast_amd.evaluate import ensemble_scores
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D

    lat = s["latents"][:, :, 1:]
    cols, fields = [], []
    wd, td, cd = s["lat_w"].cuda(), s["truth"].cuda(), s["clim"].cuda()
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        x = lat[:, :, s0 : s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ENS, C_LAT, h, w).contiguous().cuda()
        y = s["g"].decode(x).sample
        phys = inverse_normalize_transform_3D(y.reshape(nl * ENS, C, 1, H, W), s["mean"], s["std"]).reshape(nl, ENS, C, H, W)
        for l in range(nl):
            cols.append(ensemble_scores(phys[l], td[TRUTH_SLOTS[s0 + l]], cd[s["clim_slots"][s0 + l]], wd, SST))
            fields.append(phys[l].cpu())
    return {k: torch.stack([c[k] for c in cols], dim=1).cpu() for k in KEYS}, torch.stack(fields)


@pytest.mark.parametrize("dbf", [3, 6])
def test_score_latent_rollout(setup, dbf):
    from ladcast_amd.evaluate import score_latent_rollout

    s = setup
    args = (s["latents"], s["g"], s["mean"], s["std"])
    kw = dict(sst_channel=SST, crop_init=True, decode_batch_frames=dbf)
    got = score_latent_rollout(*args, s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"], **kw)
    assert set(got) == set(KEYS) and all(got[k].shape == (C, T) and got[k].device.type == "cpu" and got[k].dtype == torch.float32 for k in KEYS)
    # 1. the composition of the pieces, bit for bit
    comp, fields = _composition(s, max(1, dbf // ENS))
    for k in KEYS:
        assert _same_bits(got[k], comp[k]), k
    # 2. the oracle on the same decoded fields
    for l in range(T):
        want = S.ensemble_scores(fields[l], s["truth"][TRUTH_SLOTS[l]], s["clim"][s["clim_slots"][l]], s["lat_w"], sst_channel=SST)
        for k in KEYS:
            _close(got[k][:, l], want[k], 1e-5)
    assert all(torch.isfinite(got[k]).all() for k in KEYS)  # the SST channel averages over the sea points
    # 3. NaN fill and errors
    wide = score_latent_rollout(*args, s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"], total_num_steps=5, **kw)
    for k in KEYS:
        assert wide[k].shape == (C, 5) and _same_bits(wide[k][:, :T], got[k]) and bool(torch.isnan(wide[k][:, T:]).all())
    with pytest.raises(ValueError):
        score_latent_rollout(*args, s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"], total_num_steps=2, **kw)
    # 4. host-resident tables: only the needed planes are staged, the same bits
    host = score_latent_rollout(*args, s["truth"].numpy(), TRUTH_SLOTS, s["clim"], s["clim_slots"], s["lat_w"], **kw)
    for k in KEYS:
        assert _same_bits(host[k], got[k]), k
    with pytest.raises(ValueError):  # a slot outside the table, host or device
        score_latent_rollout(*args, s["truth"].numpy(), [2, 6, 3], s["clim"], s["clim_slots"], s["lat_w"], **kw)
    with pytest.raises(ValueError):
        score_latent_rollout(*args, s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), [2, 1, 5], s["lat_w"], **kw)


@pytest.mark.parametrize("in_memory", [False, True])
def test_cli_round_trip(setup, tmp_path, in_memory):
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
    lat2 = torch.randn(2, ENS, C_LAT, 1 + T, h, w, generator=gen)
    save_latent_npy(lat2, [INIT, 2020022900], str(tmp_path / "rollout"))  # the second one + 18 h is past the end date
    # frames from 2020-02-27 00 h, 6 h apart: INIT is frame 6, its leads are frames 7, 8, 9
    truth, full_slots, planes = _tables(gen, s["mean"], s["std"], 10)
    pole = lambda t: torch.cat([torch.full_like(t[..., :1, :], 1e9), t], dim=-2)  # noqa: E731  (an extra south-pole row, cropped)
    np.save(tmp_path / "truth.npy", pole(truth).numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H + 1, W))  # sparse: three planes written
    for i, slot in enumerate(full_slots):
        clim[slot // 4, slot % 4] = pole(planes[i]).numpy()
    clim.flush()
    del clim
    out_dir = tmp_path / "scores"
    argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
            "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
            "--end_date", "2020-02-29T12", "--output", str(out_dir), "--step_size_hour", "6", "--latent_spatial_scale", "8",
            "--total_lead_time_hour", "18", "--crop_init", "--force_ens_size", "2", "--decode_batch_frames", "4", "--sst_channel_idx", str(SST),
            "--variable_names", *names] + (["--load_ds_in_memory"] if in_memory else [])
    torch.manual_seed(1234)  # the CLI's from_config draws the weights make_dcae(seed=1234) draws, before its norm perturbation
    with pytest.warns(UserWarning):
        res = EG.main(argv)
    ts = str(INIT)
    for k in KEYS:
        assert np.load(out_dir / f"{ts}_{k}.npy").shape == (C, T) and np.load(out_dir / f"{k}.npy").shape == (1, C, T)
        assert not (out_dir / f"2020022900_{k}.npy").exists()
    stamp = np.load(out_dir / "timestamp.npy")
    assert stamp.dtype == np.float32 and stamp.tolist() == [float(np.float32(INIT))]
    assert len(list(out_dir.iterdir())) == 11
    # the values are the function's, on the model the command line built
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in s["mean"]]), torch.tensor([float(v) for v in s["std"]])
    want = EG.score_latent_rollout(str(tmp_path / "rollout" / f"latent_{ts}.npy"), model, mean32, std32, truth, [7, 8, 9], planes, [0, 1, 2],
                                   EG.lat_weights_for(H), sst_channel=SST, crop_init=True, force_ens_size=2, decode_batch_frames=4)
    for k in KEYS:
        assert _same_bits(torch.from_numpy(np.load(out_dir / f"{ts}_{k}.npy")), want[k]), k
        assert _same_bits(torch.from_numpy(res[k][0]), want[k]) and np.array_equal(np.load(out_dir / f"{k}.npy"), res[k], equal_nan=True)
        assert np.isfinite(res[k]).all()


@pytest.mark.parametrize("dbf", [3, 6])
def test_every_metric_at_once_is_each_metric_alone(setup, dbf):
    """every optional metric switched on in one call: each returned tensor is the bits (NaN pattern included) of the call with only
    that metric on, the five base scores are the bits of a call with none, and the key set is exactly the union; total_num_steps = 4
    leaves one column unwritten"""
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.energy import EnergyGroup
    from ladcast_amd.evaluate.regional import Region
    from ladcast_amd.evaluate.utils import Event

    s = setup
    args = (s["latents"], s["g"], s["mean"], s["std"], s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"])
    kw = dict(sst_channel=SST, crop_init=True, decode_batch_frames=dbf, total_num_steps=T + 1)
    events = [Event(0, "gt", float(s["mean"][0])), Event(SST, "lt", 0.0, True)]  # the second: an anomaly event on the SST channel
    regions = [Region("box", -20.0, 20.0, 30.0, 120.0), Region("across", 10.0, 60.0, 340.0, 20.0)]  # the second crosses 0 degrees east
    alone = dict(reliability=(dict(reliability=True), EG.RELIABILITY_KEYS),
                 spectrum=(dict(spectrum=True), EG.SPECTRUM_KEYS),
                 events=(dict(events=events), EG.EVENTS_KEYS),
                 fss=(dict(events=events, fss_radii=(0, 2)), EG.EVENTS_KEYS + EG.FSS_KEYS),
                 regional=(dict(regions=regions), EG.REGIONAL_KEYS),
                 energy=(dict(energy=True, energy_groups=[EnergyGroup("pair", (0, 1))]), EG.ENERGY_KEYS + EG.ENERGY_GROUP_NAMES))
    every = {}
    for opts, _ in alone.values():
        every.update(opts)
    got = EG.score_latent_rollout(*args, **every, **kw)
    plain = EG.score_latent_rollout(*args, **kw)
    assert set(plain) == set(KEYS)
    assert set(got) == set(KEYS).union(*(keys for _, keys in alone.values()))
    assert all(v.device.type == "cpu" for v in got.values())
    for k in KEYS:
        assert got[k].shape == (C, T + 1) and _same_bits(got[k], plain[k]), k
        assert bool(torch.isnan(got[k][:, T]).all()) and bool(torch.isfinite(got[k][:, :T]).all()), k
    for name, (opts, keys) in alone.items():
        one = EG.score_latent_rollout(*args, **opts, **kw)
        assert set(one) == set(KEYS) | set(keys), name
        for k in KEYS + tuple(keys):
            assert got[k].dtype == one[k].dtype and _same_bits(got[k], one[k]), (name, k)
