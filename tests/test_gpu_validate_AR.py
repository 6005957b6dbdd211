"""The validation hook on the device (ladcast_amd.evaluate.log_validation; reference: train_AR.py:55-385).
(a) Against the reference's own code: tests/golden/validation_ref.npz holds the tables and the sampler call sequence the reference's
    `log_validation` produced over the IEEE-exact stand-ins of tests/validation_synth.py; the driver runs over the same stand-ins on the
    device.  Names, lead times and the (sampler_type, timestamp) sequence (quirk Q12) are equal, values agree at the project's 1e-5 (`_close`
    rule of tests/test_gpu_rollout_scores.py: the kernel sums in another order than torch).
(b) Wiring with the real tiny models: the per-initial-time buffers the chunked partial fills leave are the bits of ONE validation_scores
    launch over fields assembled by hand from ensemble_AR_sampler -> decode_latent_ens with the same decode batching; result shapes without
    CRPS / without the multistep chain; the command line."""
import json
import os
from datetime import timedelta

import numpy as np
import pytest
import torch

from tests import validation_synth as VS
from tests.synth import make_ar, make_dcae, tiny_ar_config, tiny_dcae_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, tol):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape and bool(torch.isfinite(a).all())
    assert ((a - b).abs() <= tol * (b.abs() + b.abs().mean())).all(), float(((a - b).abs() / (b.abs() + b.abs().mean())).max())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


# ---- (a) the reference's tables -------------------------------------------------------------------------------------------------------
class Tracker:
    def __init__(self):
        self.logged = []

    def log(self, tables):
        self.logged.append(tables)


def _run_standins(**kw):
    from ladcast_amd.evaluate import NpyLatentStore, log_validation

    sampler = VS.RecordingSampler()
    mean, std = VS.field_statistics()
    store = NpyLatentStore(VS.latent_frames().numpy(), VS.START, VS.STEP_HOURS)
    res = log_validation("validation", store, VS.CHANNEL_NAMES, None, mean, std, VS.T_IN, VS.R, VS.UpsampleDecoder("cuda"), VS.latent_transform,
                         VS.latent_inv_transform, timestamp_list=list(VS.INIT_TIMES), step_size_hour=VS.STEP_HOURS,
                         total_lead_time_hour=VS.T * VS.STEP_HOURS, ensemble_size=VS.ENS, num_inference_steps=VS.INFERENCE_STEPS, sampler=sampler, **kw)
    return res, sampler.calls


def test_tables_equal_the_reference_hook():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "validation_ref.npz"))
    tracker = Tracker()
    (rmse, crps), calls = _run_standins(eval_ms=True, eval_crps=True, return_df=True, trackers=[tracker])
    assert list(rmse.columns) == gold["rmse_columns"].tolist() and list(crps.columns) == gold["crps_columns"].tolist()
    assert rmse["lead time"].tolist() == gold["rmse_values"][:, 0].tolist() == [6, 12, 18, 24] and crps["lead time"].tolist() == [6, 12, 18, 24]
    assert [c[0] for c in calls] == gold["call_sampler_type"].tolist() and [c[1] for c in calls] == gold["call_timestamp"].tolist()
    _close(rmse.to_numpy(dtype=np.float64)[:, 1:], gold["rmse_values"][:, 1:], 1e-5)
    _close(crps.to_numpy(dtype=np.float64)[:, 1:], gold["crps_values"][:, 1:], 1e-5)
    (logged,) = tracker.logged
    assert set(logged) == {"merged_RMSE", "CRPS"} and logged["merged_RMSE"] is rmse and logged["CRPS"] is crps
    # without return_df nothing is returned, as in the reference; the rollout driver's timestamps on request
    res, calls2 = _run_standins(eval_ms=True, eval_crps=True, advance_by_chunk=True)
    assert res is None
    want = [int((t + timedelta(hours=step * VS.R * VS.STEP_HOURS)).strftime("%Y%m%d%H")) for t in VS.INIT_TIMES for step in range(VS.T // VS.R) for _ in range(2)]
    assert [c[1] for c in calls2] == want and want[2] == 2018010200 and [c[0] for c in calls2] == [c[0] for c in calls]


# ---- (b) the real tiny models ----------------------------------------------------------------------------------------------------------
ENS, T, R, STEPS, C_FIELD = 3, 4, 2, 3, 8
NAMES, LEVELS_B, N_ATM = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"], (300, 500, 850), 2
AR_CFG = tiny_ar_config()
# 8 fields + 5 static channels out of the AR model's 84 latent channels; widths in the full-size config's pattern (multiples of the 84 latent
# channels, so that every channel-regrouping shortcut divides)
DCAE_CFG = dict(tiny_dcae_config(), latent_channels=84, encoder_block_out_channels=(84, 84, 84, 168), decoder_block_out_channels=(84, 84, 84, 168))


@pytest.fixture(scope="module")
def real():
    from ladcast_amd.evaluate import NpyLatentStore
    from ladcast_amd.models import AutoencoderDC, LaDCastTransformer3DModel
    from ladcast_amd.pipelines.utils import get_inv_transform_3D, get_transform_3D

    ar = LaDCastTransformer3DModel.from_config(AR_CFG)
    ar.load_state_dict(make_ar(AR_CFG).state_dict(), strict=True)
    g = AutoencoderDC.from_config(DCAE_CFG)
    g.load_state_dict(make_dcae(DCAE_CFG).state_dict(), strict=True)
    gen = torch.Generator().manual_seed(51)
    frames = 0.5 * torch.randn(8, 84, 15, 30, generator=gen)
    mean, std = torch.randn(C_FIELD, generator=gen), torch.rand(C_FIELD, generator=gen) + 0.5
    targs = {"mean": (0.1 * torch.randn(84, generator=gen)).tolist(), "std": (torch.rand(84, generator=gen) + 0.5).tolist(), "target_std": 0.5}
    return dict(ar=ar.cuda().eval(), g=g.cuda().eval(), frames=frames, mean=mean, std=std, targs=targs, init=VS.START + timedelta(hours=12),
                store=NpyLatentStore(frames.numpy(), VS.START, 6), fwd=get_transform_3D("normalize", targs), inv=get_inv_transform_3D("normalize", targs))


def test_chunked_fills_equal_one_launch_over_hand_assembled_fields(real):
    from ladcast_amd.evaluate import get_normalized_lat_weights_based_on_cos, validate_initial_time, validation_scores
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, ensemble_AR_sampler
    from ladcast_amd.pipelines.utils import decode_latent_ens, inverse_normalize_transform_3D
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    s = real
    pipe = AutoRegressive2DPipeline(s["ar"], scheduler=EDMDPMSolverMultistepScheduler())
    mean_d, std_d = s["mean"].cuda(), s["std"].cuda()
    seen = {}
    got = validate_initial_time(s["init"], s["store"], pipe, s["g"], mean_d, std_d, 1, R, s["fwd"], s["inv"], total_num_steps=T, ensemble_size=ENS,
                                num_inference_steps=STEPS, eval_ms=True, decode_batch_frames=ENS, on_chunk=lambda n, k, x: seen.__setitem__((n, k), x.clone()))
    assert set(got) == {"EDM", "MS"} and all(b.shape == (3, C_FIELD, T) and b.is_cuda and bool(torch.isfinite(b).all()) for b in got.values())
    # by hand: the same chains, every lead time's members decoded in one decoder call (decode_batch_frames = ens), then ONE launch
    known = s["fwd"](s["frames"][2:3].cuda().permute(1, 0, 2, 3).contiguous()).unsqueeze(0)
    ref = s["frames"][3 : 3 + T].cuda()
    truth = torch.cat([s["g"].decode(ref[i : i + ENS]).sample for i in range(0, T, ENS)])
    truth = inverse_normalize_transform_3D(truth.unsqueeze(2), s["mean"], s["std"]).squeeze(2).permute(1, 0, 2, 3).contiguous()  # (C, T, H, W)
    w = get_normalized_lat_weights_based_on_cos(torch.from_numpy(np.linspace(-88.5, 90, 120))).float().cuda()
    for name, kind in (("EDM", "edm"), ("MS", "pipeline")):
        chain, fields = known, []
        for step in range(T // R):
            ts = torch.tensor([int((s["init"] + timedelta(hours=6 * step)).strftime("%Y%m%d%H"))]).cuda()
            smp = ensemble_AR_sampler(pipe, ENS, R, STEPS, known_latents=chain, timestamps=ts, sampler_type=kind, device="cuda")
            assert torch.equal(smp, seen[(name, step)]), (name, step)
            chain = smp[:, :, -1:].contiguous()
            lat = s["inv"](smp)
            fields += [decode_latent_ens(s["g"], lat[:, :, l : l + 1]) for l in range(R)]  # (ens, C, 1, H, W), still normalised
        one = validation_scores(torch.cat(fields, dim=2), truth, w, mean=mean_d, std=std_d)
        assert _same_bits(got[name], one._buffer), name
    assert not torch.equal(got["EDM"], got["MS"])


def test_result_shapes_without_crps_and_without_the_multistep_chain(real):
    from ladcast_amd.evaluate import log_validation

    s = real
    cols = [f"{v}_level{p}" for v in NAMES[:N_ATM] for p in LEVELS_B] + NAMES[N_ATM:]
    kw = dict(timestamp_list=[s["init"]], total_lead_time_hour=6 * T, ensemble_size=ENS, num_inference_steps=STEPS, levels=LEVELS_B, num_atm_vars=N_ATM,
              return_df=True)
    args = ("validation", s["store"], NAMES, s["ar"], s["mean"], s["std"], 1, R, s["g"], s["fwd"], s["inv"])
    rmse = log_validation(*args, eval_ms=False, eval_crps=False, **kw)  # a NameError in the reference (:321)
    assert list(rmse.columns) == ["lead time"] + [f"EDM_ens_{c}" for c in cols] + [f"EDM_single_{c}" for c in cols] and len(rmse) == T
    assert np.isfinite(rmse.to_numpy(dtype=np.float64)).all()
    rmse2, crps = log_validation(*args, eval_ms=False, eval_crps=True, **kw)
    assert list(crps.columns) == ["lead time"] + [f"CRPS_{c}" for c in cols] and crps.shape == (T, 1 + C_FIELD)
    assert rmse2.equals(rmse)  # the same seeds, the same chain: run to run the same bits
    ens, single = rmse.to_numpy()[:, 1 : 1 + C_FIELD], rmse.to_numpy()[:, 1 + C_FIELD :]
    assert (single > ens).all()
    with pytest.raises(ValueError, match="column names"):
        log_validation(*args, **dict(kw, num_atm_vars=1))


def test_command_line_writes_both_tables(real, tmp_path):
    import pandas as pd

    from ladcast_amd.evaluate import validate_AR as VA

    s = real
    lv = [str(p) for p in LEVELS_B]
    norm = {"geopotential": {"mean": {p: float(s["mean"][i]) for i, p in enumerate(lv)}, "std": {p: float(s["std"][i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {p: float(s["mean"][3 + i]) for i, p in enumerate(lv)}, "std": {p: float(s["std"][3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(s["mean"][6]), "std": float(s["std"][6])},
            "sea_surface_temperature": {"mean": float(s["mean"][7]), "std": float(s["std"][7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "names.json").write_text(json.dumps(NAMES))
    (tmp_path / "latent_normal.json").write_text(json.dumps({"mean": s["targs"]["mean"], "std": s["targs"]["std"]}))
    (tmp_path / "config.json").write_text(json.dumps(DCAE_CFG))
    s["ar"].save_pretrained(str(tmp_path / "ar"))
    np.save(tmp_path / "lat.npy", s["frames"].numpy())
    argv = ["--latent_path", str(tmp_path / "lat.npy"), "--start_date", "2018-01-01", "--init_times", "2018-01-01T12", "2018010118", "--ar_model",
            str(tmp_path / "ar"), "--encdec_model", str(tmp_path / "config.json"), "--latent_normal_json", str(tmp_path / "latent_normal.json"),
            "--normalization_json", str(tmp_path / "norm.json"), "--channel_names_json", str(tmp_path / "names.json"), "--ensemble_size", "2",
            "--num_inference_steps", "2", "--total_lead_time_hour", "12", "--return_seq_len", "1", "--levels", *lv, "--num_atm_vars", str(N_ATM),
            "--decode_batch_frames", "2", "--output", str(tmp_path / "val")]
    with pytest.warns(UserWarning):  # the autoencoder is a config.json alone: initial weights
        rmse, crps = VA.main(argv)
    cols = [f"{v}_level{p}" for v in NAMES[:N_ATM] for p in LEVELS_B] + NAMES[N_ATM:]
    assert list(rmse.columns) == ["lead time"] + [f"{a}_{b}_{c}" for a in ("EDM", "MS") for b in ("ens", "single") for c in cols]
    assert sorted(os.listdir(tmp_path / "val")) == ["CRPS.csv", "merged_RMSE.csv"]
    for df, name in ((rmse, "merged_RMSE.csv"), (crps, "CRPS.csv")):
        back = pd.read_csv(tmp_path / "val" / name)
        assert list(back.columns) == list(df.columns) and back["lead time"].tolist() == [6, 12]
        assert np.allclose(back.to_numpy(dtype=np.float64), df.to_numpy(dtype=np.float64), rtol=1e-12, atol=0) and np.isfinite(back.to_numpy()).all()
