"""The two dataset-preparation command lines end to end on the tiny synthetic DC-AE (tests/synth.py), saved to a checkpoint directory:
raw .npy frames -> `compute_mean_std_era5` -> the normalisation JSON -> `encode_data` -> the latent store and the latent statistics JSON.

Five raw frames (9 channels: the last, the surface pressure, is dropped by the encoder; 49 rows: the first is cropped) with NaNs in the
SST channel, in two files (3 + 2) and batches of 2: a batch spans the files and the last one is ragged.  Statistics are held to the
accuracy rule of tests/preprocess_oracle.py against its exact-arithmetic oracle."""
import json

import numpy as np
import pytest
import torch

from tests import preprocess_oracle as PO
from tests.synth import make_dcae, rel_l2, synth_field, tiny_dcae_config

pytestmark = pytest.mark.gpu

SST = 7
LEVELS3 = [300, 500, 850]
NAMES8 = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]  # 2 x 3 levels + 2
NAMES9 = NAMES8 + ["surface_pressure"]


def _json_vectors(norm, names):
    """the JSON's float64 values in `mean_std_from_json`'s channel order"""
    mean, std = [], []
    for v in names:
        p = norm[v]
        if isinstance(p["mean"], dict):
            mean += list(p["mean"].values())
            std += [p["std"][k] for k in p["mean"]]
        else:
            mean.append(p["mean"])
            std.append(p["std"])
    return np.array(mean), np.array(std)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.preprocess import compute_mean_std_era5 as CM
    from ladcast_amd.preprocess import encode_data as ED

    tmp = tmp_path_factory.mktemp("prep")
    cfg = tiny_dcae_config()  # 8 fields + 5 static channels, 8 latent channels
    g = AutoencoderDC.from_config(cfg)
    g.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    g.save_pretrained(str(tmp / "DCAE"))
    gen = torch.Generator().manual_seed(5)
    scale = torch.tensor([900.0, 700.0, 500.0, 12.0, 9.0, 7.0, 15.0, 4.0, 800.0]).view(1, 9, 1, 1)
    shift = torch.tensor([9.0e4, 5.5e4, 1.4e4, 230.0, 255.0, 280.0, 285.0, 290.0, 9.8e4]).view(1, 9, 1, 1)
    frames = synth_field(5, 9, 49, 64, seed=50) * scale + shift
    land = torch.rand(49, 64, generator=gen) < 0.3
    frames[:, SST][:, land] = float("nan")
    frames = frames.numpy()
    np.save(tmp / "a.npy", frames[:3])
    np.save(tmp / "b.npy", frames[3:])
    np.save(tmp / "lsm.npy", synth_field(1, 1, 49, 64, seed=51)[0, 0].numpy())
    np.save(tmp / "oro.npy", (synth_field(1, 4, 49, 64, seed=52)[0] * 3.0 + 1.0).numpy())
    (tmp / "names8.json").write_text(json.dumps({"channel_names": NAMES8, "pressure_levels": LEVELS3, "num_atm_vars": 2}))
    (tmp / "names9.json").write_text(json.dumps({"channel_names": NAMES9, "pressure_levels": LEVELS3, "num_atm_vars": 2}))
    files = [str(tmp / "a.npy"), str(tmp / "b.npy")]
    CM.main(["--frames", *files, "--variable_names_json", str(tmp / "names9.json"), "--static", f"land_sea_mask={tmp / 'lsm.npy'}",
             f"orography={tmp / 'oro.npy'}", "--batch_size", "2", "--output", str(tmp / "norm.json")])
    latents = ED.main(["--frames", *files, "--normalization_json", str(tmp / "norm.json"), "--variable_names_json", str(tmp / "names8.json"),
                       "--encdec_model", str(tmp / "DCAE"), "--lsm_path", str(tmp / "lsm.npy"), "--orography_path", str(tmp / "oro.npy"),
                       "--batch_size", "2", "--sst_channel_idx", str(SST), "--output", str(tmp / "latents.npy"), "--latent_normal_json",
                       str(tmp / "latent_normal.json")])
    return dict(tmp=tmp, frames=frames, latents=latents, g=g.cuda().eval())


def test_normalization_json_meets_the_rule(run):
    from ladcast_amd.evaluate.track import mean_std_from_json

    with open(run["tmp"] / "norm.json") as f:
        norm = json.load(f)
    assert list(norm) == NAMES9 + ["land_sea_mask", "orography"] and list(norm["temperature"]["mean"]) == [str(p) for p in LEVELS3]
    want = PO.exact_moments(run["frames"])  # all 5 frames, all 49 rows
    mean, std = _json_vectors(norm, NAMES9)
    r = PO.worst_ratio(mean, std, want)
    print(f"\ncompute_mean_std_era5 on 5 frames in batches of 2: {r:.3g} of the rule's bound")
    assert r <= 1.0 and np.isfinite(mean[SST]) and want[SST]["n"] < want[0]["n"]  # the SST mean ignores the NaNs
    m32, s32 = mean_std_from_json(norm, NAMES9)
    assert np.array_equal(m32.numpy(), mean.astype(np.float32)) and np.array_equal(s32.numpy(), std.astype(np.float32))
    for name, path in (("land_sea_mask", "lsm.npy"), ("orography", "oro.npy")):  # a static file is one pooled variable
        w = PO.exact_channel(np.load(run["tmp"] / path))
        assert max(PO.rule_ratios(norm[name]["mean"], norm[name]["std"], w)) <= 1.0


@pytest.fixture(scope="module")
def by_hand(run):
    """preprocess_batch + vae.encode on the command line's batches (0-1, 2-3, 4), and one frame per call"""
    from ladcast_amd.evaluate.evaluate_encdec_model import preprocess_batch
    from ladcast_amd.evaluate.pred_rollout import build_static_conditioning
    from ladcast_amd.evaluate.track import mean_std_from_json

    with open(run["tmp"] / "norm.json") as f:
        mean, std = mean_std_from_json(json.load(f), NAMES8)
    static = build_static_conditioning(torch.from_numpy(np.load(run["tmp"] / "lsm.npy")), torch.from_numpy(np.load(run["tmp"] / "oro.npy"))).cuda().unsqueeze(0)
    raw = torch.from_numpy(run["frames"]).cuda()

    def encode(sl):
        x, _ = preprocess_batch(raw[sl], mean.cuda(), std.cuda(), crop_south_pole=True, sst_channel_idx=SST, incl_sur_pressure=False)
        assert not torch.isnan(x).any()
        with torch.no_grad():
            return run["g"].encode(x, static_conditioning_tensor=static).latent.cpu()

    batched = torch.cat([encode(slice(0, 2)), encode(slice(2, 4)), encode(slice(4, 5))])
    single = torch.cat([encode(slice(i, i + 1)) for i in range(5)])
    return batched, single


def test_latent_store(run, by_hand):
    batched, single = by_hand
    saved = np.load(run["tmp"] / "latents.npy")
    assert saved.shape == (5, 8, 6, 8) and saved.dtype == np.float32 and not np.isnan(saved).any()
    assert np.array_equal(saved.view(np.int32), run["latents"].view(np.int32))
    assert np.array_equal(saved.view(np.int32), batched.numpy().view(np.int32))  # bit-equal to the same batches encoded by hand
    # one frame per call (the reference's loop): the batch split moves a frame's result at fp32 rounding level only - the bound
    # tests/test_gpu_dcae.py::test_bulk_encoder_matches_frame_by_frame_oracle holds the batched encoder to
    e = rel_l2(torch.from_numpy(saved), single)
    print(f"\nencode_data, batches of 2 vs one frame per call: rel-L2 {e:.2e}")
    assert e < 1e-6


def test_latent_normal_json(run):
    from ladcast_amd.evaluate.pred_rollout import load_latent_transform_args

    args = load_latent_transform_args(str(run["tmp"] / "latent_normal.json"))
    assert set(args) == {"mean", "std", "target_std"} and len(args["mean"]) == len(args["std"]) == 8
    want = PO.exact_moments(run["latents"])
    r = PO.worst_ratio(args["mean"], args["std"], want)
    print(f"\nlatent statistics over 5 frames in batches of 2: {r:.3g} of the rule's bound")
    assert r <= 1.0 and all(w["n"] == 5 * 6 * 8 for w in want)
