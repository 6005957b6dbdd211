"""`evaluate_reconstruction` and its command line on the tiny synthetic DC-AE (tests/synth.py) with static channels, against the CPU
oracle DC-AE forward fed through the float64 restatement of the reference's loss math (tests/recon_oracle.py, pinned to the reference's
outputs by tests/test_recon_cpu.py).

Band: a reconstruction is an encode followed by a decode of the encoder's OWN latent, so it carries both halves' errors; the band is the
sum of the fp32 ceilings that tests/precision_bands.py holds the tiny DC-AE's encode and decode to (`tiny_dcae_encode` + `tiny_dcae_decode`),
applied as a relative L2 distance to the (B-weighted) per-channel RMSE vector and as a relative distance to the scalar loss - both are
first-order in the reconstruction's error, and the statistics are O(1) so that un-normalising does not amplify it."""
import csv
import json

import numpy as np
import pytest
import torch

from tests import recon_oracle as RO
from tests.precision_bands import ceiling
from tests.synth import make_dcae, rel_l2, synth_field, tiny_dcae_config

pytestmark = pytest.mark.gpu

SST = 3
BAND = ceiling("tiny_dcae_encode") + ceiling("tiny_dcae_decode")


@pytest.fixture(scope="module")
def setup():
    from ladcast_amd.models import AutoencoderDC

    cfg = tiny_dcae_config()  # 8 fields + 5 static channels
    o = make_dcae(cfg)
    g = AutoencoderDC.from_config(cfg)
    g.load_state_dict(o.state_dict(), strict=True)
    g = g.cuda().eval()
    gen = torch.Generator().manual_seed(21)
    mean, std = torch.randn(8, generator=gen), torch.rand(8, generator=gen) + 0.5
    frames = []
    for i, B in enumerate((2, 1)):  # two batches of different size; raw frames: 9 channels (the last is dropped), 49 rows (the first is cropped)
        x = synth_field(B, 9, 49, 64, seed=30 + i) * torch.cat([std, torch.ones(1)]).view(1, 9, 1, 1) + torch.cat([mean, torch.zeros(1)]).view(1, 9, 1, 1)
        land = torch.rand(49, 64, generator=gen) < 0.3
        x[:, SST][:, land] = float("nan")
        frames.append(x)
    static_raw = synth_field(1, 5, 48, 64, seed=1)[0] * 3.0 + 1.0
    w = RO.lat_weights(49, True)

    def forward(x, static):
        with torch.no_grad():
            return o(x, static_conditioning_tensor=static, return_static=True).sample

    want = RO.evaluate(forward, frames, mean, std, static_raw, w, SST)
    return dict(g=g, frames=frames, mean=mean, std=std, static_raw=static_raw, w=w, want=want)


def test_evaluate_reconstruction_matches_oracle(setup):
    from ladcast_amd.evaluate.evaluate_encdec_model import evaluate_reconstruction

    s = setup
    loss, rmse = evaluate_reconstruction(s["g"], s["frames"], s["mean"], s["std"], s["static_raw"], s["w"], sst_channel_idx=SST)
    want_loss, want_rmse = s["want"]
    e_rmse, e_loss = rel_l2(rmse, want_rmse), abs(loss - want_loss) / abs(want_loss)
    print(f"\nevaluate_reconstruction, tiny DC-AE [fp32]: val_loss_fn_loss {loss:.6g} (oracle {want_loss:.6g}, rel {e_loss:.2e}), "
          f"val_lw_rmse rel-L2 {e_rmse:.2e}; band {BAND:.2e}")
    assert rmse.shape == (13,) and rmse.device.type == "cpu" and np.isfinite(loss)
    assert e_rmse < BAND and e_loss < BAND, (e_rmse, e_loss, BAND)
    loss2, rmse2 = evaluate_reconstruction(s["g"], [f.cuda() for f in s["frames"]], s["mean"].cuda(), s["std"].cuda(), s["static_raw"].cuda(), s["w"].cuda(),
                                           sst_channel_idx=SST)
    assert loss2 == loss and torch.equal(rmse2, rmse)  # device inputs, a second run: the same bits


def test_cli_round_trip(setup, tmp_path):
    from ladcast_amd.evaluate import evaluate_encdec_model as EM

    s = setup
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    settings = {"channel_names": names, "static_names": [f"static{i}" for i in range(5)], "pressure_levels": [300, 500, 850], "num_atm_vars": 2,
                "num_sur_vars": 2}
    norm = {"geopotential": {"mean": {str(p): float(s["mean"][i]) for i, p in enumerate((300, 500, 850))},
                             "std": {str(p): float(s["std"][i]) for i, p in enumerate((300, 500, 850))}},
            "temperature": {"mean": {str(p): float(s["mean"][3 + i]) for i, p in enumerate((300, 500, 850))},
                            "std": {str(p): float(s["std"][3 + i]) for i, p in enumerate((300, 500, 850))}},
            "2m_temperature": {"mean": float(s["mean"][6]), "std": float(s["std"][6])},
            "sea_surface_temperature": {"mean": float(s["mean"][7]), "std": float(s["std"][7])}}
    (tmp_path / "settings.json").write_text(json.dumps(settings))
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    np.save(tmp_path / "y0.npy", torch.cat(s["frames"]).numpy())  # 3 frames: batches of 2 + 1
    np.save(tmp_path / "y1.npy", s["frames"][1].numpy())
    np.save(tmp_path / "static.npy", torch.cat([s["static_raw"][:, :1], s["static_raw"]], dim=1).numpy())  # (5, 49, 64): the first row is cropped
    torch.manual_seed(1234)  # the CLI's from_config draws the weights make_dcae(seed=1234) draws, before its norm perturbation
    csv_path = tmp_path / "eval.csv"
    with pytest.warns(UserWarning):
        rows = EM.main(["--frames", f"2018={tmp_path / 'y0.npy'}", f"2019={tmp_path / 'y1.npy'}", "--normalization_json", str(tmp_path / "norm.json"),
                        "--settings_json", str(tmp_path / "settings.json"), "--encdec_model", str(tmp_path / "config.json"), "--static_path",
                        str(tmp_path / "static.npy"), "--sst_channel_idx", str(SST), "--batch_size", "2", "--csv_path", str(csv_path)])
    with open(csv_path) as f:
        got = list(csv.DictReader(f))
    cols = EM.rmse_column_names(settings)
    assert list(got[0].keys()) == ["year", "val_loss_fn_loss"] + cols and len(cols) == 13 and [r["year"] for r in got] == ["2018", "2019"]
    assert cols[0] == "val_lw_rmse_geopotential_level_300" and cols[6] == "val_lw_rmse_2m_temperature" and cols[-1] == "val_lw_rmse_static4"
    # the values are the function's, on the model the CLI built
    from ladcast_amd.models import AutoencoderDC

    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in s["mean"]]), torch.tensor([float(v) for v in s["std"]])
    for row, frames in zip(got, (s["frames"], s["frames"][1:])):
        loss, rmse = EM.evaluate_reconstruction(model, frames, mean32, std32, s["static_raw"], EM.equiangular_lat_weights(49, True), sst_channel_idx=SST)
        assert float(row["val_loss_fn_loss"]) == loss and [float(row[c]) for c in cols] == [float(v) for v in rmse]
    assert rows[0]["year"] == "2018"
