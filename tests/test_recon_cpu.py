"""CPU checks of the DC-AE reconstruction evaluation: the float64 restatement (tests/recon_oracle.py) against the reference's own
outputs (tests/golden/recon_ref.npz), the new C ABI entries, and the CSV naming / year grouping of the real command-line path with a
stub in place of the device scorer."""
import csv
import json

import numpy as np
import pytest
import torch

from tests import recon_oracle as RO


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/recon_ref.npz")


def test_restated_preprocess_is_bit_equal_to_the_reference(ref):
    for i, shape in enumerate(RO.PRE_SHAPES):
        x, mean, std = RO.pre_inputs(shape, seed=100 + i)
        assert np.array_equal(x.numpy(), ref[f"pre{i}_x"], equal_nan=True) and np.array_equal(mean.numpy(), ref[f"pre{i}_mean"])
        for crop in (0, 1):
            for keep in (0, 1):
                C = shape[1] - (0 if keep else 1)
                y, mask = RO.preprocess(x, mean[:C], std[:C], bool(crop), RO.PRE_SST, bool(keep))
                want = ref[f"pre{i}_c{crop}k{keep}_y"]
                assert y.shape == want.shape == (shape[0], C, shape[2] - crop, shape[3])
                assert np.array_equal(y.numpy().view(np.int32), want.view(np.int32)) and np.array_equal(mask.numpy(), ref[f"pre{i}_c{crop}k{keep}_mask"])
        m = ref[f"pre{i}_c0k1_mask"]
        if shape[0] > 1:  # one SST plane all NaN, one without any
            assert m[0].all() and not m[1].any()


@pytest.mark.parametrize("name", list(RO.SCORE_CASES))
def test_restated_scores_reproduce_the_reference(ref, name):
    """fp32 point values + float64 sums against the reference's fp32 outputs, at the 1e-5 `_close` bound of the GPU tests"""
    d = RO.score_inputs(name)
    assert torch.equal(RO.checksum(d), torch.from_numpy(ref[f"{name}_checksum"])), "the seeded inputs differ from the fixture's"
    if RO.SCORE_CASES[name]["stored"]:
        for k in ("pred", "target", "mask", "w", "mean", "std"):
            assert np.array_equal(d[k].numpy(), ref[f"{name}_{k}"]), k
    rel, absn, lw = RO.scores(d["pred"], d["target"], d["static"], d["mask"], d["sst"], d["w"], d["mean"], d["std"])
    RO.close(rel, ref[f"{name}_rel"], 1e-5, "rel")
    RO.close(absn, ref[f"{name}_abs"], 1e-5, "abs")
    RO.close(lw, ref[f"{name}_lw"], 1e-5, "lw_mse")
    RO.close(rel.mean(dim=0, keepdim=True).mean(dim=1)[0], ref[f"{name}_loss"], 1e-5, "loss")
    keep = [c for c in range(rel.shape[1]) if c != RO.ZERO]
    RO.close(rel[:, keep].mean(dim=0, keepdim=True).mean(dim=1)[0], ref[f"{name}_loss_finite"], 1e-5, "loss without the zero channel")
    want_rel = ref[f"{name}_rel"]
    assert np.isinf(want_rel[-1, RO.ZERO]) and (want_rel.shape[0] == 1 or np.isnan(want_rel[0, RO.ZERO]))  # the zero-target pattern is there
    if d["pred"][0, 0].numel() * d["pred"].shape[0] == 1:  # a single point: nothing to sum, bit-equal
        assert np.array_equal(lw.float().numpy().view(np.int32), ref[f"{name}_lw"].view(np.int32))


def test_binding_declares_the_recon_entries():
    from ladcast_amd import hip

    for name in ("ldc_recon_preprocess", "ldc_recon_scores", "ldc_recon_scores_workspace_bytes"):
        assert name in hip.SIGNATURES and hasattr(hip.lib, name)
    assert hip.ABI_VERSION == 5
    # one record of 4 floats per (plane, chunk of whole rows, ~1024 points)
    assert hip.lib.ldc_recon_scores_workspace_bytes(2, 12, 33, 68) == 2 * 12 * 3 * 16
    assert hip.lib.ldc_recon_scores_workspace_bytes(2, 89, 120, 240) == 2 * 89 * 30 * 16
    assert hip.lib.ldc_recon_scores_workspace_bytes(1, 2, 1, 1) == 32 and hip.lib.ldc_recon_scores_workspace_bytes(0, 2, 1, 1) == 0


def test_cli_names_columns_and_groups_by_year(tmp_path):
    """the real `main`: argument parsing, .npy batching, per-year grouping, the reference's column names and order, the CSV file"""
    from ladcast_amd.evaluate import evaluate_encdec_model as EM

    settings = {"channel_names": ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"], "static_names": ["land_sea_mask"],
                "pressure_levels": [500, 850], "num_atm_vars": 2, "num_sur_vars": 2}
    (tmp_path / "settings.json").write_text(json.dumps(settings))
    (tmp_path / "norm.json").write_text("{}")
    np.save(tmp_path / "a.npy", np.full((5, 7, 3, 4), 1.0, dtype=np.float32))
    np.save(tmp_path / "b.npy", np.full((2, 7, 3, 4), 3.0, dtype=np.float32))
    seen = []

    def stub(batches):
        sizes = [tuple(b.shape) for b in batches]
        seen.append(sizes)
        n = sum(s[0] for s in sizes)
        return float(n), torch.arange(7, dtype=torch.float32) + 0.5 * n

    csv_path = tmp_path / "out.csv"
    rows = EM.main(["--frames", f"2018={tmp_path / 'a.npy'}", f"2021={tmp_path / 'b.npy'}", "--normalization_json", str(tmp_path / "norm.json"),
                    "--settings_json", str(tmp_path / "settings.json"), "--batch_size", "2", "--csv_path", str(csv_path)], evaluate=stub)
    assert seen == [[(2, 7, 3, 4), (2, 7, 3, 4), (1, 7, 3, 4)], [(2, 7, 3, 4)]]  # one call per year, the last batch smaller
    with open(csv_path) as f:
        got = list(csv.reader(f))
    assert got[0] == ["year", "val_loss_fn_loss", "val_lw_rmse_geopotential_level_500", "val_lw_rmse_geopotential_level_850",
                      "val_lw_rmse_temperature_level_500", "val_lw_rmse_temperature_level_850", "val_lw_rmse_2m_temperature",
                      "val_lw_rmse_sea_surface_temperature", "val_lw_rmse_land_sea_mask"]
    assert len(got) == 3 and [r[0] for r in got[1:]] == ["2018", "2021"]
    assert [float(v) for v in got[1][1:]] == [5.0] + [c + 2.5 for c in range(7)] and [float(v) for v in got[2][1:]] == [2.0] + [c + 1.0 for c in range(7)]
    assert rows[0]["val_lw_rmse_land_sea_mask"] == 8.5
    # the reference's defaults: 6 variables x 13 levels + 6 surface variables
    cols = EM.rmse_column_names({"channel_names": [f"v{i}" for i in range(12)], "static_names": ["lsm", "oro"]})
    assert len(cols) == 6 * 13 + 6 + 2 and cols[0] == "val_lw_rmse_v0_level_50" and cols[78] == "val_lw_rmse_v6" and cols[-1] == "val_lw_rmse_oro"
    with pytest.raises(ValueError):
        EM.yearly_rows([("2018", lambda: [])], lambda b: (0.0, torch.zeros(3)), settings)  # channel count and names disagree
    with pytest.raises(SystemExit):
        EM.main(["--frames", "2018", "--normalization_json", "x", "--settings_json", str(tmp_path / "settings.json"), "--csv_path", str(csv_path)], evaluate=stub)


def test_lat_weights_match_the_reference_grid():
    from ladcast_amd.evaluate import evaluate_encdec_model as EM

    lat = np.linspace(-88.5, 90, 120)  # evaluate_encdec_model.py:144-145
    w = np.cos(np.deg2rad(lat))
    assert np.array_equal(EM.equiangular_lat_weights(121, True).numpy(), (w / w.mean()).astype(np.float32))
    assert torch.equal(EM.equiangular_lat_weights(49, True), RO.lat_weights(49, True))
