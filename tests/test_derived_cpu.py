"""Derived fields without a device: the command-line parser, the file handling of `evaluate_ens_gpu.main` and `products.main` with
`--derive` (an injected scorer / products callable stands in for the autoencoder and the device), and the host reference
(tests/derived_refs.py) against itself."""
import json

import numpy as np
import pytest
import torch

from tests import derived_refs as R

SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
U10, V10, U850, V850, U200, V200 = ("10m_u_component_of_wind", "10m_v_component_of_wind", "u_component_of_wind_level850",
                                    "v_component_of_wind_level850", "u_component_of_wind_level200", "v_component_of_wind_level200")


def _names():
    from ladcast_amd.evaluate.products import column_names
    from ladcast_amd.evaluate.track import VARIABLE_NAMES

    return column_names(VARIABLE_NAMES)


# ---- a. parse_derived ------------------------------------------------------------------------------------------------------------------------
def test_parse_derived_by_name_and_by_index():
    from ladcast_amd.evaluate import Derived, parse_derived

    names = _names()
    assert len(names) == 84 and all(n in names for n in (U10, V10, U850, V850, U200, V200))
    got = parse_derived([["wind_speed_10m", "speed", U10, V10], ["thickness", "diff", "geopotential_level500", "geopotential_level1000"],
                         ["shear_200_850", "shear", U200, V200, U850, V850], ["by_index", "speed", "3", str(names.index(V10))]], names)
    ix = names.index
    assert got == [Derived("wind_speed_10m", "speed", (ix(U10), ix(V10))),
                   Derived("thickness", "diff", (ix("geopotential_level500"), ix("geopotential_level1000"))),
                   Derived("shear_200_850", "shear", (ix(U200), ix(V200), ix(U850), ix(V850))), Derived("by_index", "speed", (3, ix(V10)))]
    assert all(d.scale is None for d in got)
    assert parse_derived([["twice", "speed", U10, U10]], names)[0].channels == (ix(U10), ix(U10))  # both inputs of one field
    assert parse_derived([], names) == []


@pytest.mark.parametrize("entries", [
    [["w", "hypot", U10, V10]],  # an unknown kind
    [["w", "speed", U10]], [["w", "speed", U10, V10, U850]], [["w", "diff", U10]], [["w", "shear", U10, V10]], [["w", "shear", U10, V10, U850, V850, U200]],
    [["w", "speed"]], [["w"]],
    [["w", "speed", U10, V10], ["w", "diff", U10, V10]],  # a name that repeats
    [[U10, "speed", U10, V10]],  # a decoded channel's name
    [[f"w{k}", "speed", U10, V10] for k in range(17)],  # more than 16 fields
    [["w", "speed", U10, V10], ["x", "diff", "w", U10]],  # a channel that resolves to a derived name
    [["w", "speed", U10, "84"]], [["w", "speed", U10, "no_such_channel"]], [["w", "speed", U10, "-1"]],
])
def test_parse_derived_refuses(entries):
    from ladcast_amd.evaluate import parse_derived

    with pytest.raises(ValueError):
        parse_derived(entries, _names())


def test_sixteen_fields_pass_and_metadata():
    from ladcast_amd.evaluate import Derived, derived_metadata, parse_derived
    from ladcast_amd.evaluate.derived import field_scales

    names = _names()
    assert len(parse_derived([[f"w{k}", "speed", U10, V10] for k in range(16)], names)) == 16
    fields = [Derived("speed", "speed", (0, 1)), Derived("d", "diff", (2, 4), 7.5), Derived("sh", "shear", (0, 1, 5, 6))]
    std = torch.arange(1.0, 9.0)
    assert field_scales(fields, std) == [np.sqrt(1.0 + 4.0), 7.5, np.sqrt(1.0 + 4.0 + 36.0 + 49.0)]
    meta = derived_metadata(fields, [f"c{i}" for i in range(8)], std)
    assert meta[2] == dict(name="sh", kind="shear", channels=[0, 1, 5, 6], channel_names=["c0", "c1", "c5", "c6"], index=10, scale=np.sqrt(90.0))
    assert [m["index"] for m in meta] == [8, 9, 10]
    assert [m["scale"] for m in derived_metadata(fields, [f"c{i}" for i in range(8)])] == [None, 7.5, None]  # no std: only a scale given by hand


# ---- b. evaluate_ens_gpu.main ----------------------------------------------------------------------------------------------------------------
DERIVE = ["--derive", "wind_speed_10m", "speed", U10, V10, "--derive", "thickness", "diff", "geopotential_level500", "geopotential_level1000",
          "--derive", "shear", "shear", U200, V200, U850, V850]


def _run_main(tmp_path, name, extra, rows):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    if not res.exists():
        res.mkdir()
        for ts in (2018123000, 2018123106):
            np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    T, M = 4, 1

    def score(path, time_str, t_slots, c_slots):
        out = {k: np.full((rows, T), 1.0 + i, dtype=np.float32) for i, k in enumerate(SCORES)}
        n_ev = sum(1 for a in extra if a in ("--event", "--event_anomaly"))
        if n_ev:
            out.update(event_hist=torch.ones(n_ev, T, M + 1, 2, dtype=torch.int32), event_hist_weighted=torch.ones(n_ev, T, M + 1, 2),
                       event_n_invalid=torch.zeros(n_ev, T, dtype=torch.int32))
        return out

    out_dir = tmp_path / name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + extra, score=score)
    return out_dir, out


def test_main_derive_adds_rows_and_derived_json(tmp_path):
    names = _names()
    C, D = len(names), 3
    plain, _ = _run_main(tmp_path, "plain", [], C)
    out_dir, out = _run_main(tmp_path, "derived", DERIVE + ["--event", "wind_speed_10m", "gt", "17.2", "--event", "shear", "lt", "5",
                                                           "--event_anomaly", "thickness", "gt", "10"], C + D)
    assert "derived.json" not in [p.name for p in plain.iterdir()]
    for k in SCORES:
        assert np.load(out_dir / f"{k}.npy").shape == (2, C + D, 4) and out[k].shape == (2, C + D, 4)
        assert np.load(out_dir / f"2018123000_{k}.npy").shape == (C + D, 4)
    meta = json.loads((out_dir / "derived.json").read_text())
    assert meta["decoded_channels"] == C and [m["name"] for m in meta["derived"]] == ["wind_speed_10m", "thickness", "shear"]
    ix = names.index
    assert meta["derived"][0] == dict(name="wind_speed_10m", kind="speed", channels=[ix(U10), ix(V10)], channel_names=[U10, V10], index=C, scale=None)
    assert meta["derived"][2]["channels"] == [ix(U200), ix(V200), ix(U850), ix(V850)] and meta["derived"][2]["index"] == C + 2
    ev = json.loads((out_dir / "events.json").read_text())["events"]
    assert [(e["channel"], e["channel_index"], e["anomaly"]) for e in ev] == [("wind_speed_10m", C, False), ("shear", C + 2, False), ("thickness", C + 1, True)]


def test_main_derive_refusals(tmp_path):
    names = _names()
    C = len(names)
    with pytest.raises(ValueError, match="anomaly"):  # the climatology of a speed is not the speed of the climatology
        _run_main(tmp_path, "bad", DERIVE + ["--event_anomaly", "wind_speed_10m", "gt", "5"], C + 3)
    with pytest.raises(ValueError, match="anomaly"):
        _run_main(tmp_path, "bad", DERIVE + ["--event_anomaly", str(C + 2), "gt", "5"], C + 3)
    with pytest.raises(ValueError, match="SST"):  # a field that reads the nanmean channel
        _run_main(tmp_path, "bad", ["--derive", "d", "diff", "sea_surface_temperature", "2m_temperature"], C + 1)
    with pytest.raises(ValueError, match="SST"):
        _run_main(tmp_path, "bad", ["--derive", "d", "diff", U10, V10, "--sst_channel_idx", str(names.index(V10))], C + 1)
    with pytest.raises(ValueError):
        _run_main(tmp_path, "bad", ["--derive", "d", "norm", U10, V10], C + 1)
    with pytest.raises(ValueError):  # an event on a name that no --derive made
        _run_main(tmp_path, "bad", ["--event", "wind_speed_10m", "gt", "17.2"], C)


def test_library_refusals_need_no_device():
    from ladcast_amd.evaluate.derived import Derived, check_scoring_fields, _field_list
    from ladcast_amd.evaluate.utils import Event

    fields = [Derived("s", "speed", (0, 1)), Derived("d", "diff", (2, 4))]
    check_scoring_fields(fields, 8, 3, [Event(8, "gt", 1.0), Event(9, "gt", 1.0, True), Event(0, "gt", 1.0, True)])  # fine
    with pytest.raises(ValueError):
        check_scoring_fields(fields, 8, 3, [Event(8, "gt", 1.0, True)])
    with pytest.raises(ValueError):
        check_scoring_fields(fields, 8, 4)
    for bad in ([], [("s", "speed", (0, 8))], [("s", "speed", (0,))], [("s", "hypot", (0, 1))], [("s", "speed", (0, 1))] * 17, [("s", "speed", (0, 1), -1.0)]):
        with pytest.raises(ValueError):
            _field_list(bad, 8)


# ---- c. products.main ------------------------------------------------------------------------------------------------------------------------
def test_products_main_with_derive(tmp_path):
    from ladcast_amd.evaluate import products as P
    from ladcast_amd.pipelines.io import save_latent_npy

    names = _names()
    C = len(names)
    ENS, T, H, W = 4, 2, 3, 5
    save_latent_npy(torch.zeros(1, ENS, 2, 1 + T, 2, 2), [2020010100], str(tmp_path / "rollout"))
    stub = lambda path, time_str: dict({n: torch.zeros(2, T, H, W) for n in P.PRODUCT_STAT_NAMES}, exceed=torch.zeros(1, 2, T, H, W))  # noqa: E731
    argv = ["--result_path", str(tmp_path / "rollout"), "--output", str(tmp_path / "products")]
    meta = P.main(argv + DERIVE[:5] + ["--channels", "wind_speed_10m", "2m_temperature", "--exceed", "wind_speed_10m", "gt", "17.2"], products=stub)
    assert meta["channels"] == ["wind_speed_10m", "2m_temperature"] and meta["channel_indices"] == [C, names.index("2m_temperature")]
    assert meta["thresholds"] == [dict(channel="wind_speed_10m", channel_index=C, direction="gt", threshold=17.2)]
    assert meta["derived"] == [dict(name="wind_speed_10m", kind="speed", channels=[names.index(U10), names.index(V10)], channel_names=[U10, V10], index=C, scale=None)]
    assert json.loads((tmp_path / "products" / "products.json").read_text()) == meta
    all_meta = P.main(argv + DERIVE, products=lambda p, t: {n: torch.zeros(C + 3, T, H, W) for n in P.PRODUCT_STAT_NAMES})
    assert len(all_meta["channels"]) == C + 3 and all_meta["channels"][C:] == ["wind_speed_10m", "thickness", "shear"]
    assert "derived" not in P.main(argv, products=lambda p, t: {n: torch.zeros(C, T, H, W) for n in P.PRODUCT_STAT_NAMES})
    with pytest.raises(ValueError):
        P.main(argv + ["--exceed", "wind_speed_10m", "gt", "17.2"], products=stub)  # no --derive: no such channel
    with pytest.raises(ValueError):
        P.main(argv + ["--derive", "w", "speed", U10], products=stub)


# ---- d. the reference against itself ---------------------------------------------------------------------------------------------------------
def test_reference_speed_is_hypot_and_shear_its_difference_form():
    g = np.random.default_rng(11)
    a, b, c, d = (g.standard_normal(4096).astype(np.float32) * s for s in (10.0, 3.0, 7.0, 1e-3))
    want = np.hypot(a.astype(np.float64), b.astype(np.float64)).astype(np.float32)
    got = R.field("speed", a, b)
    assert got.dtype == np.float32 and int(R.ulp_distance(got, want).max()) <= 1  # hypot and sqrt of the exact squares' sum: both faithful in double
    assert int((got != want).sum()) <= 4
    sh = R.field("shear", a, b, c, d)
    want = np.hypot(a.astype(np.float64) - c, b.astype(np.float64) - d).astype(np.float32)
    assert int(R.ulp_distance(sh, want).max()) <= 1
    assert np.array_equal(R.field("diff", a, b), a - b) and R.field("diff", a, b).dtype == np.float32


def test_reference_extremes():
    big, tiny, nan, inf = np.float32(1e30), np.float32(1e-30), np.float32("nan"), np.float32("inf")
    s = R.field("speed", np.array([big, -big, tiny, 0.0, nan, 1.0, nan, inf, -inf], dtype=np.float32), np.array([big, big, tiny, -0.0, 1.0, nan, nan, 1.0, nan], dtype=np.float32))
    assert np.isfinite(s[:4]).all() and abs(float(s[0]) / 1e30 - np.sqrt(2.0)) < 1e-6 and s[0] == s[1]
    assert float(s[2]) > 1.4e-30 and s[3] == 0.0
    assert np.isnan(s[4:7]).all() and s[7] == inf and np.isnan(s[8])  # sqrt(inf + NaN) is NaN: the formula, not hypot's special case
    sh = R.field("shear", *(np.array([v], dtype=np.float32) for v in (big, -big, -big, big)))
    assert np.isfinite(sh).all() and abs(float(sh[0]) / 1e30 - 2.0 * np.sqrt(2.0)) < 1e-6  # the differences are 2e30: fp32 squares would overflow
    assert np.isnan(R.field("shear", *(np.array([v], dtype=np.float32) for v in (1.0, 1.0, nan, 1.0)))).all()
    assert np.isnan(R.field("diff", np.array([inf], dtype=np.float32), np.array([inf], dtype=np.float32))).all()


def test_reference_denormalises_as_inv_norm_rounds():
    g = np.random.default_rng(12)
    x = g.standard_normal((2, 3, 5)).astype(np.float32)
    mean, std = np.array([1.5, -2.0, 0.25], dtype=np.float32), np.array([0.7, 1.3, 2.1], dtype=np.float32)
    one = R.derive(x, [("d", "diff", (0, 2))], 1, mean, std)
    a = (x[:, 0] * std[0]).astype(np.float32) + mean[0]
    b = (x[:, 2] * std[2]).astype(np.float32) + mean[2]
    assert one.shape == (2, 1, 5) and np.array_equal(one[:, 0], (a - b).astype(np.float32))
    t = R.derive(x, [("d", "diff", (0, 2))], 1, mean, std, target_std=0.5)
    a = ((x[:, 0] / np.float32(0.5)).astype(np.float32) * std[0]).astype(np.float32) + mean[0]
    b = ((x[:, 2] / np.float32(0.5)).astype(np.float32) * std[2]).astype(np.float32) + mean[2]
    assert np.array_equal(t[:, 0], (a - b).astype(np.float32))
    assert np.array_equal(R.derive(x, [("d", "diff", (0, 2))], 1)[:, 0], x[:, 0] - x[:, 2])  # no mean: physical already
    assert R.ulp_distance(np.float32([0.0, 1.0, np.nan]), np.float32([-0.0, np.nextafter(np.float32(1), np.float32(2)), np.nan])).tolist() == [0, 1, 0]
