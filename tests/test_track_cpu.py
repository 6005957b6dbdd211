"""CPU checks of the cyclone tracker (ladcast_amd/evaluate/track.py): the numpy restatement tests/track_oracle.py against the
fixture made by the reference's own tracking code (tests/golden/make_track_golden.py), round_to_grid, the kernel's restatement of
Python's `%`, the CSV round trip through the reference's loaders, and argument refusal."""
import math
import os
from datetime import datetime

import numpy as np
import pytest

from tests import track_oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_ref.npz")
T0 = datetime(2018, 10, 1, 0)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_grid_is_the_reference_grid(gold):
    from ladcast_amd.evaluate import track as TR

    assert np.array_equal(gold["lat"], TR.latitude_grid()) and np.array_equal(gold["lon"], TR.longitude_grid())
    assert TR.latitude_grid().shape == (120,) and TR.longitude_grid().shape == (240,) and TR.latitude_grid().dtype == np.float64
    assert TR.MSLP_CHANNEL == 81 and TR.Z700_CHANNEL == 9 and TR.GRID_RES == TR.NEIGHBOR_DEG == 1.5
    assert TR.VARIABLE_NAMES[9] == "mean_sea_level_pressure" and len(TR.VARIABLE_NAMES) == 12


def test_oracle_equals_every_fixture_query(gold):
    for q in range(gold["q_found"].size):
        f = gold["q_fields"][gold["q_field_idx"][q]]
        r = O.find_local_minimum(f, tuple(gold["q_center"][q]), int(gold["q_inner"][q]))
        if gold["q_found"][q]:
            assert r is not None, q
            assert (r[0], r[1]) == tuple(gold["q_latlon"][q]) and np.float32(r[2]) == gold["q_value"][q], q
        else:
            assert r is None, q
    assert 0 < gold["q_found"].sum() < gold["q_found"].size  # both outcomes are pinned


def test_oracle_equals_every_fixture_track(gold):
    for i in range(int(gold["n_tracks"])):
        em = bool(gold[f"t{i}_enforce_msl"])
        mslp = gold[f"t{i}_mslp"]
        trk = O.track_first_n_steps(T0, *gold[f"t{i}_start"], mslp, mslp.shape[0] - 1, inner_box_sizes=list(gold[f"t{i}_boxes"]),
                                    enforce_msl=em, z700=gold.get(f"t{i}_z700"), land_sea_mask=gold.get(f"t{i}_lsm"))
        assert np.array_equal(np.array([(a, b) for _, a, b in trk]), gold[f"t{i}_track"]), i
    mem = gold["ens_members"]
    for e in range(mem.shape[0]):
        trk = O.track_first_n_steps(T0, *gold["ens_start"], mem[e], mem.shape[1] - 1)
        assert np.array_equal(np.array([(a, b) for _, a, b in trk]), gold["ens_tracks"][e]), e
    mean = O.nanmean_members(mem)
    assert np.array_equal(mean, gold["ens_mean_field"], equal_nan=True)
    trk = O.track_first_n_steps(T0, *gold["ens_start"], mean, mem.shape[1] - 1)
    assert np.array_equal(np.array([(a, b) for _, a, b in trk]), gold["ens_mean_track"])


def test_nanmean_is_a_sequential_member_sum(gold):
    """what ldc_track_nanmean computes: NaN -> 0, fp32 sum in member order, one division by the count"""
    x = gold["ens_members"]
    acc = np.where(np.isnan(x[0]), np.float32(0), x[0])
    for e in range(1, x.shape[0]):
        acc = acc + np.where(np.isnan(x[e]), np.float32(0), x[e])
    cnt = (~np.isnan(x)).sum(axis=0)
    with np.errstate(invalid="ignore"):
        seq = (acc / cnt.astype(np.float32)).astype(np.float32)
    assert np.array_equal(seq, O.nanmean_members(x), equal_nan=True)


def test_nearest_index_is_pandas_rule():
    """the oracle's (and the kernel's) nearest lookup of the land-sea mask against pandas' own get_indexer(method="nearest")"""
    import pandas as pd

    lat, lon = O.grid()
    xs = [-95.0, -90.0, -89.25, -88.5, -87.75, -0.75, 0.0, 0.75, 1.0, 89.25, 90.0, 90.75, 95.0, 179.25, 358.5, 359.25, 360.0, 361.0]
    for coord in (lat, lon):
        for x in xs:
            assert O.nearest_index(coord, x) == int(pd.Index(coord).get_indexer([x], method="nearest")[0]), x


def test_round_to_grid_half_to_even(gold):
    from ladcast_amd.evaluate.track import round_to_grid

    for v, want in zip(gold["round_in"], gold["round_out"]):
        assert round_to_grid(v) == want and O.round_to_grid(v) == want
    assert round_to_grid(0.75) == 0.0 and round_to_grid(2.25) == 3.0 and round_to_grid(3.75) == 3.0  # 0.5, 1.5, 2.5 steps
    assert round_to_grid(359.4) == 360.0  # no % 360 at the start: lon0 can be 360.0


def test_python_mod_restatement_over_edge_values():
    from ladcast_amd.evaluate.track import py_mod_restated

    vals = [0.0, -0.0, 1e-300, -1e-300, 5e-324, -5e-324, 1e-17, -1e-17, 359.99999999999994, -359.99999999999994, 360.0, -360.0, 720.0,
            -720.0, 180.0, -180.0, 1.5, -1.5, 358.5, -358.5, 361.5, -361.5, 1e18, -1e18, 0.1, -0.1, 355.5 - 2.25, -4.5, 364.5]
    for x in vals:
        for m in (360.0, -360.0, 1.5):
            got, want = py_mod_restated(x, m), x % m
            assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want), (x, m, got, want)


def test_csv_round_trip_through_the_reference_loaders(tmp_path):
    from ladcast_amd.evaluate.track import load_ensemble_mean, load_ensemble_members, save_tracks_csv
    from datetime import timedelta

    trk = lambda la, lo: [(T0 + timedelta(hours=6 * k), la + 1.5 * k, (lo + 3.0 * k) % 360) for k in range(5)]  # noqa: E731
    ens = {"M0": trk(15.0, 352.5), "M2": trk(16.5, 355.5), "M10": trk(-88.5, 0.0)}
    mean = trk(15.0, 354.0)
    mcsv, acsv = str(tmp_path / "ladcast_members.csv"), str(tmp_path / "ladcast_mean.csv")
    save_tracks_csv(ens, mean, mcsv, acsv)
    assert open(mcsv).readline().strip() == "time,lat,lon,member,step"
    assert open(acsv).readline().strip() == "time,lat,lon,step,member"
    back = load_ensemble_members(mcsv)
    assert set(back) == set(ens)
    for k, v in ens.items():
        assert [(t.to_pydatetime(), la, lo) for t, la, lo in back[k]] == v
    assert [(t.to_pydatetime(), la, lo) for t, la, lo in load_ensemble_mean(acsv)] == mean


def test_caps_and_validation():
    import torch

    from ladcast_amd.evaluate import track as TR

    for bad in ([], [7, 4, 31], [-1], [2.5], list(range(9))):
        with pytest.raises(ValueError):
            TR._check_boxes(bad)
    assert TR._check_boxes([7, 4, 1]) == [7, 4, 1] and TR._check_boxes([30] * 8) == [30] * 8
    with pytest.raises(ValueError):
        TR._grid("cpu", np.array([0.0, 2.0, 1.0]), None)  # not ascending
    with pytest.raises(ValueError):
        TR._grid("cpu", None, np.arange(2000.0))  # over the grid cap
    # host tensors are refused before anything else (no CPU fallback)
    f = torch.zeros(3, 120, 240)
    with pytest.raises(RuntimeError):
        TR.track_first_n_steps(T0, 15.0, 150.0, f, n_steps=2)
    with pytest.raises(RuntimeError):
        TR.find_local_minimum(f[0], (15.0, 150.0), 7)
    with pytest.raises(RuntimeError):
        TR.find_local_minima(f, [(15.0, 150.0)], [7])
