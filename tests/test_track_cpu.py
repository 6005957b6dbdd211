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


# ---- the edge fixture: custom grids, off-grid centres, exact ties (tests/golden/make_track_golden.py --edges) ---------------
EDGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_edge_ref.npz")


@pytest.fixture(scope="module")
def edge():
    return dict(np.load(EDGE))


def edge_grid(edge, name):
    return edge[f"{name}_lat"], edge[f"{name}_lon"]


def edge_fields(edge, name):
    """the (F, H, W) fp32 planes of one grid; the planes of the 1024 x 1024 grid are rebuilt from the stored formulas"""
    if f"{name}_fields" in edge:
        return edge[f"{name}_fields"]
    lat, lon = edge_grid(edge, name)
    return np.stack([O.formula_field(lat.size, lon.size, *f) for f in edge[f"{name}_formulas"]])


def test_edge_fixture_holds_what_it_was_built_for(edge):
    names = [str(n) for n in edge["grid_names"]]
    assert names == ["G1", "G2", "G3", "G4a", "G4b", "G5", "G6"]
    shapes = [tuple(c.size for c in edge_grid(edge, n)) for n in names]
    assert shapes == [(120, 240), (21, 41), (37, 53), (1, 240), (120, 1), (120, 241), (1024, 1024)]
    assert edge["G5_lon"][0] == 0.0 and edge["G5_lon"][-1] == 360.0
    for gi, n in enumerate(names):
        found = edge["q_found"][edge["q_grid"] == gi]
        assert 0 < found.sum() < found.size, n  # both outcomes on every grid
        assert O.is_dyadic(*edge_grid(edge, n)) == (n not in ("G3", "G6")), n
    tie = (edge["q_ties"] >= 2) & (edge["q_found"] == 1)
    assert tie.sum() >= 12 and (tie & (edge["q_wrapped"] == 1)).sum() >= 3
    assert set(edge["q_inner"][edge["q_grid"] == names.index("G6")]) == {0, 1}
    assert {0, 1, 5, 12, 30} <= set(edge["q_inner"].tolist())
    assert os.path.getsize(EDGE) < 200e3


def test_oracle_equals_every_edge_query_and_the_key_preconditions_hold(edge):
    """tests/track_oracle.py on custom grids against the reference-made fixture, and - recomputed here - what the fixture's builder
    asserted about the distance keys: on dyadic grids and centres every d * d equals d ** 2; elsewhere the winner's key is either
    identical to a runner-up's under both or more than 4 ulp away"""
    names = [str(n) for n in edge["grid_names"]]
    cache = {n: (edge_grid(edge, n), edge_fields(edge, n)) for n in names}
    for q in range(edge["q_found"].size):
        (lat, lon), fields = cache[names[edge["q_grid"][q]]]
        center, inner = tuple(float(v) for v in edge["q_center"][q]), int(edge["q_inner"][q])
        fin = O.survivors(fields[edge["q_field"][q]], center, inner, lat, lon)
        n_min, problem = O.key_check(fin, center, O.is_dyadic(lat, lon, center))
        assert problem is None and n_min == edge["q_ties"][q], (q, problem, n_min)
        r = O.find_local_minimum(fields[edge["q_field"][q]], center, inner, lat, lon)
        if edge["q_found"][q]:
            assert r is not None, q
            assert (r[0], r[1]) == tuple(edge["q_latlon"][q]) and np.float32(r[2]).tobytes() == edge["q_value"][q].tobytes(), q
        else:
            assert r is None, q
    # the issue's own example: four candidates equally far from (0.75, 359.25), the seam's small longitude is visited first
    lat, lon = O.grid()
    assert O.find_local_minimum(np.full((120, 240), 7.0, np.float32), (0.75, 359.25), 1, lat, lon) == (0.0, 0.0, 7.0)


def test_oracle_equals_every_edge_track(edge):
    for i in range(int(edge["n_tracks"])):
        lat, lon = edge_grid(edge, str(edge[f"t{i}_grid"]))
        em = bool(edge[f"t{i}_enforce_msl"])
        mslp = edge[f"t{i}_mslp"]
        dyadic = O.is_dyadic(lat, lon)

        def search(field, center, inner, la, lo):
            _, problem = O.key_check(O.survivors(field, center, inner, la, lo), center, dyadic)
            assert problem is None, (i, center, inner, problem)
            return O.find_local_minimum(field, center, inner, la, lo)

        trk = O.track_first_n_steps(T0, *edge[f"t{i}_start"], mslp, mslp.shape[0] - 1, inner_box_sizes=list(edge[f"t{i}_boxes"]), enforce_msl=em,
                                    z700=edge.get(f"t{i}_z700"), land_sea_mask=edge.get(f"t{i}_lsm"), lat=lat, lon=lon, search=search)
        assert np.array_equal(np.array([(a, b) for _, a, b in trk]), edge[f"t{i}_track"]), i


def test_nearest_index_is_pandas_rule_on_custom_grids(edge):
    """midpoints of the regional grid (exact ties), the irregular grid, one-entry coordinates and points outside each of them"""
    import pandas as pd

    lat2, lon2 = edge_grid(edge, "G2")
    lat3, lon3 = edge_grid(edge, "G3")
    rng = np.random.default_rng(5)
    cases = [(lat2, np.concatenate([lat2[:-1] + 0.5, lat2, [-10.5, -11.0, 10.5, 95.0, -95.0]])),
             (lon2, np.concatenate([lon2[:-1] + 0.5, lon2, [99.5, 99.0, 140.5, -3.0, 363.0, 720.5]])),
             (lat3, np.concatenate([(lat3[:-1] + lat3[1:]) / 2, lat3, rng.uniform(-95, 95, 40), [-95.0, 95.0]])),
             (lon3, np.concatenate([(lon3[:-1] + lon3[1:]) / 2, lon3, rng.uniform(-5, 365, 40), [-3.0, 363.0, 720.5]])),
             (np.array([12.0]), np.array([11.0, 12.0, 13.0, -95.0, 95.0])), (np.array([181.5]), np.array([-3.0, 181.5, 363.0, 720.5]))]
    for coord, xs in cases:
        want = pd.Index(coord).get_indexer(xs, method="nearest")
        for x, w in zip(xs, want):
            assert O.nearest_index(coord, float(x)) == int(w), (coord.size, x)


def test_non_finite_centres_find_nothing(edge):
    """NaN, +inf, -inf in either coordinate: the oracle (as the reference's masks: every comparison with NaN is False; inf % 360 is NaN)
    returns None on every grid, which is what the GPU tests hold the kernel to"""
    bad = [float("nan"), float("inf"), float("-inf")]
    for name in ("G1", "G2", "G3", "G4a", "G4b", "G5"):
        lat, lon = edge_grid(edge, name)
        const = edge_fields(edge, name)[0]
        for b in bad:
            for center in ((b, float(lon[lon.size // 2])), (float(lat[lat.size // 2]), b), (b, b)):
                for inner in (0, 1, 30):
                    assert O.find_local_minimum(const, center, inner, lat, lon) is None, (name, center, inner)
        assert O.find_local_minimum(const, (float(lat[lat.size // 2]), float(lon[lon.size // 2])), 30, lat, lon) is not None, name
