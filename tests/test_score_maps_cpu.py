"""No device: the judge of tests/score_map_refs.py (the fp32 restatement of csrc/score_maps.hip stays inside the counted bound, is exact
on the integer tables, and every planted defect fails a table), the host functions of ladcast_amd.evaluate.score_maps on hand-made
sums, the parsing of the --map flags, and the second header of the C ABI."""
import argparse
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import score_map_refs as S


@pytest.fixture(scope="module")
def tables():
    return [(name, tab, ex, S.maps_ref(tab)) for name, tab, ex in S.cpu_tables()]


def test_the_restatement_stays_inside_the_bound_and_is_exact_on_integers(tables):
    for name, tab, ex, ref in tables:
        got = S.kernel_f32(tab)
        r = S.check(got, ref, name)
        print(f"{name}: worst err / bound {r:.4f}")
        if ex:
            assert S.exact(got, ref), name
            assert int(ref["counts"][:, :, 1].sum()) == 0 and int(ref["counts"][:, :, 0].sum()) > 0
    assert S.order_ok(S.kernel_f32(S.order_table()))


def test_the_tables_reach_what_they_are_for(tables):
    ref = {name: r for name, _, _, r in tables}
    n = ref["nan table"]["counts"]
    assert int(n[:, :, 1].sum()) > 0 and bool((n[:, :, 2] < n[:, :, 0]).any())  # invalid samples; valid ones that are not ACC-valid
    s = ref["nan table"]["sums"][0]
    assert bool(torch.isinf(s[:, :, 0]).any()) and bool(torch.isfinite(s[:, :, 0]).any())  # +inf is a value
    s, n = ref["no climatology"]["sums"][0], ref["no climatology"]["counts"]
    assert bool((s[:, :, 5:] == S.SENTINEL).all()) and bool((n[:, :, 2] == S.SENTINEL_N).all())
    t = S.integer_table(9, 1, 257)
    assert -1 in t["plane_of_lead"] and t["channel_idx"] != sorted(t["channel_idx"]) and len(t["calls"]) == 3
    assert sorted(p for p in t["plane_of_lead"] if p >= 0).count(1) == 2  # two leads of a call share plane 1


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_every_planted_defect_fails_a_table(tables, defect):
    failed = [name for name, tab, _, ref in tables if not S.passes(S.kernel_f32(tab, defect=defect), ref)]
    if not S.order_ok(S.kernel_f32(S.order_table(), defect=defect)):
        failed.append("order")
    print(f"{defect}: caught by {failed}")
    assert failed, defect


# ---- the host functions ---------------------------------------------------------------------------------------------------------------
def _hand_made():
    """one channel, one plane, 2 x 2 points: point (0, 0) two clean samples, (0, 1) one valid sample without climatology, (1, 0) none valid,
    (1, 1) one sample"""
    sums, counts = np.zeros((1, 1, 8, 2, 2)), np.zeros((1, 1, 3, 2, 2), dtype=np.int32)
    sums[0, 0, :, 0, 0] = [2.0, 10.0, 4.0, 6.0, 2.0, 3.0, 9.0, 4.0]
    counts[0, 0, :, 0, 0] = [2, 0, 2]
    sums[0, 0, :5, 0, 1] = [-1.0, 1.0, 0.25, 1.5, 0.5]
    counts[0, 0, :, 0, 1] = [1, 1, 0]
    counts[0, 0, :, 1, 0] = [0, 3, 0]
    sums[0, 0, :, 1, 1] = [0.5, 0.25, 1.0, 0.75, 0.5, -2.0, 4.0, 1.0]
    counts[0, 0, :, 1, 1] = [1, 0, 1]
    return sums, counts


def test_score_maps_on_hand_made_sums():
    from ladcast_amd.evaluate.score_maps import SCORE_MAP_NAMES, score_maps

    sums, counts = _hand_made()
    sc = score_maps(sums, counts, 3)
    assert set(sc) == set(SCORE_MAP_NAMES) and all(v.shape == (1, 1, 2, 2) for v in sc.values())
    at = lambda k, i, j: float(sc[k][0, 0, i, j])  # noqa: E731
    assert at("bias", 0, 0) == 1.0 and at("ens_mse", 0, 0) == 5.0 and at("rmse", 0, 0) == 5.0 ** 0.5 and at("ens_var", 0, 0) == 2.0
    assert at("ssr", 0, 0) == (4.0 / 3.0) ** 0.5 * (2.0 / 5.0) ** 0.5
    assert at("crps_skill", 0, 0) == 3.0 and at("crps_spread", 0, 0) == 1.0 and at("crps", 0, 0) == 2.5 and at("ens_acc", 0, 0) == 0.5
    assert at("bias", 0, 1) == -1.0 and np.isnan(at("ens_acc", 0, 1))  # valid without a climatology sample
    assert all(np.isnan(at(k, 1, 0)) for k in SCORE_MAP_NAMES if k != "n_valid") and sc["n_valid"][0, 0].tolist() == [[2, 1], [0, 1]]
    assert at("ens_acc", 1, 1) == -1.0
    assert np.isnan(score_maps(sums, counts, 1)["ssr"]).all()
    with pytest.raises(ValueError):
        score_maps(sums[:, :, :7], counts, 3)
    with pytest.raises(ValueError):
        score_maps(sums, counts, 0)


def test_regional_from_maps_on_hand_made_sums():
    from ladcast_amd.evaluate.regional import regional_scores
    from ladcast_amd.evaluate.score_maps import regional_from_maps

    sums, counts = _hand_made()
    sums[0, 0, :, 1, 0] = np.inf  # outside region 1: never added
    w = np.array([0.5, 2.0], dtype=np.float32)
    mask = np.array([[3, 1], [1, 3]], dtype=np.uint32)  # region 0: every point; region 1: (0, 0) and (1, 1)
    s, n = regional_from_maps(sums, counts, w, mask, 2)
    assert s.shape == (2, 1, 1, 10) and s.dtype == np.float64 and n.shape == (2, 1, 1, 3) and n.dtype == np.int64
    assert n[1, 0, 0].tolist() == [3, 0, 3] and n[0, 0, 0].tolist() == [4, 4, 3]
    want = [0.5 * 2 + 2.0 * 1, 0.5 * 2.0 + 2.0 * 0.5, 0.5 * 10 + 2.0 * 0.25, 0.5 * 4 + 2.0 * 1.0, 0.5 * 6 + 2.0 * 0.75, 0.5 * 2 + 2.0 * 0.5,
            0.5 * 2 + 2.0 * 1, 0.5 * 3 + 2.0 * -2.0, 0.5 * 9 + 2.0 * 4.0, 0.5 * 4 + 2.0 * 1.0]
    assert s[1, 0, 0].tolist() == want
    assert np.isinf(s[0, 0, 0, 1])  # region 0 holds the point
    sc = regional_scores(s[1:], n[1:], 3)
    assert float(sc["bias"][0, 0, 0]) == want[1] / want[0] and float(sc["weight"][0, 0, 0]) == 3.0
    with pytest.raises(ValueError):
        regional_from_maps(sums, counts, w[:1], mask, 2)
    with pytest.raises(ValueError):
        regional_from_maps(sums, counts, w, mask[:1], 2)
    with pytest.raises(ValueError):
        regional_from_maps(sums, counts, w, mask, 33)


def test_the_accumulator_checks_its_arguments():
    from ladcast_amd.evaluate.score_maps import ScoreMaps

    acc = ScoreMaps([3, 0], [0, -1, 1, 1], 2)
    assert acc.channels == [3, 0] and acc.n_init == 0 and acc.members is None and acc.sums is None
    for bad in (dict(channels=[]), dict(channels=[-1]), dict(channels=[0.5]), dict(plane_of_lead=[]), dict(plane_of_lead=[2]), dict(plane_of_lead=[-2]),
                dict(n_planes=0), dict(n_planes=65536)):
        with pytest.raises(ValueError):
            ScoreMaps(**dict(dict(channels=[0], plane_of_lead=[0], n_planes=2), **bad))
    with pytest.raises(RuntimeError):
        acc.download()


# ---- the flags ------------------------------------------------------------------------------------------------------------------------
def test_lead_hours_and_lead_bins_are_parsed():
    from ladcast_amd.evaluate.score_maps import parse_map_planes

    assert parse_map_planes(4, 6) == ([0, 1, 2, 3], [dict(lead_hours=[h]) for h in (6, 12, 18, 24)])
    assert parse_map_planes(4, 6, lead_hours=["24", "6"]) == ([1, -1, -1, 0], [dict(lead_hours=[24]), dict(lead_hours=[6])])
    pol, planes = parse_map_planes(6, 6, lead_bins=["6-12", "19-36"])
    assert pol == [0, 0, -1, 1, 1, 1] and planes == [dict(lead_hours=[6, 12], bin=[6, 12]), dict(lead_hours=[24, 30, 36], bin=[19, 36])]
    for kw in (dict(lead_hours=["6"], lead_bins=["6-12"]), dict(lead_hours=["7"]), dict(lead_hours=["30"]), dict(lead_hours=["0"]), dict(lead_hours=["6", "6"]),
               dict(lead_hours=["six"]), dict(lead_hours=[]), dict(lead_bins=["12-6"]), dict(lead_bins=["6"]), dict(lead_bins=["a-b"]), dict(lead_bins=["-6-12"]),
               dict(lead_bins=["7-11"]), dict(lead_bins=["6-12", "12-18"]), dict(lead_bins=["30-60"])):
        with pytest.raises(ValueError):
            parse_map_planes(4, 6, **kw)


def _args(argv):
    from ladcast_amd.evaluate.rollout_metrics import Maps

    ap = argparse.ArgumentParser()
    Maps.add_arguments(ap)
    ap.add_argument("--variable_names", nargs="+", default=["geopotential", "2m_temperature"])
    ap.add_argument("--levels", type=int, nargs="+", default=[500, 850])
    ap.add_argument("--num_atm_vars", type=int, default=1)
    ap.add_argument("--derive", nargs="+", action="append", default=[])
    ap.add_argument("--total_lead_time_hour", type=int, default=24)
    ap.add_argument("--step_size_hour", type=int, default=6)
    return ap.parse_args(argv)


def test_the_map_flags():
    from ladcast_amd.evaluate.rollout_metrics import METRICS, Maps, _channel_names

    assert METRICS[-1] is Maps
    assert Maps.from_args(_args([]), 4, []) is None
    names = _channel_names(_args([]))
    assert len(names) == 3
    m = Maps.from_args(_args(["--map", names[2], "0"]), 4, [])
    assert m.maps.channels == [2, 0] and m.names == [names[2], names[0]] and m.maps.plane_of_lead == [0, 1, 2, 3] and m.maps.n_planes == 4 and m.max_gib == 16.0
    m = Maps.from_args(_args(["--map", "all", "--map_lead_bins", "6-12", "18-24", "--map_max_gib", "0.5"]), 4, [])
    assert m.maps.channels == [0, 1, 2] and m.maps.plane_of_lead == [0, 0, 1, 1] and m.maps.n_planes == 2 and m.max_gib == 0.5
    m = Maps.from_args(_args(["--map", "1", "--derive", "thick", "diff", "0", "1", "--map", "thick"]), 4, [])  # a derived field is a channel
    assert m.maps.channels == [3] and m.names == ["thick"]
    for argv in (["--map_lead_hours", "6"], ["--map_lead_bins", "6-12"], ["--map", "nothing"], ["--map", "7"], ["--map", "0", "0"],
                 ["--map", "0", "--map_lead_hours", "6", "--map_lead_bins", "6-12"], ["--map", "0", "--map_lead_hours", "5"], ["--map", "0", "--map_max_gib", "0"]):
        with pytest.raises(ValueError):
            Maps.from_args(_args(argv), 4, [])
    # the guard: the bytes are printed and a run above the limit is refused before anything is decoded
    m = Maps.from_args(_args(["--map", "all", "--map_max_gib", "0.001"]), 4, [])
    assert m.maps.nbytes(120, 240) == 3 * 4 * 120 * 240 * 76
    with pytest.raises(ValueError, match="map_max_gib"):
        m.rollout_kwargs(120, 240, None, None)
    m.max_gib = 1.0
    assert m.rollout_kwargs(120, 240, None, None) == dict(score_maps=m.maps)
    assert Maps.for_rollout(dict(reliability=False)) is None  # an option dict from before the metric existed
    with pytest.raises(ValueError):
        Maps.for_rollout(dict(score_maps=object()))


# ---- the second header ----------------------------------------------------------------------------------------------------------------
def test_the_second_header():
    from ladcast_amd import abi

    assert os.path.basename(abi.EXT_HEADER_PATH) == "ladcast_hip_ext.h"
    with open(abi.EXT_HEADER_PATH) as f:
        text = f.read()
    constants, structs, signatures = abi.parse(text)  # every prototype parses (the reader raises on a statement it cannot split)
    assert structs == {} and signatures.keys() == abi.EXT_SIGNATURES.keys() and constants == abi.EXT_CONSTANTS
    assert set(signatures) == {"ldc_score_maps_bytes", "ldc_rollout_score_maps"}
    assert constants == dict(LDC_SCORE_MAPS_TERMS=8, LDC_SCORE_MAPS_COUNTS=3)
    assert not set(signatures) & set(abi.SIGNATURES) and not set(constants) & set(abi.CONSTANTS)
    assert len(abi.SIGNATURES) == 116 and len(abi.STRUCTS) == 9  # the first header's tables are what they were
    res, args = signatures["ldc_rollout_score_maps"]
    assert res is ctypes.c_int and len(args) == 27 and args[0] is ctypes.c_void_p and args[1] is ctypes.c_longlong and args[6] is ctypes.c_float
    assert signatures["ldc_score_maps_bytes"] == (ctypes.c_longlong, [ctypes.c_int] * 4)
    assert '#include "ladcast_hip.h"' in text and "LDC_ABI_VERSION" not in text.replace("LDC_ABI_VERSION (5)", "")  # stays at ABI 5: no version of its own


def test_the_library_exports_the_second_header():
    from ladcast_amd import abi, hip

    for name, (res, args) in abi.EXT_SIGNATURES.items():
        fn = getattr(hip.lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert hip.SIGNATURES is abi.SIGNATURES and not set(abi.EXT_SIGNATURES) & set(hip.SIGNATURES)
    assert hip.score_maps_bytes(84, 40, 120, 240) == 84 * 40 * 120 * 240 * 76 == 7354368000  # 7.4 GB: why the maps stay on the device
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (65536, 1, 1, 1), (1, 65536, 1, 1), (1, 1, 4097, 4096)):
        assert hip.score_maps_bytes(*bad) == 0, bad
    assert (hip.SCORE_MAPS_TERMS, hip.SCORE_MAPS_COUNTS) == (abi.EXT_CONSTANTS["LDC_SCORE_MAPS_TERMS"], abi.EXT_CONSTANTS["LDC_SCORE_MAPS_COUNTS"])
