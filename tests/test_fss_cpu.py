"""CPU proofs for the neighbourhood verification kernel (csrc/fss.hip) - no GPU:
  a. the vectorised oracle of tests/fss_refs.py equals the definitions written as loops, bit for bit, on every tiny table; every case has
     contributing centres, windows clipped at a pole and windows whose N is reduced by invalid neighbours; the kernel's reduction order,
     restated in float64, meets the COUNTED bound; every planted defect fails the tables
  b. `fss_scores`: r = 0 against `event_scores`' Brier score, the perfect forecast, `useful_scale` on a hand-made table, the NaN rules
  c. the command line: `--fss_scales` parsing, the files `main` writes, pooling over initial times
  d. the wrappers' argument errors, raised before the device check
  e. the library exports and the workspace formula"""
import json
import math

import numpy as np
import pytest
import torch

from tests import events_refs as ER
from tests import fss_refs as R


def ref_of(c):
    return R.fss_ref(c["x"], c["t"], c["w"], c["events"], c["radii"], c["cl"])


CASES = dict(R.cpu_cases())


# ---- a. oracle, bound, planted defects ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if "17x33" not in n or "M=9 " in n or "M=65 " in n])  # the largest grid: two M suffice
def test_oracle_equals_the_definitions_as_loops(name):
    c = CASES[name]
    ref, brute = ref_of(c), R.fss_brute(c["x"], c["t"], c["w"], c["events"], c["radii"], c["cl"])
    assert np.array_equal(ref["sums"][0], brute["sums"]) and np.array_equal(ref["n_invalid"], brute["n_invalid"])


def test_case_tables_cover_the_window_situations():
    assert {c[0] for c in R.INT_CASES} == {1, 8, 9, 64, 65, 130} and {c[1:] for c in R.INT_CASES} == {(5, 7), (16, 16), (17, 33), (3, 50)}
    for name, c in CASES.items():
        H, W = c["x"].shape[2:]
        rs = c["radii"]
        assert set(rs) >= {0, 1, 2, (W - 1) // 2} and all(2 * r + 1 <= W for r in rs), name
        ref = ref_of(c)
        assert (ref["contributing"] > 0).all(), name  # every (event, radius) has contributing centres
        assert (ref["clipped"][:, 1:] > 0).all() and (ref["clipped"][:, 0] == 0).all(), name  # r >= 1: windows lose rows at a pole
        assert (ref["reduced"][1, 1:] > 0).all(), name  # channel 1's land block and NaN member reduce N below the window size
        assert ref["n_invalid"][1] > 0 and ref["n_invalid"][0] == 0, name
        assert R.passes(dict(sums=ref["sums"][0], n_invalid=ref["n_invalid"]), ref)  # the reference alone passes its own bound
    assert any(r >= c["x"].shape[2] for c in CASES.values() for r in c["radii"])  # a window taller than the grid: every row
    assert R.integer_case(9, 3, 50)["radii"] == (0, 1, 2, 3, 24)
    # the seam feature: the truth shows event 0 on columns W - 1 | 0, the forecast on 0 | 1
    for H, W in R.INT_GRIDS:
        n, o, valid, _ = R.classify(*(R.integer_case(9, H, W)[k] for k in ("x", "t", "cl")), R.INT_EVENTS[0])
        mid = H // 2
        assert o[mid, W - 1] == o[mid, 0] == 1 and o[mid, 1] == 0 and n[mid, 0] == n[mid, 1] == 9 and n[mid, W - 1] == 0
        assert o[0].sum() > 0 and o[H - 1].sum() > 0  # features in the first and the last row


def test_clean_restatement_meets_every_bound():
    for name, c in CASES.items():
        got = R.kernel_f64(c["v"], c["t"], c["w"], c["events"], c["radii"], c["cl"])
        r = R.check(got, ref_of(c), name)
        assert r <= 1.0, name


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for name, c in CASES.items():
        if "M=9 " not in name and "special" not in name:
            continue  # the window logic does not depend on M: one M of the table and the special fields
        got = R.kernel_f64(c["v"], c["t"], c["w"], c["events"], c["radii"], c["cl"], defect=defect)
        if not R.passes(got, ref_of(c)):
            caught.append(name)
    assert caught, f"{defect}: no case of the tables fails"
    print(f"{defect}: caught by {len(caught)} cases")


def test_special_fields():
    from ladcast_amd.evaluate import fss_scores

    c = R.special_case("perfect")
    ref = ref_of(c)
    s = ref["sums"][0]
    assert (s[..., 5] == 0.0).all() and np.array_equal(s[..., 1], s[..., 2]) and np.array_equal(s[..., 3], s[..., 4])
    sc = fss_scores(s)
    events_seen = s[..., 3] > 0
    assert events_seen.any() and (sc["fss"][events_seen] == 1.0).all()
    s = ref_of(R.special_case("all_event"))["sums"][0]
    assert np.array_equal(s[..., 0], s[..., 1]) and np.array_equal(s[..., 0], s[..., 2]) and (fss_scores(s)["fss"] == 1.0).all()
    s = ref_of(R.special_case("no_event"))["sums"][0]
    assert (s[..., 1:] == 0.0).all() and (s[..., 0] > 0).all() and np.isnan(fss_scores(s)["fss"]).all()


# ---- b. the host scores ------------------------------------------------------------------------------------------------------------------
def test_fss_scores_radius_zero_is_the_brier_score():
    """r = 0: N = 1, Pf = n / M, Po = o, so s5 = sum w (n / M - o)^2 and s5 / s0 is the Brier score `event_scores` derives from the
    weighted histogram of the same case (float64 weights here: the two agree to the rounding of two float64 sums)"""
    from ladcast_amd.evaluate import event_scores, fss_scores

    for M, H, W in ((9, 5, 7), (65, 16, 16)):
        c = R.integer_case(M, H, W)
        ref = R.fss_ref(c["x"], c["t"], c["w"], c["events"], (0,), c["cl"])
        ev = ER.events_ref(c["x"], c["t"], c["w"], c["events"], c["cl"])
        assert np.array_equal(ref["n_invalid"], ev["n_invalid"].numpy())
        hw = ev["hist_w"][0].numpy()
        brier = event_scores(hw)["brier"]
        s = ref["sums"][0][:, 0]
        assert np.allclose(s[:, 5] / s[:, 0], brier, rtol=64 * H * W * 2.0 ** -53, atol=0)
        assert np.allclose(s[:, 0], hw.sum((-1, -2)), rtol=H * W * 2.0 ** -53, atol=0)
        # and to the last bit against the same sum taken term by term
        for e, evd in enumerate(c["events"]):
            n, o, valid, _ = R.classify(c["x"], c["t"], c["cl"], evd)
            w = np.broadcast_to(c["w"].float().double().numpy().reshape(H, 1), (H, W))[valid]
            d = n[valid] / (np.float64(M) * 1.0) - o[valid] / 1.0
            assert s[e, 5] == math.fsum((w * d) * d)
        sc = fss_scores(ref["sums"][0])
        assert np.array_equal(sc["obs_fraction"], s[None, :, 2].T / s[None, :, 0].T)


def test_fss_scores_useful_scale_and_nan_rules():
    from ladcast_amd.evaluate import FSS_SCORE_NAMES, fss_scores

    # (S = 3, L = 4, 6): obs_fraction 0.2 -> target 0.6; fss per (scale, lead)
    fss = np.array([[0.1, 0.7, 0.3, np.nan], [0.59, 0.2, 0.6, np.nan], [0.9, 0.9, 0.2, np.nan]])
    s = np.zeros((3, 4, 6))
    s[..., 0], s[..., 1], s[..., 2] = 10.0, 3.0, 2.0
    s[..., 3], s[..., 4] = 1.0, 1.0
    s[..., 5] = np.where(np.isnan(fss), 0.0, (1.0 - fss) * 2.0)
    s[:, 3, 3:5] = 0.0  # no event at lead 3: denominator 0
    sc = fss_scores(s, radii=(5, 1, 9))
    assert set(FSS_SCORE_NAMES) <= set(sc) and sc["fss"].shape == (3, 4)
    assert np.allclose(sc["fss"][:, :3], fss[:, :3], rtol=1e-15) and np.isnan(sc["fss"][:, 3]).all()
    assert np.array_equal(sc["fss_target"], np.full((3, 4), 0.5 + (2.0 / 10.0) / 2)) and np.array_equal(sc["freq_bias"], np.full((3, 4), 1.5))
    assert np.array_equal(sc["fcst_fraction"], np.full((3, 4), 0.3))
    # lead 0: scale 9 only (0.59 < 0.6); lead 1: scales 5 and 9 -> 5; lead 2: scale 1 exactly on the target; lead 3: none
    assert sc["useful_scale"].tolist() == [9, 5, 1, -1] and sc["useful_scale"].dtype == np.int64
    assert "useful_scale" not in fss_scores(s)
    zero = fss_scores(np.zeros((2, 6)))
    assert all(np.isnan(zero[k]).all() for k in FSS_SCORE_NAMES)
    with pytest.raises(ValueError):
        fss_scores(np.zeros((3, 5)))
    with pytest.raises(ValueError):
        fss_scores(s, radii=(1, 2))


# ---- c. the command line -----------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
FSS_FILES = ("event_fss_sums", "event_fss_n_invalid", "event_fss", "event_fss_target", "event_fss_obs_fraction", "event_fss_freq_bias",
             "event_fss_useful_scale")


def test_parse_fss_scales():
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    assert EG.parse_fss_scales(["0", "3", "10"]) == [0, 3, 10] and EG.parse_fss_scales(["7"]) == [7]
    assert EG.parse_fss_scales([str(r) for r in range(16)]) == list(range(16))
    for bad in (["1.5"], ["a"], ["-1"], ["2", "2"], [], [str(r) for r in range(17)]):
        with pytest.raises(ValueError):
            EG.parse_fss_scales(bad)


def _run_main(tmp_path, name, extra, fss=True):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    if not res.exists():
        res.mkdir()
        for ts in (2018123000, 2018123106):
            np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    C, T, E, S, M = 3, 4, 2, 3, 3
    g = np.random.default_rng(7)
    per_init = []

    def score(path, time_str, t_slots, c_slots):
        out = {k: np.full((C, T), 1.0 + i, dtype=np.float32) for i, k in enumerate(SCORES)}
        h = g.integers(0, 50, (E, T, M + 1, 2)).astype(np.int32)
        out.update(event_hist=torch.from_numpy(h), event_hist_weighted=torch.from_numpy(h.astype(np.float32)),
                   event_n_invalid=torch.zeros((E, T), dtype=torch.int32))
        if fss:
            s = g.uniform(0.5, 1.5, (E, S, T, 6))
            per_init.append(s)
            out.update(event_fss_sums=torch.from_numpy(s), event_fss_n_invalid=torch.full((E, T), len(per_init), dtype=torch.int32))
        return out

    out_dir = tmp_path / name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + extra, score=score)
    return out_dir, out, per_init


def test_main_fss_scales_writes_the_fss_files(tmp_path):
    from ladcast_amd.evaluate import fss_scores

    ev = ["--event", "2m_temperature", "gt", "303.15", "--event_anomaly", "geopotential_level500", "lt", "-50"]
    plain, _, _ = _run_main(tmp_path, "plain", ev, fss=False)
    with_fss, out, per_init = _run_main(tmp_path, "fss", ev + ["--fss_scales", "4", "0", "9"])
    before = sorted(p.name for p in plain.iterdir())
    assert sorted(p.name for p in with_fss.iterdir()) == sorted(before + [f"{k}.npy" for k in FSS_FILES])
    a = {k: np.load(with_fss / f"{k}.npy") for k in FSS_FILES}
    E, S, T = 2, 3, 4
    assert len(per_init) == 2 and np.array_equal(a["event_fss_sums"], per_init[0] + per_init[1]) and a["event_fss_sums"].dtype == np.float64
    assert a["event_fss_n_invalid"].shape == (2, E, T) and a["event_fss_n_invalid"].dtype == np.int32 and (a["event_fss_n_invalid"][1] == 2).all()
    sc = fss_scores(a["event_fss_sums"], [4, 0, 9])
    for f, k in (("event_fss", "fss"), ("event_fss_target", "fss_target"), ("event_fss_obs_fraction", "obs_fraction"), ("event_fss_freq_bias", "freq_bias")):
        assert a[f].shape == (E, S, T) and a[f].dtype == np.float64 and np.array_equal(a[f], sc[k]) and np.array_equal(a[f], out[f]), f
    assert a["event_fss_useful_scale"].shape == (E, T) and a["event_fss_useful_scale"].dtype == np.int64
    assert np.array_equal(a["event_fss_useful_scale"], sc["useful_scale"])
    meta = json.loads((with_fss / "events.json").read_text())
    assert meta["fss_radii"] == [4, 0, 9] and meta["fss_width_deg"] is None and len(meta["events"]) == 2  # an injected scorer: no grid known
    assert "fss_radii" not in json.loads((plain / "events.json").read_text())


def test_main_fss_scales_refuses_bad_entries(tmp_path):
    ev = ["--event", "0", "gt", "1", "--event", "1", "lt", "0"]
    with pytest.raises(ValueError, match="--fss_scales needs --event"):
        _run_main(tmp_path, "bad", ["--fss_scales", "1"])
    for bad in (["-2"], ["1", "1"], ["x"]):
        with pytest.raises(ValueError):
            _run_main(tmp_path, "bad", ev + ["--fss_scales"] + bad)
    with pytest.raises(ValueError, match="--fss_scales needs"):  # a scorer that does not return the fss arrays
        _run_main(tmp_path, "bad", ev + ["--fss_scales", "1"], fss=False)


# ---- d. the wrappers' argument errors --------------------------------------------------------------------------------------------------
_M, _C, _L, _H, _W = 2, 1, 1, 3, 8


def _call(*, forecast=None, weight=None, events=((0, "gt", 0.5),), radii=(0, 1), **kw):
    from ladcast_amd import evaluate as E

    x = torch.zeros(_M, _C, _L, _H, _W) if forecast is None else forecast
    t, w = torch.zeros(_C, _L, _H, _W), torch.ones(_H) if weight is None else weight
    return E.rollout_fss(x, t, w, events, radii, **kw)


def test_rollout_fss_argument_errors_come_before_the_device_check():
    from ladcast_amd.evaluate import Event, empty_fss

    cases = [
        (dict(forecast=torch.zeros(_M, _C, _H, _W)), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(forecast=torch.zeros(_M, _C, _L, _H, _W, dtype=torch.float64)), NotImplementedError, "fp32 only"),
        (dict(mean=torch.zeros(_C)), ValueError, "mean and std go together"),
        (dict(weight=torch.ones(_H + 1)), ValueError, "lat_weight must have one value per latitude row"),
        (dict(events=[(0, "gt", float("nan"))]), ValueError, "NaN"),
        (dict(events=[(0, "ge", 0.5)]), ValueError, "direction"),
        (dict(events=[Event(0, "gt", 0.5, True)]), ValueError, "climatology"),
        (dict(events=[(1, "gt", 0.5)]), ValueError, "channel"),
        (dict(events=[]), ValueError, "events"),
        (dict(radii=[]), ValueError, "radii"),
        (dict(radii=list(range(17))), ValueError, "radii"),
        (dict(radii=[-1]), ValueError, "negative"),
        (dict(radii=[1.5]), ValueError, "whole numbers"),
        (dict(radii=[4]), ValueError, "wider"),  # 2 r + 1 = 9 > W = 8
        (dict(l_off=-1), ValueError, "l_off"),
        (dict(out=dict(a=1)), ValueError, "out must be"),
        (dict(out=empty_fss(1, 3, 1, "cpu")), ValueError, "out must be"),  # another number of radii
        (dict(out=empty_fss(1, 2, 1, "cpu"), l_off=1), ValueError, "out must be"),  # no room
    ]
    for kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            _call(**kw)
    with pytest.raises(RuntimeError, match="device tensors"):  # nothing wrong but the host tensors
        _call(radii=[0, 3])  # 2 r + 1 = 7 <= 8 is served; r = 3 >= H too
    d = empty_fss(2, 3, 4, "cpu")
    assert d["event_fss_sums"].shape == (2, 3, 4, 6) and d["event_fss_sums"].dtype == torch.float64
    assert d["event_fss_n_invalid"].shape == (2, 4) and d["event_fss_n_invalid"].dtype == torch.int32


def test_score_latent_rollout_refuses_fss_radii_without_events():
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    with pytest.raises(ValueError, match="fss_radii needs events"):
        EG.score_latent_rollout(torch.zeros(2, 1, 1, 2, 2), None, None, None, torch.zeros(3, 1, 4, 4), [0], None, None, torch.ones(4), fss_radii=[1])


# ---- e. the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_workspace():
    from ladcast_amd import hip
    from ladcast_amd.evaluate import utils as eu

    for name in ("ldc_rollout_fss", "ldc_rollout_fss_workspace_bytes"):
        assert hasattr(hip.lib, name) and name in hip.SIGNATURES
    assert hip.FSS_SCALES_MAX == eu.MAX_FSS_SCALES == R.MAX_SCALES == 16 and hip.FSS_SUMS == R.NT == len(eu.FSS_SUM_NAMES)
    assert hip.lib.ldc_abi_version() == 5
    wb = hip.lib.ldc_rollout_fss_workspace_bytes
    for M, E, S, L, H, W in ((5, 3, 2, 2, 3, 50), (64, 1, 1, 1, 16, 16), (65, 2, 16, 1, 17, 33), (1024, 32, 4, 4, 120, 240), (64, 8, 4, 1, 721, 1440)):
        assert wb(M, E, S, L, H, W) == R.workspace_bytes(E, S, L, H, W) and wb(M, E, S, L, H, W) % 8 == 0
    for bad in ((0, 1, 1, 1, 4, 4), (1025, 1, 1, 1, 4, 4), (4, 0, 1, 1, 4, 4), (4, 33, 1, 1, 4, 4), (4, 1, 0, 1, 4, 4), (4, 1, 17, 1, 4, 4),
                (4, 1, 1, 0, 4, 4), (4, 1, 1, 65536, 4, 4), (4, 1, 1, 1, 0, 4), (4, 1, 1, 1, 4097, 4096), (1024, 1, 1, 1, 2048, 2048)):
        assert wb(*bad) == 0, bad  # the last: M H W = 2^32 > 2^31, Sn would not fit uint32
    assert wb(1024, 1, 1, 1, 1024, 2048) > 0 and wb(512, 1, 1, 1, 2048, 2048) > 0  # M H W = 2^31 exactly
    assert hip.rollout_fss_workspace_bytes(50, 8, 4, 4, 120, 240) == R.workspace_bytes(8, 4, 4, 120, 240) and hip.rollout_fss_workspace_bytes(0, 1, 1, 1, 4, 4) == 0
