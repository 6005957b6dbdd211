"""Host side of the rollout-scoring driver (ladcast_amd.evaluate.evaluate_ens_gpu): the climatology / truth slot arithmetic against
pandas (what the reference's climatology_to_timeseries and `ds.sel(time=...)` index with) and the command line's file handling with an
injected scoring callable.  No GPU."""
import numpy as np
import pandas as pd
import pytest

from ladcast_amd.evaluate import evaluate_ens_gpu as EG

HOURS = (0, 6, 12, 18)


def _pandas_slots(start, lead, interval=6, exclude_start=True):
    """evaluate/utils.py:173-186 through the slot formula"""
    start = pd.to_datetime(start)
    idx = pd.date_range(start=start, end=start + pd.Timedelta(hours=lead), freq=f"{interval}h")
    if exclude_start:
        idx = idx[1:]
    return [(int(d) - 1) * len(HOURS) + HOURS.index(int(h)) for d, h in zip(idx.dayofyear, idx.hour)]


@pytest.mark.parametrize("start,lead,interval,exclude_start", [
    ("2020-02-27T18", 48, 6, True),  # crosses 29 February
    ("2019-12-30T12", 48, 6, True),  # the year wraps: day 365 -> day 1
    ("2020-12-30T00", 72, 6, True),  # reaches day 366
    ("2018-06-01T06", 60, 12, False),  # the start kept, 12 h apart
])
def test_climatology_slots_equal_pandas(start, lead, interval, exclude_start):
    got = EG.climatology_slots(start, lead, interval=interval, exclude_start=exclude_start)
    want = _pandas_slots(start, lead, interval, exclude_start)
    assert got == want and len(got) == lead // interval + (0 if exclude_start else 1)
    assert EG.climatology_slots(pd.to_datetime(start).to_pydatetime(), lead, interval, exclude_start) == want
    assert all(0 <= s < 366 * 4 for s in got)


def test_climatology_slot_landmarks():
    assert EG.climatology_slots("2020-02-28T18", 12)[:2] == [59 * 4 + 0, 59 * 4 + 1]  # 29 February = day 60
    assert EG.climatology_slots("2019-12-31T12", 12) == [364 * 4 + 3, 0]
    assert EG.climatology_slots("2020-12-30T18", 6) == [365 * 4]  # day 366
    assert EG.climatology_slots(2018010100, 12, exclude_start=False) == [0, 1, 2]


def test_hour_outside_the_climatology_raises():
    with pytest.raises(ValueError):
        EG.climatology_slots("2018-01-01T03", 12)
    with pytest.raises(ValueError):
        EG.climatology_slots("2018-01-01T00", 12, interval=3)
    with pytest.raises(ValueError):
        EG.climatology_slots("2018-01-01T00", 12, hours=(0, 12))


def test_truth_slot_arithmetic():
    """frames start at start_date, `step` apart: lead t of the forecast from `init` is frame (init - start) / step + 1 + t - the
    positions pandas gives the reference's ref_timerange inside the dataset's time axis"""
    axis = pd.date_range(start="2018-01-01", end="2018-01-20", freq="6h")
    for init in ("2018-01-01T00", "2018-01-03T18"):
        t0 = pd.to_datetime(init)
        ref = pd.date_range(start=t0 + pd.Timedelta(hours=6), end=t0 + pd.Timedelta(hours=48), freq="6h")
        want = [int(i) for i in axis.get_indexer(ref)]
        assert EG.truth_frame_slots(init, "2018-01-01", 6, 8) == want
    assert EG.truth_frame_slots(2018010100, "2018-01-01", 6, 3) == [1, 2, 3]
    assert EG.truth_frame_slots(2018010318, "2018-01-01", 6, 2) == [12, 13]
    with pytest.raises(ValueError):
        EG.truth_frame_slots("2018-01-01T03", "2018-01-01", 6, 2)


def test_main_refuses_lead_time_not_divisible_by_step(tmp_path):
    with pytest.raises(ValueError, match="divisible"):
        EG.main(["--result_path", str(tmp_path), "--output", str(tmp_path / "o"), "--total_lead_time_hour", "20", "--step_size_hour", "6"],
                score=lambda *a: None)


def test_main_writes_the_reference_files(tmp_path):
    """three latent files, the last later than end_date - lead: two are scored; names, shapes, dtypes, slots and the float32 timestamp"""
    res = tmp_path / "rollout"
    res.mkdir()
    for ts in (2018123000, 2018123118, 2019010100):
        np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    C, T = 3, 4
    calls = []

    def score(path, time_str, t_slots, c_slots):
        calls.append((path, time_str, t_slots, c_slots))
        base = np.full((C, T), float(len(calls)), dtype=np.float32)
        return {k: base + i for i, k in enumerate(("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps"))}

    out_dir = tmp_path / "scores"
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"], score=score)
    assert [c[1] for c in calls] == ["2018123000", "2018123118"]  # 2019010100 + 24 h is past the end date
    assert calls[0][0].endswith("latent_2018123000.npy")
    assert calls[0][2] == [5, 6, 7, 8] and calls[1][2] == [12, 13, 14, 15]  # (init - start) / 6 h + 1 + t
    assert calls[0][3] == _pandas_slots("2018-12-30T00", 24) and calls[1][3] == _pandas_slots("2018-12-31T18", 24)
    assert calls[1][3] == [0, 1, 2, 3]  # 2019-01-01 00 .. 18: the year wrapped
    names = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
    for n, ts in enumerate(("2018123000", "2018123118")):
        for i, k in enumerate(names):
            a = np.load(out_dir / f"{ts}_{k}.npy")
            assert a.shape == (C, T) and a.dtype == np.float32 and (a == n + 1 + i).all()
    for i, k in enumerate(names):
        a = np.load(out_dir / f"{k}.npy")
        assert a.shape == (2, C, T) and a.dtype == np.float32 and (a[1] == 2 + i).all() and np.array_equal(a, out[k])
    ts = np.load(out_dir / "timestamp.npy")
    assert ts.dtype == np.float32 and ts.shape == (2,)
    assert ts.tolist() == [float(np.float32(2018123000)), 2018123136.0]  # fp32 holds 24 bits: the reference's rounding, kept
    assert sorted(p.name for p in out_dir.iterdir()) == sorted([f"{t}_{k}.npy" for t in ("2018123000", "2018123118") for k in names]
                                                               + [f"{k}.npy" for k in names] + ["timestamp.npy"])


def test_main_refuses_a_result_of_the_wrong_shape(tmp_path):
    res = tmp_path / "rollout"
    res.mkdir()
    np.save(res / "latent_2018010100.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    bad = {k: np.zeros((3, 5), dtype=np.float32) for k in ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")}
    with pytest.raises(ValueError):
        EG.main(["--result_path", str(res), "--output", str(tmp_path / "o"), "--end_date", "2018-02-01", "--total_lead_time_hour", "24"],
                score=lambda *a: bad)


def test_lat_weights():
    import torch

    w = EG.lat_weights_for(120)
    lat = np.linspace(-88.5, 90, 120)
    want = np.cos(np.deg2rad(lat)) / np.cos(np.deg2rad(lat)).mean()
    assert w.dtype == torch.float32 and w.shape == (120,) and np.allclose(w.numpy(), want, rtol=1e-6, atol=1e-7)
    w48 = EG.lat_weights_for(48)
    lat48 = np.linspace(-90, 90, 49)[1:]
    assert w48.shape == (48,) and np.allclose(w48.numpy(), np.cos(np.deg2rad(lat48)) / np.cos(np.deg2rad(lat48)).mean(), rtol=1e-6, atol=1e-7)


# ---- the prologue the nine rollout wrappers share: one exception per mistake, before the device is asked for -----------------------------
_M, _C, _L, _H, _W = 2, 1, 1, 3, 8
_WRAPPERS = ("rollout_scores", "validation_scores", "rollout_reliability", "rollout_spectrum", "rollout_products", "rollout_events", "rollout_fss",
             "rollout_regional", "rollout_energy")
_CHECK_L_OFF = _WRAPPERS[4:]  # these refuse a negative l_off on the host; the four older ones pass it to the library


def _wrapper_call(name, *, forecast=None, weight=None, **kw):
    """`name` on host tensors of shape (2, 1, 1, 3, 8), valid but for what the caller replaces"""
    import torch

    from ladcast_amd import evaluate as E

    x = torch.zeros(_M, _C, _L, _H, _W) if forecast is None else forecast
    t, w = torch.zeros(_C, _L, _H, _W), torch.ones(_H) if weight is None else weight
    if name == "rollout_scores":
        return E.rollout_scores(x, t, t.clone(), w, -1, **kw)
    if name == "rollout_reliability":
        return E.rollout_reliability(x, t, w, -1, **kw)
    if name == "rollout_products":
        return E.rollout_products(x, **kw)
    if name == "rollout_events":
        return E.rollout_events(x, t, w, [E.Event(0, "gt", 0.5)], **kw)
    if name == "rollout_fss":
        return E.rollout_fss(x, t, w, [E.Event(0, "gt", 0.5)], [0, 1], **kw)
    if name == "rollout_regional":
        return E.rollout_regional(x, t, w, np.ones((_H, _W), dtype=np.uint32), 1, **kw)
    return getattr(E, name)(x, t, w, **kw)


@pytest.mark.parametrize("name", _WRAPPERS)
def test_rollout_wrappers_share_their_argument_errors(name):
    import torch

    cases = [
        (dict(forecast=torch.zeros(_M, _C, _H, _W)), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(lead_dim=1), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(forecast=torch.zeros(_M, _C, _L, _H, _W, dtype=torch.float64)), NotImplementedError, "fp32 only"),
        (dict(mean=torch.zeros(_C)), ValueError, "mean and std go together"),
        (dict(mean=torch.zeros(_C + 1), std=torch.ones(_C + 1)), ValueError, r"mean / std must hold one value per channel \(1\)"),
    ]
    if name != "rollout_products":  # no weight there
        what = "row_weight" if name == "rollout_spectrum" else "lat_weight"
        cases.append((dict(weight=torch.ones(_H + 1)), ValueError, f"{what} must have one value per latitude row"))
    if name in _CHECK_L_OFF:
        cases.append((dict(l_off=-1), ValueError, "l_off must not be negative"))
    for kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            _wrapper_call(name, **kw)
    with pytest.raises(RuntimeError, match="device tensors"):  # nothing wrong but the host tensors
        _wrapper_call(name)
    with pytest.raises(RuntimeError, match="device tensors"):
        _wrapper_call(name, mean=torch.zeros(_C), std=torch.ones(_C))
