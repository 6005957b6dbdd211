"""Host side of the threshold-event verification (csrc/events.hip, ladcast_amd.evaluate.rollout_events / event_scores, the --event flags
of evaluate_ens_gpu).  No GPU:
  a. the fp32 restatement of the kernel (tests/events_refs.py) meets the oracle at every case; every planted defect fails at least one
  b. event_scores: the decomposition, the direct Brier score, the ROC area against Mann-Whitney, the degenerate forecasts
  c. the command line's file handling with an injected scorer
  d. rollout_events raises the shared exceptions in the shared order
  e. the library's exports and the descriptor's layout"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import events_refs as R


# ---- a. the restatement against the oracle -----------------------------------------------------------------------------------------------
def _ref(c):
    return R.events_ref(c["x"], c["t"], c["w"], c["events"], c["cl"])


def _restated(c, defect=None):
    return R.kernel_f32(c["v"], c["t"], c["w"], c["events"], c["cl"], c["norm"], defect=defect)


def test_clean_restatement_meets_every_bound():
    worst = 0.0
    for name, c in R.cpu_cases():
        worst = max(worst, R.check(_restated(c), _ref(c), name))
    print(f"worst err / bound {worst:.4f}")


def test_oracle_equals_the_definitions_point_by_point():
    for c in (R.integer_case(2, 3, 50), R.nan_table_case(), R.physical_case(8)):
        ref, b = _ref(c), R.brute_force(c["x"], c["t"], c["w"], c["events"], c["cl"])
        assert torch.equal(ref["hist"], b["hist"]) and torch.equal(ref["n_invalid"], b["n_invalid"])
        assert torch.allclose(ref["hist_w"][0], b["hist_w"], rtol=1e-12, atol=0)
    c = R.nan_table_case()
    assert _ref(c)["n_invalid"].tolist() == R.nan_table_invalid(c["kind"])


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    cases = [("nan table", R.nan_table_case()), ("physical", R.physical_case(8)), ("integer", R.integer_case(9, 3, 50)),
             ("integer", R.integer_case(1, 1, 257))]
    caught = [name for name, c in cases if not R.passes(_restated(c, defect), _ref(c))]
    assert caught, f"defect {defect!r} passes every case: the tables have no teeth"
    print(defect, "caught by", caught)


def test_case_tables_cover_the_kernel_paths():
    assert {R.tiles_per_wg(M) for M in R.INT_M} >= {1, 2, 3, 4, 32}
    assert [R.n_records(H * W, M) for M, H, W in R.INT_EXTRA] == [2]  # several tiles per workgroup AND several records
    assert 2 * (127 + 1) == R.TPB and 2 * (128 + 1) > R.TPB and -(-2 * (1024 + 1) // R.TPB) == 9 and 2 * (1024 + 1) % R.TPB == 2
    assert all(R.n_records(H * W, R.R.FINISH_M) > 64 for H, W in R.FINISH_SHAPES)
    for M in (64, 128, 1024):  # the extreme bins are filled, the last bin slot among them
        h = _ref(R.integer_case(M, 3, 50))["hist"]
        assert int(h[0, M].sum()) > 0 and int(h[0, 0].sum()) > 0
    assert all(e != ev[0] for e, ev in enumerate(R.INT_EVENTS))  # no event e reads channel e


# ---- b. event_scores -----------------------------------------------------------------------------------------------------------------------
def _synthetic(M, N, seed, skill=0.6):
    g = np.random.default_rng(seed)
    p_true = g.uniform(0, 1, N)
    o = (g.uniform(0, 1, N) < p_true).astype(np.int64)
    n = g.binomial(M, skill * p_true + (1 - skill) * 0.5)
    w = g.uniform(0.2, 1.5, N)
    h = np.zeros((M + 1, 2))
    np.add.at(h, (n, o), w)
    return n, o, w, h


@pytest.mark.parametrize("M,N", [(1, 300), (5, 400), (50, 600)])
def test_event_scores_decomposition_brier_and_roc(M, N):
    from ladcast_amd.evaluate import event_scores

    n, o, w, h = _synthetic(M, N, 7 * M + N)
    s = event_scores(h)
    assert abs(s["brier"] - (s["reliability"] - s["resolution"] + s["uncertainty"])) <= 1e-12 * max(s["brier"], s["uncertainty"])
    direct = (w * (n / M - o) ** 2).sum() / w.sum()
    assert abs(s["brier"] - direct) <= 1e-12 * direct
    assert abs(s["base_rate"] - (w * o).sum() / w.sum()) <= 1e-12 and abs(s["forecast_mean"] - (w * n / M).sum() / w.sum()) <= 1e-12
    assert abs(s["bss"] - (1 - direct / s["uncertainty"])) <= 1e-10
    # Mann-Whitney over all (event point, non-event point) pairs, ties counted half, weights multiplied
    ev, ne = o == 1, o == 0
    d = n[ev][:, None] - n[ne][None, :]
    ww = w[ev][:, None] * w[ne][None, :]
    mw = (ww * ((d > 0) + 0.5 * (d == 0))).sum() / ww.sum()
    assert abs(s["roc_area"] - mw) <= 1e-12
    assert s["roc_pod"].shape == s["roc_pofd"].shape == (M + 2,) and s["roc_pod"][0] == s["roc_pofd"][0] == 0 and s["roc_pod"][-1] == s["roc_pofd"][-1] == 1
    assert s["rel_obs"].shape == (M + 1,) and abs(np.nansum(s["rel_weight"]) - 1) <= 1e-12
    filled = h.sum(-1) > 0
    assert np.array_equal(np.isnan(s["rel_obs"]), ~filled)  # an empty bin is NaN on the curve
    both = event_scores(np.stack([h, 3 * h]))  # leading dimensions; the scores do not depend on the scale of the weights
    for k in ("brier", "reliability", "resolution", "uncertainty", "bss", "roc_area"):
        assert both[k].shape == (2,) and abs(both[k][0] - s[k]) <= 1e-15 and abs(both[k][1] - s[k]) <= 1e-12


def test_event_scores_degenerate_forecasts():
    from ladcast_amd.evaluate import event_scores

    M = 4
    perfect = np.zeros((M + 1, 2))
    perfect[0, 0], perfect[M, 1] = 7.0, 3.0
    s = event_scores(perfect)
    assert s["roc_area"] == 1.0 and s["brier"] == 0.0 and s["reliability"] == 0.0 and abs(s["bss"] - 1.0) <= 1e-15
    const = np.zeros((M + 1, 2))
    const[2] = (6.0, 2.0)
    s = event_scores(const)
    assert s["roc_area"] == 0.5 and s["resolution"] == 0.0 and abs(s["brier"] - (0.75 * 0.25 + 0.25 * 0.25)) <= 1e-15
    one_class = np.zeros((M + 1, 2))
    one_class[:, 0] = (1.0, 2.0, 0.0, 1.0, 0.5)
    s = event_scores(one_class)
    assert np.isnan(s["roc_area"]) and np.isnan(s["bss"]) and s["uncertainty"] == 0.0 and np.isfinite(s["brier"])
    s = event_scores(np.zeros((2, M + 1, 2)))
    assert all(np.isnan(s[k]).all() for k in ("brier", "reliability", "resolution", "uncertainty", "bss", "base_rate", "forecast_mean", "roc_area"))
    counts = event_scores(np.array([[3, 0], [1, 1], [0, 2]], dtype=np.int64))  # counts are weights
    assert abs(counts["brier"] - (0.25 + 0.25) / 7) <= 1e-15
    with pytest.raises(ValueError):
        event_scores(np.zeros((5, 3)))


# ---- c. the command line -------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
EVENT_FILES = ("event_hist", "event_hist_weighted", "event_n_invalid", "event_brier", "event_bss", "event_reliability", "event_resolution",
               "event_uncertainty", "event_roc_area")


def _run_main(tmp_path, name, extra, M=3):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    if not res.exists():
        res.mkdir()
        for ts in (2018123000, 2018123106):
            np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    C, T, E = 3, 4, 3
    g = np.random.default_rng(5)
    per_init = []

    def score(path, time_str, t_slots, c_slots):
        out = {k: np.full((C, T), 1.0 + i, dtype=np.float32) for i, k in enumerate(SCORES)}
        if extra:
            h = g.integers(0, 50, (E, T, M + 1, 2)).astype(np.int32)
            hw = (h * g.uniform(0.5, 1.5, h.shape)).astype(np.float32)
            per_init.append((h, hw))
            out.update(event_hist=torch.from_numpy(h), event_hist_weighted=torch.from_numpy(hw),
                       event_n_invalid=torch.full((E, T), len(per_init), dtype=torch.int32))
        return out

    out_dir = tmp_path / name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + extra, score=score)
    return out_dir, out, per_init


def test_main_event_flags_write_the_event_files(tmp_path):
    from ladcast_amd.evaluate import event_scores

    plain, _, _ = _run_main(tmp_path, "plain", [])
    flags = ["--event", "2m_temperature", "gt", "303.15", "--event_anomaly", "geopotential_level500", "lt", "-50", "--event", "7", "lt", "250"]
    with_ev, out, per_init = _run_main(tmp_path, "events", flags)
    before = sorted(p.name for p in plain.iterdir())
    assert before == sorted([f"{t}_{k}.npy" for t in ("2018123000", "2018123106") for k in SCORES] + [f"{k}.npy" for k in SCORES] + ["timestamp.npy"])
    assert sorted(p.name for p in with_ev.iterdir()) == sorted(before + [f"{k}.npy" for k in EVENT_FILES] + ["events.json"])
    for p in plain.iterdir():
        assert (with_ev / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(with_ev / f"{k}.npy") for k in EVENT_FILES}
    E, T, M = 3, 4, 3
    assert a["event_hist"].shape == a["event_hist_weighted"].shape == (E, T, M + 1, 2)
    assert a["event_hist"].dtype == np.int64 and a["event_hist_weighted"].dtype == np.float64
    assert a["event_n_invalid"].shape == (2, E, T) and a["event_n_invalid"].dtype == np.int32 and a["event_n_invalid"][1].tolist() == np.full((E, T), 2).tolist()
    assert len(per_init) == 2  # pooling over the two initial times is the sum
    assert np.array_equal(a["event_hist"], per_init[0][0].astype(np.int64) + per_init[1][0])
    assert np.array_equal(a["event_hist_weighted"], per_init[0][1].astype(np.float64) + per_init[1][1].astype(np.float64))
    sc = event_scores(a["event_hist_weighted"])
    for k in ("brier", "bss", "reliability", "resolution", "uncertainty", "roc_area"):
        f = a[f"event_{k}"]
        assert f.shape == (E, T) and f.dtype == np.float64 and np.array_equal(f, sc[k]) and np.array_equal(f, out[f"event_{k}"])
    meta = json.loads((with_ev / "events.json").read_text())["events"]
    from ladcast_amd.evaluate.products import column_names
    from ladcast_amd.evaluate.track import VARIABLE_NAMES

    names = column_names(VARIABLE_NAMES)
    assert [(m["channel"], m["direction"], m["threshold"], m["anomaly"]) for m in meta] == [
        ("2m_temperature", "gt", 303.15, False), (names[7], "lt", 250.0, False), ("geopotential_level500", "lt", -50.0, True)]
    assert [m["channel_index"] for m in meta] == [names.index("2m_temperature"), 7, names.index("geopotential_level500")]


def test_main_event_flags_refuse_bad_entries(tmp_path):
    for bad in (["--event", "no_such_channel", "gt", "1"], ["--event", "0", "ge", "1"], ["--event_anomaly", "0", "gt", "nan"]):
        with pytest.raises(ValueError):
            _run_main(tmp_path, "bad", bad)
    with pytest.raises(ValueError, match="--event needs"):  # a scorer that does not return the event arrays
        from ladcast_amd.evaluate import evaluate_ens_gpu as EG

        EG.main(["--result_path", str(tmp_path / "rollout"), "--output", str(tmp_path / "o"), "--start_date", "2018-12-29", "--end_date",
                 "2019-01-01T18", "--total_lead_time_hour", "24", "--event", "0", "gt", "1"],
                score=lambda *a: {k: np.zeros((3, 4), dtype=np.float32) for k in SCORES})


# ---- d. the wrapper's argument errors ------------------------------------------------------------------------------------------------------
_M, _C, _L, _H, _W = 2, 1, 1, 3, 8


def _call(*, forecast=None, weight=None, events=((0, "gt", 0.5),), **kw):
    from ladcast_amd import evaluate as E

    x = torch.zeros(_M, _C, _L, _H, _W) if forecast is None else forecast
    t, w = torch.zeros(_C, _L, _H, _W), torch.ones(_H) if weight is None else weight
    return E.rollout_events(x, t, w, events, **kw)


def test_rollout_events_shares_the_argument_errors():
    from ladcast_amd.evaluate import Event

    cl = torch.zeros(_C, _L, _H, _W)
    cases = [
        (dict(forecast=torch.zeros(_M, _C, _H, _W)), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(lead_dim=1), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(forecast=torch.zeros(_M, _C, _L, _H, _W, dtype=torch.float64)), NotImplementedError, "fp32 only"),
        (dict(mean=torch.zeros(_C)), ValueError, "mean and std go together"),
        (dict(mean=torch.zeros(_C + 1), std=torch.ones(_C + 1)), ValueError, r"mean / std must hold one value per channel \(1\)"),
        (dict(weight=torch.ones(_H + 1)), ValueError, "lat_weight must have one value per latitude row"),
        (dict(events=[(0, "gt", float("nan"))]), ValueError, "NaN"),
        (dict(events=[(0, "ge", 0.5)]), ValueError, "direction"),
        (dict(events=[Event(0, "gt", 0.5, True)]), ValueError, "climatology"),
        (dict(events=[(1, "gt", 0.5)]), ValueError, "channel"),
        (dict(events=[]), ValueError, "events"),
        (dict(events=[(0, "lt", 0.0)] * 33), ValueError, "events"),
        (dict(events=[(0, "gt", 0.5, True)], clim=torch.zeros(_C, _L, _H + 1, _W)), ValueError, "clim must be"),
    ]
    for kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            _call(**kw)
    with pytest.raises(RuntimeError, match="device tensors"):  # nothing wrong but the host tensors
        _call()
    with pytest.raises(RuntimeError, match="device tensors"):
        _call(events=[Event(0, "lt", 0.5, True)], clim=cl, mean=torch.zeros(_C), std=torch.ones(_C))


def test_score_latent_rollout_refuses_an_anomaly_event_without_climatology():
    from ladcast_amd.evaluate import Event, evaluate_ens_gpu as EG

    with pytest.raises(ValueError, match="climatology"):
        EG.score_latent_rollout(torch.zeros(2, 1, 1, 2, 2), None, None, None, torch.zeros(3, 1, 4, 4), [0], None, None, torch.ones(4),
                                events=[Event(0, "gt", 1.0, True)])


# ---- e. the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_and_descriptor_layout():
    from ladcast_amd import hip

    for name in ("ldc_rollout_events", "ldc_rollout_events_workspace_bytes", "ldc_sizeof_events_desc"):
        assert hasattr(hip.lib, name) and name in hip.SIGNATURES
    assert hip.lib.ldc_sizeof_events_desc() == ctypes.sizeof(hip.EventsDesc) == 4 + 4 * 4 * hip.EVENTS_MAX and hip.EVENTS_MAX == R.MAX_E
    assert hip.lib.ldc_abi_version() == 5
    wb = hip.lib.ldc_rollout_events_workspace_bytes
    for M, E, L, H, W in ((5, 3, 2, 3, 50), (64, 1, 1, 16, 16), (65, 2, 1, 1, 257), (1024, 32, 4, 120, 240)):
        assert wb(M, E, L, H, W) == R.workspace_bytes(M, E, L, H * W)
    for bad in ((0, 1, 1, 4, 4), (1025, 1, 1, 4, 4), (4, 0, 1, 4, 4), (4, 33, 1, 4, 4), (4, 1, 0, 4, 4), (4, 1, 65536, 4, 4), (4, 1, 1, 0, 4),
                (4, 1, 1, 4097, 4096)):
        assert wb(*bad) == 0, bad
    # the workspace stays level with M: about half a word per point and (event, lead time)
    per_point = [wb(M, 1, 1, 120, 240) / (4 * 120 * 240) for M in (32, 50, 64, 128, 1024)]
    assert max(per_point) < 0.6, per_point  # (4 M + 8) / (256 ceil(M / 32)) <= 0.5 + 1 / M words, plus the last record's unused tiles
    d = hip.events_desc([(2, 1, 303.15, 0), (0, -1, -1.5, 1)])
    assert d.n_events == 2 and list(d.channel[:2]) == [2, 0] and list(d.dir[:2]) == [1, -1] and list(d.anomaly[:2]) == [0, 1]
    assert d.thr[0] == np.float32(303.15) and d.thr[1] == -1.5
    for bad in ([], [(0, 2, 1.0, 0)], [(0, 1, float("nan"), 0)], [(0, 1, 1.0, 2)], [(0, 1, 1.0, 0)] * 33):
        with pytest.raises(ValueError):
            hip.events_desc(bad)
