"""CPU checks of the dataset-preparation leg (ladcast_amd.preprocess): the new C ABI entries, the exact-arithmetic oracle against rational
arithmetic, the condition on the GPU tests' inputs (numpy's float64 statistics meet the accuracy rule on every one of them, so a GPU
failure is the kernel's), the two JSON layouts through their readers, and what the command lines refuse before touching the device."""
import json
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import preprocess_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_moments_entries():
    from ladcast_amd import hip

    with open(os.path.join(ROOT, "include", "ladcast_hip.h")) as f:
        header = f.read()
    for name in ("ldc_field_moments_workspace_bytes", "ldc_field_moments"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in hip.SIGNATURES and hasattr(hip.lib, name)
    assert re.search(r"#define\s+LDC_ABI_VERSION\s+5\b", header) and hip.ABI_VERSION == 5 and hip.lib.ldc_abi_version() == 5
    wb = hip.lib.ldc_field_moments_workspace_bytes
    # one 32-byte record per chunk of <= 4096 values: whole rows, or pieces of a row
    assert wb(1, 1, 1, 1) == 32 and wb(2, 4, 15, 30) == 2 * 4 * 32
    assert wb(32, 84, 120, 240) == 32 * 84 * 8 * 32  # 17 rows per chunk: 8 chunks
    assert wb(2, 2, 150, 64) == 2 * 2 * 3 * 32 and wb(1, 2, 2, 8200) == 2 * 2 * 3 * 32
    assert wb(0, 1, 1, 1) == 0 and wb(1, 1, -1, 1) == 0
    assert wb(1 << 12, 1 << 12, 1, 1) == 0  # 2^24 records: above what one launch holds


def test_oracle_agrees_with_rational_arithmetic():
    rng = np.random.default_rng(7)
    inputs = [np.float32([1.5]), np.float32([0.1, 0.2, 0.3]), rng.standard_normal(37).astype(np.float32) * 3 + 100,
              (rng.standard_normal(50) * 3 + 2.0e5).astype(np.float32), np.float32([np.nan, 4.0, np.nan, 7.0, 1e-3]),
              np.full(9, np.float32(0.3))]
    for v in inputs:
        n, mean, var = PO.fraction_moments(v)
        got = PO.exact_channel(v)
        assert got["n"] == n
        std = math.sqrt(var) if var else 0.0  # Fraction -> float rounds correctly; sqrt adds one rounding
        assert abs(Fraction(got["mean_hi"]) + Fraction(got["mean_lo"]) - mean) <= Fraction(2) ** -60 * max(abs(mean), 1)
        assert abs(got["std"] - std) <= 2.0 ** -50 * std and (var != 0 or got["std"] == 0.0)
        assert max(PO.rule_ratios(float(mean), std, got)) <= 0.25  # the correctly rounded doubles: half an ulp of |mean| = 2e5 is 0.07 of the bound at std 2.5
    assert PO.fraction_moments(np.float32([np.nan]))[0] == 0 and PO.exact_channel(np.float32([np.nan]))["n"] == 0
    assert PO.rule_ratios(float("nan"), float("nan"), PO.exact_channel(np.float32([np.nan]))) == (0.0, 0.0)


@pytest.mark.parametrize("name", list(PO.CASES))
def test_numpy_float64_meets_the_rule_on_every_gpu_input(name):
    x, view, want = PO.case(name)
    mean, std = PO.numpy_stats(x[view])
    r = PO.worst_ratio(mean, std, want)
    print(f"\n{name} {x[view].shape}: numpy float64 nanmean / nanstd at {r:.3g} of the rule's bound")
    assert r <= 1.0, r
    if name == "stream":  # the frames of every streamed batch meet it too
        i = 0
        for b in PO.STREAM_SPLIT:
            part = x[i : i + b]
            assert PO.worst_ratio(*PO.numpy_stats(part), PO.exact_moments(part)) <= 1.0
            i += b


def test_unpivoted_sum_of_squares_violates_the_rule_on_the_teeth_case():
    """the case has teeth: float64 sum x^2 / n - mean^2 misses the bound ~2000 times over in the channel with mean 2e5 and std 3 (the
    cancellation costs (mean / std)^2 = 2^32 of float64's 2^53).  The channel with mean 1e5 and std 3e3 loses only 2^10 that way and
    stays inside in float64 (0.002 of the bound); it is the mid-range companion, so only the case as a whole is asserted to fail."""
    x, view, want = PO.case("teeth")
    mean, std = PO.unpivoted_stats(x[view])
    ratios = [max(PO.rule_ratios(float(m), float(s), w)) for m, s, w in zip(mean, std, want)]
    print(f"\nunpivoted float64 sum of squares on the teeth case: {ratios[0]:.3g} and {ratios[1]:.3g} of the bound")
    assert ratios[0] > 100.0 and max(ratios) > 1.0, ratios
    assert abs(want[0]["mean_hi"] - 2.0e5) < 1 and abs(want[0]["std"] - 3) < 0.2 and abs(want[1]["std"] - 3.0e3) < 200


def test_normalization_dict_round_trips_through_the_reader():
    from ladcast_amd.evaluate.track import LEVELS, VARIABLE_NAMES, mean_std_from_json
    from ladcast_amd.preprocess import normalization_dict

    rng = np.random.default_rng(3)
    mean, std = rng.standard_normal(84) * 100, rng.random(84) + 0.5
    d = normalization_dict(mean, std, VARIABLE_NAMES, LEVELS)
    assert list(d) == list(VARIABLE_NAMES) and list(d["geopotential"]["mean"]) == list(LEVELS) and isinstance(d["2m_temperature"]["mean"], float)
    back = json.loads(json.dumps(d))
    assert list(back["temperature"]["std"]) == [str(p) for p in LEVELS]
    m, s = mean_std_from_json(back)
    assert np.array_equal(m.numpy(), mean.astype(np.float32)) and np.array_equal(s.numpy(), std.astype(np.float32))
    # levels in a non-sorted order stay in that order; a subset of the variables reads its own channels
    d2 = normalization_dict(np.arange(8.0), np.arange(8.0) + 10, ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"], [850, 300, 500])
    assert list(d2["temperature"]["mean"].items()) == [(850, 3.0), (300, 4.0), (500, 5.0)] and d2["sea_surface_temperature"] == {"mean": 7.0, "std": 17.0}
    m2, s2 = mean_std_from_json(json.loads(json.dumps(d2)), ["temperature", "sea_surface_temperature"])
    assert m2.tolist() == [3.0, 4.0, 5.0, 7.0] and s2.tolist() == [13.0, 14.0, 15.0, 17.0]
    for bad in (dict(mean=np.zeros(7), std=np.zeros(7)), dict(mean=np.zeros(8), std=np.zeros(7))):
        with pytest.raises(ValueError):
            normalization_dict(bad["mean"], bad["std"], ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"], [850, 300, 500])
    assert normalization_dict([1.0, 2.0], [3.0, 4.0], ["a", "b"], []) == {"a": {"mean": 1.0, "std": 3.0}, "b": {"mean": 2.0, "std": 4.0}}


def test_latent_normal_dict_round_trips_through_the_reader(tmp_path):
    from ladcast_amd.evaluate.pred_rollout import load_latent_transform_args
    from ladcast_amd.preprocess import latent_normal_dict

    mean, std = np.linspace(-1, 1, 84), np.linspace(0.5, 2, 84)
    d = latent_normal_dict(mean, std)
    assert list(d) == ["mean", "std"]
    p = tmp_path / "latent_normal.json"
    p.write_text(json.dumps(d))
    args = load_latent_transform_args(str(p))
    assert args["mean"] == mean.tolist() and args["std"] == std.tolist() and args["target_std"] == 0.5
    with pytest.raises(ValueError):
        latent_normal_dict([1.0], [1.0, 2.0])


def test_command_lines_refuse_bad_inputs_before_the_device(tmp_path):
    from ladcast_amd.preprocess import compute_mean_std_era5 as CM
    from ladcast_amd.preprocess import encode_data as ED

    names = {"channel_names": ["geopotential", "2m_temperature"], "pressure_levels": [500, 850], "num_atm_vars": 1}  # 3 channels
    (tmp_path / "names.json").write_text(json.dumps(names))
    np.save(tmp_path / "ok.npy", np.zeros((2, 3, 4, 8), dtype=np.float32))
    np.save(tmp_path / "four.npy", np.zeros((2, 4, 4, 8), dtype=np.float32))
    np.save(tmp_path / "f64.npy", np.zeros((2, 3, 4, 8), dtype=np.float64))
    np.save(tmp_path / "f64_four.npy", np.zeros((2, 4, 4, 8), dtype=np.float64))
    nj, out = str(tmp_path / "names.json"), str(tmp_path / "out.json")
    stats = lambda frames, *more: CM.main(["--frames", str(tmp_path / frames), "--variable_names_json", nj, "--output", out, *more])  # noqa: E731
    enc = lambda frames, *more: ED.main(["--frames", str(tmp_path / frames), "--variable_names_json", nj, "--normalization_json", out,  # noqa: E731
                                         "--encdec_model", str(tmp_path), "--output", str(tmp_path / "lat.npy"), "--latent_normal_json",
                                         str(tmp_path / "ln.json"), *more])
    for call, args in ((stats, ("four.npy",)), (stats, ("f64.npy",)), (stats, ("ok.npy", "--batch_size", "0")),
                       (enc, ("ok.npy",)),  # the encoder's frames carry one more channel (the dropped surface pressure): 3 is one short
                       (enc, ("f64_four.npy",)), (enc, ("four.npy", "--batch_size", "0"))):
        with pytest.raises(SystemExit) as e:
            call(*args)
        assert e.value.code not in (0, None), args
    with pytest.raises(SystemExit):  # the default names are the 84 channels
        CM.main(["--frames", str(tmp_path / "ok.npy"), "--output", out])
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "lat.npy")
    # batches span files and end ragged
    a, b = np.arange(3, dtype=np.float32).reshape(3, 1, 1, 1), np.arange(3, 5, dtype=np.float32).reshape(2, 1, 1, 1)
    assert [t.reshape(-1).tolist() for t in CM.frame_batches([a, b], 2)] == [[0.0, 1.0], [2.0, 3.0], [4.0]]
