"""CPU side of the ensemble-products feature (csrc/products.hip: ldc_rollout_products; tests/products_refs.py):
  - the fp32 restatement of the kernel's arithmetic is within the counted bounds of the float64 oracle on every case of the GPU tests
  - every planted defect is caught by `check`
  - the host-side ValueErrors of `rollout_products`, the descriptor the host builds
  - the new symbols in header, binding and library
  - the command line's parsing, naming and file layout, with the device call stubbed"""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import products_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both_leads(x, quantiles, thr, dirs, what, channels=None):
    worst = 0.0
    for l in range(x.shape[2]):
        xs = x[:, :, l] if channels is None else x[:, list(channels), l]
        worst = max(worst, R.check(R.kernel_f32(xs, quantiles, thr, dirs), R.products_ref(xs, quantiles, thr, dirs), f"{what} lead {l}"))
    return worst


# ---- the bounds admit the kernel's arithmetic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.REGISTER_M)
def test_kernel_f32_within_bounds_integers(M):
    for H, W in R.SHAPES:
        c = R.integer_case(M, H, W)
        r = both_leads(c["x"], R.QUANTILES, c["thr"], c["dirs"], f"M={M} {H}x{W}")
        print(f"integers M={M} {H}x{W}: worst err / bound {r:.4f}")
        got = R.kernel_f32(c["x"][:, :, 0], R.QUANTILES, c["thr"], c["dirs"])
        ref = R.products_ref(c["x"][:, :, 0], R.QUANTILES, c["thr"], c["dirs"])
        assert R.same_value_bits(got["mean"], ref["mean"][0].float()), "every sum is exact: the mean is the float64 value rounded once"
        assert bool(torch.isnan(got["std"]).all()) == (M == 1)


@pytest.mark.parametrize("M", R.STREAM_M)
def test_kernel_f32_within_bounds_streaming(M):
    H, W = R.SHAPES[0]
    c = R.integer_case(M, H, W)
    r = both_leads(c["x"], (), c["thr"], c["dirs"], f"M={M}")
    print(f"streaming M={M}: worst err / bound {r:.4f}")


@pytest.mark.parametrize("with_inf", [False, True])
@pytest.mark.parametrize("M", [4, 9, 64])
def test_kernel_f32_within_bounds_ties(M, with_inf):
    H, W = R.SHAPES[1]
    c = R.ties_case(M, H, W, with_inf)
    both_leads(c["x"], R.QUANTILES, c["thr"], c["dirs"], f"ties M={M} inf={with_inf}")


@pytest.mark.parametrize("target_std", [1.0, 0.5])
@pytest.mark.parametrize("M", R.PHYS_M)
def test_kernel_f32_within_bounds_physical(M, target_std):
    H, W = R.SHAPES[1]
    c = R.physical_case(M, H, W)
    x = R.inv_norm_f32(c["v"], c["mean"], c["std"], target_std)
    for channels in (None, (2, 0)):
        thr, dirs = R.phys_thresholds(channels or (0, 1, 2))
        r = both_leads(x, R.QUANTILES, thr, dirs, f"physical M={M} target_std={target_std} channels={channels}", channels)
        print(f"physical M={M} target_std={target_std} channels={channels}: worst err / bound {r:.4f}")


def test_kernel_f32_nan_table():
    H, W = R.SHAPES[0]
    c = R.nan_case(H, W)
    both_leads(c["x"], R.QUANTILES, c["thr"], c["dirs"], "NaN table")
    got = R.kernel_f32(c["x"][:, :, 0], R.QUANTILES, c["thr"], c["dirs"])
    h, w = c["point"]
    for k in R.STAT_NAMES:
        nan = torch.isnan(got[k])
        assert int(nan.sum()) == R.C and bool(nan[:, h, w].all()), k
    assert int(torch.isnan(got["quantiles"]).sum()) == len(R.QUANTILES) * R.C
    p, ch = c["nan_thr"]
    nan = torch.isnan(got["exceed"])
    assert bool(nan[p, ch].all()) and int(nan.sum()) == H * W + (len(c["dirs"]) * R.C - 1)


# ---- planted defects ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defects_are_caught(defect):
    H, W = R.SHAPES[0]
    cases = [R.integer_case(5, H, W), R.integer_case(64, H, W), R.nan_case(H, W)]
    caught = 0
    for c in cases:
        xs = c["x"][:, :, 0]
        ref = R.products_ref(xs, R.QUANTILES, c["thr"], c["dirs"])
        R.check(R.kernel_f32(xs, R.QUANTILES, c["thr"], c["dirs"]), ref, "clean")
        try:
            R.check(R.kernel_f32(xs, R.QUANTILES, c["thr"], c["dirs"], defect=defect), ref, defect)
        except AssertionError:
            caught += 1
    assert caught >= (1 if defect == "nan_ignored" else 3), f"{defect}: caught on {caught} of {len(cases)} cases"


# ---- the host side ------------------------------------------------------------------------------------------------------------------------
def test_descriptor_matches_the_oracle_positions():
    import ctypes

    from ladcast_amd import hip

    assert hip.lib.ldc_sizeof_products_desc() == ctypes.sizeof(hip.ProductsDesc) == 4 * (2 + 16 + 16 + 8)
    for M in R.REGISTER_M:
        d = hip.products_desc(R.QUANTILES, M, (1, -1))
        assert (d.n_quant, d.n_thr, d.thr_dir[0], d.thr_dir[1]) == (len(R.QUANTILES), 2, 1, -1)
        assert [(d.q_lo[k], d.q_t[k]) for k in range(d.n_quant)] == [R.quantile_pos(q, M) for q in R.QUANTILES]
        assert (d.q_lo[0], d.q_t[0]) == (0, 0.0) and (d.q_lo[d.n_quant - 1], d.q_t[d.n_quant - 1]) == (M - 1, 0.0)
    d = hip.products_desc([0.5], 5)
    assert (d.q_lo[0], d.q_t[0]) == (2, 0.0)  # the median of an odd ensemble is a member


def test_rollout_products_value_errors():
    from ladcast_amd.evaluate.utils import ProductsDict, empty_products, rollout_products

    x = torch.zeros(5, 3, 2, 4, 6)  # host tensor: every ValueError comes before the device is asked for
    for bad in ([-0.1], [1.5], [float("nan")], [0.5] * 17):
        with pytest.raises(ValueError):
            rollout_products(x, quantiles=bad)
    thr = torch.zeros(2, 3)
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=torch.zeros(9, 3))  # more than 8 thresholds
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=thr, threshold_dirs=[1, 0])
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=thr, threshold_dirs=[1, 2])
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=thr, threshold_dirs=[1])
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=torch.zeros(2, 2))  # not (P, Cs)
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=torch.zeros(3), channels=[0, 1, 2])
    with pytest.raises(ValueError):
        rollout_products(x, thresholds=thr, channels=[2, 0])  # Cs is 2 now
    for bad in ([3], [-1], [0, 7]):
        with pytest.raises(ValueError):
            rollout_products(x, channels=bad)
    with pytest.raises(ValueError):
        rollout_products(torch.zeros(65, 1, 1, 2, 2), quantiles=[0.5])  # sorted arm: 64 members
    with pytest.raises(ValueError):
        rollout_products(torch.zeros(1025, 1, 1, 2, 2))
    with pytest.raises(ValueError):
        rollout_products(x, stats=False)  # nothing to compute
    with pytest.raises(ValueError):
        rollout_products(x[0])
    for out in (empty_products(3, 2, 4, 7, "cpu"), empty_products(2, 2, 4, 6, "cpu"), empty_products(3, 1, 4, 6, "cpu"), dict(mean=x[0])):
        with pytest.raises(ValueError):
            rollout_products(x, out=out)
    with pytest.raises(ValueError):
        rollout_products(x, quantiles=[0.5], out=empty_products(3, 2, 4, 6, "cpu"))  # no room for a quantile plane
    with pytest.raises(ValueError):
        rollout_products(x, out=empty_products(3, 3, 4, 6, "cpu"), l_off=2)  # columns 2 .. 3 of 3
    e = empty_products(3, 4, 4, 6, "cpu", n_quantiles=2, n_thresholds=1)
    assert isinstance(e, ProductsDict) and sorted(e) == ["exceed", "max", "mean", "min", "quantiles", "std"]
    assert e["mean"].shape == (3, 4, 4, 6) and e["quantiles"].shape == (2, 3, 4, 4, 6) and e["exceed"].shape == (1, 3, 4, 4, 6)
    assert all(bool(torch.isnan(v).all()) for v in e.values())
    assert sorted(empty_products(3, 4, 4, 6, "cpu", n_quantiles=1, stats=False)) == ["quantiles"]
    with pytest.raises(RuntimeError):  # valid arguments, host tensors: no CPU fallback
        rollout_products(x, quantiles=[0.5])


def test_new_symbols_in_header_binding_and_library():
    from ladcast_amd import hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    for name in ("ldc_rollout_products", "ldc_sizeof_products_desc"):
        assert re.search(rf"\b{name}\s*\(", header) and name in hip.SIGNATURES and hasattr(hip.lib, name)
    assert "LDC_PRODUCTS_MAX_QUANTILES 16" in header and "LDC_PRODUCTS_MAX_THRESHOLDS 8" in header
    assert (hip.PRODUCTS_MAX_QUANTILES, hip.PRODUCTS_MAX_THRESHOLDS) == (R.MAX_Q, R.MAX_P) == (16, 8)
    assert len(hip.SIGNATURES["ldc_rollout_products"][1]) == 22
    mk = open(os.path.join(ROOT, "ladcast_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bproducts\.hip\b", mk, re.M) and "EXTRA_products = -ffp-contract=off" in mk


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_command_line_parsing_naming_and_files(tmp_path):
    from ladcast_amd.evaluate import products as P
    from ladcast_amd.evaluate.track import VARIABLE_NAMES
    from ladcast_amd.evaluate.validate_AR import column_names
    from ladcast_amd.pipelines.io import save_latent_npy

    names = column_names(VARIABLE_NAMES)
    assert len(names) == 84 and names[7] == "geopotential_level500" and names[80] == "2m_temperature" and names[81] == "mean_sea_level_pressure"
    assert P.resolve_channels(["2m_temperature", "geopotential_level500", "81"], names) == [80, 7, 81]
    for bad in ("2m_temp", "84", "-1"):
        with pytest.raises(ValueError):
            P.resolve_channels([bad], names)
    thr, dirs, meta = P.threshold_table([("2m_temperature", "gt", "303.15"), ("81", "lt", "98000")], [80, 7, 81], names)
    assert dirs == [1, -1] and thr.shape == (2, 3) and thr.dtype == torch.float32
    assert thr[0, 0] == np.float32(303.15) and thr[1, 2] == 98000.0 and int(torch.isnan(thr).sum()) == 4
    assert meta[1] == dict(channel="mean_sea_level_pressure", channel_index=81, direction="lt", threshold=98000.0)
    with pytest.raises(ValueError):
        P.threshold_table([("sea_surface_temperature", "gt", "300")], [80, 7, 81], names)  # not among the channels
    with pytest.raises(ValueError):
        P.threshold_table([("2m_temperature", "ge", "300")], [80], names)
    assert P.threshold_table([], [80], names) == (None, [], [])

    ENS, T, H, W = 4, 2, 3, 5
    save_latent_npy(torch.zeros(2, ENS, 2, 1 + T, 2, 2), [2020010100, 2020010112], str(tmp_path / "rollout"))
    seen = []

    def stub(path, time_str):
        seen.append((os.path.basename(path), time_str))
        k = float(len(seen))
        out = {n: torch.full((3, T, H, W), k) for n in P.PRODUCT_STAT_NAMES}
        out.update(quantiles=torch.full((3, 3, T, H, W), k), exceed=torch.full((2, 3, T, H, W), k))
        return out

    argv = ["--result_path", str(tmp_path / "rollout"), "--output", str(tmp_path / "products"), "--channels", "2m_temperature", "geopotential_level500", "81",
            "--quantiles", "0.1", "0.5", "0.9", "--exceed", "2m_temperature", "gt", "303.15", "--exceed", "mean_sea_level_pressure", "lt", "98000"]
    meta = P.main(argv, products=stub)
    assert seen == [("latent_2020010100.npy", "2020010100"), ("latent_2020010112.npy", "2020010112")]
    assert sorted(p.name for p in (tmp_path / "products").iterdir()) == ["products.json", "products_2020010100.npz", "products_2020010112.npz"]
    z = np.load(tmp_path / "products" / "products_2020010112.npz")
    assert sorted(z.files) == ["exceed", "max", "mean", "min", "quantiles", "std"]
    assert z["mean"].shape == (3, T, H, W) and z["quantiles"].shape == (3, 3, T, H, W) and z["exceed"].shape == (2, 3, T, H, W)
    assert z["mean"].dtype == np.float32 and float(z["exceed"][0, 0, 0, 0, 0]) == 2.0
    assert json.loads((tmp_path / "products" / "products.json").read_text()) == meta
    assert meta["channels"] == ["2m_temperature", "geopotential_level500", "mean_sea_level_pressure"] and meta["channel_indices"] == [80, 7, 81]
    assert meta["quantiles"] == [0.1, 0.5, 0.9] and meta["ensemble_size"] == ENS and meta["init_times"] == ["2020010100", "2020010112"]
    assert [(t["channel"], t["direction"], t["threshold"]) for t in meta["thresholds"]] == [("2m_temperature", "gt", 303.15),
                                                                                            ("mean_sea_level_pressure", "lt", 98000.0)]
    with pytest.raises(ValueError):  # --exceed on a channel that is not among --channels
        P.main(argv[:4] + ["--channels", "81", "--exceed", "2m_temperature", "gt", "300"], products=stub)
    with pytest.raises(ValueError):
        P.main(argv[:4] + ["--quantiles", "1.2"], products=stub)
    with pytest.raises(ValueError):
        P.main(argv[:4] + ["--exceed", "81", "lt", "1"] * 9, products=stub)
    meta = P.main(argv[:4] + ["--force_ens_size", "3"], products=lambda p, t: {n: torch.zeros(84, T, H, W) for n in P.PRODUCT_STAT_NAMES})
    assert meta["ensemble_size"] == 3 and len(meta["channels"]) == 84 and meta["thresholds"] == [] and meta["quantiles"] == []
    assert sorted(np.load(tmp_path / "products" / "products_2020010100.npz").files) == ["max", "mean", "min", "std"]
