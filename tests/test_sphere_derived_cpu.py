"""Sphere fields (relative vorticity, divergence) without a device: the command-line parser and the two drivers' file handling with an
injected scorer, `sphere_row_tables` against an independent restatement, the host reference (tests/sphere_refs.py) against the closed
forms of the discrete operator, and header = binding = exported symbols for the new entry point.

Closed forms, for u = U cos(phi), v = 0 (solid-body rotation) on rows `h` radians apart:
  a non-pole row between two rows: zeta = 2 U sin(phi) / R * sin(2h) / (2h)   (cos^2(phi + h) - cos^2(phi - h) = -sin(2 phi) sin(2h))
  a pole row:                      zeta = s U (1 + s sin(phi_jp)) / R          (U cos^2 / (R (1 - s sin)) with cos^2 = (1 - s sin)(1 + s sin))
The inputs are fp32, so the reference sees U cos(phi) rounded: each a_n, a_s is off by at most 2^-24 of itself (half an ulp), which
the operator carries to 2^-24 (|a_n| c_n + |a_s| c_s) |q r|; the result is rounded once more (at most 1 fp32 ulp).  The double
operations themselves err 2^-29 times less."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

from tests import derived_refs as R
from tests import sphere_refs as SR
from tests.test_derived_cpu import DERIVE, U200, U850, V200, V850, _names, _run_main

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VORT = ["--derive", "vort850", "vorticity", U850, V850]
DIV = ["--derive", "div200", "divergence", U200, V200]


# ---- a. parser and drivers -------------------------------------------------------------------------------------------------------------------
def test_parse_sphere_kinds_by_name_and_by_index():
    from ladcast_amd.evaluate import SPHERE_KINDS, Derived, parse_derived
    from ladcast_amd.evaluate.derived import KIND_CHANNELS, KINDS, NONLINEAR_KINDS

    names = _names()
    ix = names.index
    got = parse_derived([VORT[1:], DIV[1:], ["by_index", "vorticity", str(ix(U200)), "5"], ["speed", "speed", U850, V850]], names)
    assert got == [Derived("vort850", "vorticity", (ix(U850), ix(V850))), Derived("div200", "divergence", (ix(U200), ix(V200))),
                   Derived("by_index", "vorticity", (ix(U200), 5)), Derived("speed", "speed", (ix(U850), ix(V850)))]
    assert sorted(KINDS) == ["diff", "divergence", "shear", "speed", "vorticity"] and sorted(SPHERE_KINDS) == ["divergence", "vorticity"]
    assert KIND_CHANNELS["vorticity"] == KIND_CHANNELS["divergence"] == 2 and not set(SPHERE_KINDS) & set(NONLINEAR_KINDS)
    for bad in ([["w", "vorticity", U850]], [["w", "vorticity", U850, V850, U200]], [["w", "divergence", U850]], [["w", "divergence"]],
                [["w", "vorticity", U850, "84"]], [["w", "curl", U850, V850]]):
        with pytest.raises(ValueError):
            parse_derived(bad, names)


def test_field_scales_and_metadata_of_sphere_fields():
    import torch

    from ladcast_amd.evaluate import Derived, derived_metadata
    from ladcast_amd.evaluate.derived import SPHERE_SCALE_LENGTH_M, field_scales

    fields = [Derived("z", "vorticity", (0, 1)), Derived("s", "speed", (0, 1)), Derived("d", "divergence", (2, 3), 2.5e-5)]
    std = torch.arange(1.0, 5.0)
    assert SPHERE_SCALE_LENGTH_M == 1.0e5
    assert field_scales(fields, std) == [math.sqrt(5.0) / 1.0e5, math.sqrt(5.0), 2.5e-5]
    meta = derived_metadata(fields, ["u", "v", "u2", "v2"], std)
    assert meta[0] == dict(name="z", kind="vorticity", channels=[0, 1], channel_names=["u", "v"], index=4, scale=math.sqrt(5.0) / 1.0e5)
    assert set(meta[2]) == {"name", "kind", "channels", "channel_names", "index", "scale"}


def test_main_scores_a_vorticity_field_with_an_anomaly_event(tmp_path):
    names = _names()
    C = len(names)
    out_dir, out = _run_main(tmp_path, "vort", VORT + DIV + ["--event_anomaly", "vort850", "gt", "5e-5", "--event", "div200", "lt", "-0.00001"], C + 2)
    meta = json.loads((out_dir / "derived.json").read_text())
    assert meta["decoded_channels"] == C
    assert meta["derived"][0] == dict(name="vort850", kind="vorticity", channels=[names.index(U850), names.index(V850)], channel_names=[U850, V850],
                                      index=C, scale=None)
    assert meta["derived"][1]["kind"] == "divergence" and meta["derived"][1]["index"] == C + 1
    assert out["ens_acc"].shape == (2, C + 2, 4) and np.load(out_dir / "ens_acc.npy").shape == (2, C + 2, 4)
    ev = json.loads((out_dir / "events.json").read_text())["events"]
    assert [(e["channel"], e["channel_index"], e["anomaly"]) for e in ev] == [("div200", C + 1, False), ("vort850", C, True)]  # plain events first
    with pytest.raises(ValueError, match="anomaly"):  # a speed field still has no climatology, next to a vorticity field or not
        _run_main(tmp_path, "bad", VORT + DERIVE + ["--event_anomaly", "wind_speed_10m", "gt", "5"], C + 4)
    with pytest.raises(ValueError, match="SST"):
        _run_main(tmp_path, "bad", ["--derive", "z", "vorticity", "sea_surface_temperature", V850], C + 1)


def test_products_main_with_a_vorticity_field(tmp_path):
    import torch

    from ladcast_amd.evaluate import products as P
    from ladcast_amd.pipelines.io import save_latent_npy

    names = _names()
    C = len(names)
    ENS, T, H, W = 4, 2, 3, 5
    save_latent_npy(torch.zeros(1, ENS, 2, 1 + T, 2, 2), [2020010100], str(tmp_path / "rollout"))
    stub = lambda path, time_str: dict({n: torch.zeros(1, T, H, W) for n in P.PRODUCT_STAT_NAMES}, exceed=torch.zeros(1, 1, T, H, W))  # noqa: E731
    meta = P.main(["--result_path", str(tmp_path / "rollout"), "--output", str(tmp_path / "products")] + VORT +
                  ["--channels", "vort850", "--exceed", "vort850", "gt", "1e-4"], products=stub)
    assert meta["channels"] == ["vort850"] and meta["channel_indices"] == [C]
    assert meta["derived"] == [dict(name="vort850", kind="vorticity", channels=[names.index(U850), names.index(V850)], channel_names=[U850, V850],
                                    index=C, scale=None)]
    assert json.loads((tmp_path / "products" / "products.json").read_text()) == meta


def test_library_checks_need_no_device():
    from ladcast_amd.evaluate.derived import Derived, _field_list, _runs, check_scoring_fields
    from ladcast_amd.evaluate.utils import Event

    fields = _field_list([("s", "speed", (0, 1)), ("z", "vorticity", (0, 1)), ("d", "diff", (2, 4)), ("dv", "divergence", [5, 6])], 8)
    assert fields[3] == Derived("dv", "divergence", (5, 6))
    check_scoring_fields(fields, 8, 3, [Event(9, "gt", 5e-5, True), Event(11, "lt", 0.0, True), Event(10, "gt", 1.0, True)])  # vorticity, divergence, diff
    with pytest.raises(ValueError, match="anomaly"):
        check_scoring_fields(fields, 8, 3, [Event(8, "gt", 1.0, True)])
    with pytest.raises(ValueError, match="SST"):
        check_scoring_fields(fields, 8, 1)
    for bad in ([("z", "vorticity", (0,))], [("z", "vorticity", (0, 1, 2, 3))], [("z", "divergence", (0, 8))], [("z", "rot", (0, 1))]):
        with pytest.raises(ValueError):
            _field_list(bad, 8)
    assert [(k, [f.name for f in run], sp) for k, run, sp in _runs(fields)] == [(0, ["s"], False), (1, ["z"], True), (2, ["d"], False), (3, ["dv"], True)]
    assert [(k, len(run), sp) for k, run, sp in _runs([fields[1], fields[3], fields[0], fields[2]])] == [(0, 2, True), (2, 2, False)]


# ---- b. the row tables -----------------------------------------------------------------------------------------------------------------------
def _lat_sets():
    from ladcast_amd.evaluate.rollout_metrics import row_latitudes

    return dict(grid120=row_latitudes(120), grid48=row_latitudes(48), both_poles=np.linspace(-90.0, 90.0, 121), no_pole=np.linspace(-88.5, 88.5, 60),
                descending=np.linspace(-90.0, 90.0, 13)[::-1].copy(), uneven=np.array([-90.0, -70.0, -65.0, -10.0, 0.5, 33.0, 80.0]), two=np.array([0.0, 90.0]))


@pytest.mark.parametrize("name", ["grid120", "grid48", "both_poles", "no_pole", "descending", "uneven", "two"])
def test_row_tables_against_the_restatement(name):
    from ladcast_amd.evaluate import sphere_row_tables
    from ladcast_amd.evaluate.derived import EARTH_RADIUS_M

    lat, W = _lat_sets()[name], 240
    tab, k = sphere_row_tables(lat, W)
    assert tab.shape == (4, len(lat)) and tab.dtype == np.float64 and EARTH_RADIUS_M == SR.R_EARTH == 6_371_000.0
    c, q, r, pc, k_ref = SR.row_tables(lat, W)
    pole = 90.0 - np.abs(lat) < 1e-6
    assert np.array_equal(pole, r == 0.0) and np.array_equal(tab[0][pole], np.zeros(int(pole.sum()))) and np.array_equal(tab[2][pole], np.zeros(int(pole.sum())))
    assert np.array_equal(tab[2] == 0.0, pole) and bool((tab[0][~pole] > 0).all()) and np.array_equal(tab[3] != 0.0, pole)
    for got, want in zip(tab, (c, q, r, pc)):  # numpy's and math's cos / sin may differ in the last place
        assert np.allclose(got, want, rtol=4e-16, atol=0.0), name
    assert k == k_ref and abs(k - W / (4.0 * math.pi)) <= 4e-16 * k
    assert bool((np.sign(tab[1]) == np.sign(lat[-1] - lat[0])).all())  # the sign of q follows the order of the rows
    if name == "grid120":
        assert pole.tolist() == [False] * 119 + [True] and abs(tab[3][-1] - math.cos(math.radians(88.5)) / (SR.R_EARTH * (1.0 - math.sin(math.radians(88.5))))) < 1e-18


def test_row_tables_refusals():
    from ladcast_amd.evaluate import sphere_row_tables

    ok = np.linspace(-90.0, 90.0, 7)
    sphere_row_tables(ok, 3)
    for lat, W in ((ok[:1], 8), (ok, 2), (ok, 0), (np.array([0.0, 10.0, 10.0, 20.0]), 8), (np.array([0.0, 10.0, 5.0, 20.0]), 8),
                   (np.array([-91.0, 0.0, 90.0]), 8), (np.array([0.0, 45.0, 90.001]), 8), (np.array([-90.0, 90.0, 95.0]), 8),
                   (np.array([0.0, 90.0 - 1e-7, 90.0]), 8), (np.array([0.0, float("nan"), 90.0]), 8), (np.array([]), 8)):
        with pytest.raises(ValueError):
            sphere_row_tables(lat, W)


# ---- c. the reference against the closed forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(120, 240), (12, 16)])
@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_reference_meets_the_closed_forms(hw, order):
    from ladcast_amd.evaluate import sphere_row_tables
    from ladcast_amd.evaluate.rollout_metrics import row_latitudes

    (H, W), U = hw, 40.0
    lat = row_latitudes(H) if order == "ascending" else row_latitudes(H)[::-1].copy()
    tab, k = sphere_row_tables(lat, W)
    c, q, r, pc = tab
    phi = np.deg2rad(lat)
    h = abs(phi[1] - phi[0])
    u = np.repeat((U * np.cos(phi)).astype(np.float32)[:, None], W, axis=1)
    v = np.zeros((H, W), dtype=np.float32)
    z = SR.field("vorticity", u, v, tab, k).astype(np.float64)
    assert np.isfinite(z).all()
    worst = 0.0
    for j in range(1, H - 1):
        if r[j] == 0.0:
            continue
        want = 2.0 * U * math.sin(phi[j]) / SR.R_EARTH * math.sin(2.0 * h) / (2.0 * h)
        bound = 2.0 ** -24 * (abs(float(u[j + 1, 0])) * c[j + 1] + abs(float(u[j - 1, 0])) * c[j - 1]) * abs(q[j] * r[j]) + float(np.spacing(np.float32(abs(want))))
        err = float(np.abs(z[j] - want).max())
        worst = max(worst, err)
        assert err <= bound, (j, err, bound)
    print(f"{hw} {order}: solid-body rotation met to {worst:.3g} 1/s at interior rows")
    poles = SR.pole_rows(tab)
    assert len(poles) == 1
    for j in poles:
        jp, s = (1 if j == 0 else H - 2), (1.0 if lat[j] > 0 else -1.0)
        want = s * U * (1.0 + s * math.sin(phi[jp])) / SR.R_EARTH
        assert np.abs(z[j] - want).max() <= 2.0 ** -24 * abs(want) + float(np.spacing(np.float32(abs(want)))), (j, z[j, 0], want)
        assert (z[j] == z[j, 0]).all()


@pytest.mark.parametrize("hw", [(120, 240), (12, 16), (7, 5)])
def test_reference_divergence_is_vorticity_of_minus_v_u(hw):
    from ladcast_amd.evaluate import sphere_row_tables

    H, W = hw
    g = np.random.default_rng(5)
    u, v = (g.standard_normal((2, H, W)) * 25.0).astype(np.float32), (g.standard_normal((2, H, W)) * 12.0).astype(np.float32)
    for lat in (np.linspace(-90.0, 90.0, H), np.linspace(-90.0, 90.0, H + 1)[1:], np.linspace(80.0, -80.0, H)):
        tab, k = sphere_row_tables(lat, W)
        for m in range(2):
            d = SR.field("divergence", u[m], v[m], tab, k)
            assert d.dtype == np.float32 and np.isfinite(d).all()
            assert np.array_equal(d.view(np.int32), SR.divergence_direct(u[m], v[m], tab, k).view(np.int32))
            assert np.array_equal(d.view(np.int32), SR.field("vorticity", -v[m], u[m], tab, k).view(np.int32))


def test_reference_nan_rule_and_denormalisation():
    from ladcast_amd.evaluate import sphere_row_tables

    H, W = 6, 8
    tab, k = sphere_row_tables(np.linspace(-90.0, 90.0, H + 1)[1:], W)  # the north pole is the last row
    g = np.random.default_rng(6)
    x = g.standard_normal((3, H, W)).astype(np.float32)
    clean = SR.derive(x, [("z", "vorticity", (0, 1))], 0, tab, k)[0]
    x[0, 2, 0] = np.nan  # u: read by the rows above and below, in the same column
    x[1, 3, W - 1] = np.nan  # v: read by the columns left and right, wrapped
    x[0, H - 2, 5] = np.nan  # u in the row next to the pole: the whole pole row, and row H - 3 in that column
    z = SR.derive(x, [("z", "vorticity", (0, 1))], 0, tab, k)[0]
    want = np.zeros((H, W), dtype=bool)
    want[1, 0] = want[3, 0] = want[3, W - 2] = want[H - 3, 5] = True
    want[H - 1, :] = True
    assert np.array_equal(np.isnan(z), want) and np.array_equal(z[~want], clean[~want])
    mean, std = np.array([1.5, -2.0, 0.25], dtype=np.float32), np.array([0.7, 1.3, 2.1], dtype=np.float32)
    y = g.standard_normal((3, H, W)).astype(np.float32)
    a = R.denorm(y[2], mean[2], std[2], 0.5), R.denorm(y[0], mean[0], std[0], 0.5)
    assert np.array_equal(SR.derive(y, [("d", "divergence", (2, 0))], 0, tab, k, mean, std, 0.5)[0], SR.field("divergence", a[0], a[1], tab, k))


# ---- d. header = binding = exports -----------------------------------------------------------------------------------------------------------
def test_abi_of_the_sphere_entry_point():
    from ladcast_amd import hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    for name in ("ldc_derive_sphere", "ldc_sizeof_sphere_desc"):
        assert re.search(rf"\b{name}\s*\(", header) and name in hip.SIGNATURES and hasattr(hip.lib, name), name
    assert ctypes.sizeof(hip.SphereDesc) == hip.lib.ldc_sizeof_sphere_desc() == 12
    assert (hip.SPHERE_VORTICITY, hip.SPHERE_DIVERGENCE) == tuple(int(re.search(rf"#define LDC_SPHERE_{n} (\d+)", header).group(1)) for n in ("VORTICITY", "DIVERGENCE"))
    assert hip.lib.ldc_abi_version() == hip.ABI_VERSION == 5 and len(hip.SIGNATURES["ldc_derive_sphere"][1]) == 22
    d = hip.sphere_desc([(hip.SPHERE_DIVERGENCE, (3, 4))])
    assert (d[0].kind, d[0].ch[0], d[0].ch[1]) == (1, 3, 4)
    for bad in ([], [(2, (0, 1))], [(0, (0,))], [(0, (0, 1))] * 17):
        with pytest.raises(ValueError):
            hip.sphere_desc(bad)
