"""The oracle, the bound and the planted defects of tests/spectrum_refs.py judged on the CPU, the host-side argument checks of
`evaluate.rollout_spectrum`, the two new symbols, and the host side of the driver's `--spectrum` flag with stubbed scores.  No GPU: the
kernel itself is run by tests/test_gpu_spectrum.py."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import spectrum_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    for shape in R.SHAPES:
        yield str(shape), R.case(shape)
    yield "pivot", R.pivot_case()
    yield "NaN row", R.nan_case(False)
    yield "NaN in a zero-weight row", R.nan_case(True)


CASES = dict(_cases())
_REF = {}


def ref_of(name):
    if name not in _REF:
        c = CASES[name]
        _REF[name] = R.spectrum_ref(c["x"], c["t"], c["w"])
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_within_the_bound(name):
    c = CASES[name]
    r = R.check(R.kernel_f32(c["x"], c["t"], c["w"]), ref_of(name), name)
    print(f"{name}: worst err / bound {r:.4f}")


@pytest.mark.parametrize("name", list(CASES))
def test_parseval(name):
    """sum_k of each plane is the weighted mean of the rows' mean squares, within the bound summed over k"""
    c = CASES[name]
    got, ref, ms = R.kernel_f32(c["x"], c["t"], c["w"]), ref_of(name), R.mean_square_ref(c["x"], c["t"], c["w"])
    for i, k in enumerate(R.NAMES):
        err, bound = np.abs(got[k].astype(np.float64).sum(-1) - ms[i]), ref[k][1].sum(-1)
        assert (err <= bound).all(), (name, k, float(err.max()), float(bound.max()))
        assert np.abs(ref[k][0].sum(-1) - ms[i]).max() <= 1e-12 * np.abs(ms[i]).max()  # the oracle itself


def test_pivot_case_is_what_the_issue_asks():
    """mean 2e5, amplitude 1e-2 at k0 = W / 2 - 1: the oracle's own P_k0 is at least 100 x the pivoted bound, the pivoted restatement
    passes, the unpivoted one misses by orders of magnitude, and so does an fp32 torch.fft.rfft of the raw rows"""
    c, ref = R.pivot_case(), ref_of("pivot")
    k0 = c["k0"]
    assert k0 == R.PIVOT_W // 2 - 1 and abs(float(c["t"].mean()) - R.PIVOT_MEAN) < 1.0
    for k in R.NAMES:
        val, bnd = ref[k][0][0, 0, k0], ref[k][1][0, 0, k0]
        print(f"{k}: P_k0 = {val:.4e}, bound {bnd:.3e}, ratio {val / bnd:.0f}")
        assert val >= 100 * bnd
    R.check(R.kernel_f32(c["x"], c["t"], c["w"]), ref, "pivoted")
    bad = R.kernel_f32(c["x"], c["t"], c["w"], defect="unpivoted")
    tc = R.torch_composition_f32(c["x"], c["t"], c["w"])
    for k in R.NAMES:
        r_bad = R.ratio_of(bad[k][..., 1:], (ref[k][0][..., 1:], ref[k][1][..., 1:]))
        r_tc = R.ratio_of(tc[k].numpy()[..., 1:], (ref[k][0][..., 1:], ref[k][1][..., 1:]))
        print(f"{k}: unpivoted fp32 err / bound {r_bad:.3g}, torch fp32 composition {r_tc:.3g}")
        assert r_bad > 100


# every planted defect fails the same bound on the case named for it (and is listed with every other case that catches it)
NAMED = dict(unpivoted="pivot", nyquist_2="(3, 2, 2, 3, 8)", s_1="(3, 1, 1, 2, 240)", mean_of_spectra="(70, 1, 1, 2, 8)", nan_row_kept="NaN row",
             zero_row_read="NaN in a zero-weight row", fold_drops_half="(2, 2, 1, 3, 6)")


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for name, c in CASES.items():
        try:
            R.check(R.kernel_f32(c["x"], c["t"], c["w"], defect=defect), ref_of(name), name)
        except AssertionError:
            caught.append(name)
    print(f"{defect}: caught by {caught}")
    assert NAMED[defect] in caught, (defect, caught)


def test_nan_rows_and_zero_weight_rows():
    clean = R.case((3, 2, 2, 3, 8))
    base = R.kernel_f32(clean["x"], clean["t"], clean["w"])
    c = R.nan_case(False)
    ref, got = R.spectrum_ref(c["x"], c["t"], c["w"]), R.kernel_f32(c["x"], c["t"], c["w"])
    assert ref["n_invalid"].tolist() == [[0, 0], [1, 0]] and np.isfinite(got["spec_members"]).all()
    for k in R.NAMES:  # the other (c, l) are untouched
        assert np.array_equal(got[k][0], base[k][0]) and np.array_equal(got[k][1, 1], base[k][1, 1]) and not np.array_equal(got[k][1, 0], base[k][1, 0])
    z = R.nan_case(True)
    refz = R.spectrum_ref(z["x"], z["t"], z["w"])
    assert refz["n_invalid"].tolist() == [[0, 0], [0, 0]]
    x = clean["x"].copy()
    x[0, 0, 0, :, 0] = np.nan  # every row of (c, l) = (0, 0)
    ref = R.spectrum_ref(x, clean["t"], clean["w"])
    assert ref["n_invalid"].tolist() == [[3, 0], [0, 0]] and all(np.isnan(ref[k][0][0, 0]).all() and np.isfinite(ref[k][0][1]).all() for k in R.NAMES)
    R.check(R.kernel_f32(x, clean["t"], clean["w"]), ref)


@pytest.mark.parametrize("W,k0", [(8, 1), (8, 3), (8, 4), (6, 1), (6, 2), (6, 3)])
def test_pure_tones_in_the_oracle(W, k0):
    y, want = R.pure_tone(W, k0, 3.0, 5.0)
    ref = R.spectrum_ref(y[None, None, None], y[None, None], np.ones(2, np.float32))
    assert np.abs(ref["spec_truth"][0][0, 0] - want).max() <= (ref["spec_truth"][1][0, 0]).max()


# ---- host-side argument checks: the documented exception before any device call ---------------------------------------------------------
def _call(M=2, C=1, L=1, H=3, W=8, w=None, **kw):
    from ladcast_amd.evaluate import rollout_spectrum

    x, t = torch.zeros(M, C, L, H, W), torch.zeros(C, L, H, W)
    return rollout_spectrum(x, t, torch.ones(H) if w is None else w, **kw)


@pytest.mark.parametrize("kw,match", [(dict(W=7), "even W"), (dict(W=2), "even W"), (dict(W=514), "even W"), (dict(w=torch.ones(4)), "one value per latitude row"),
                                      (dict(w=torch.tensor([1.0, -0.5, 1.0])), "non-negative"), (dict(w=torch.tensor([1.0, float("nan"), 1.0])), "non-negative"),
                                      (dict(M=1025), "members")])
def test_host_side_argument_checks(kw, match):
    with pytest.raises(ValueError, match=match):
        _call(**kw)


def test_valid_host_arguments_reach_the_device_check():
    with pytest.raises(RuntimeError, match="device tensors"):
        _call()


# ---- the symbols ------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_export_both_symbols():
    from ladcast_amd import hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    assert re.search(r"long long ldc_rollout_spectrum_workspace_bytes\(int M, int C, int L, int H, int W\);", header)
    assert re.search(r"\nint ldc_rollout_spectrum\(const float\* forecast,", header)
    assert "#define LDC_ABI_VERSION 5" in header
    so = os.path.join(ROOT, "ladcast_amd", "libladcast_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert " T ldc_rollout_spectrum\n" in syms and " T ldc_rollout_spectrum_workspace_bytes\n" in syms
    q = hip.lib.ldc_rollout_spectrum_workspace_bytes
    for shape in R.SHAPES + ((50, 84, 4, 120, 240),):
        assert q(*shape) == R.workspace_bytes(*shape)
    for bad in ((0, 1, 1, 1, 8), (1025, 1, 1, 1, 8), (1, 1, 1, 1, 7), (1, 1, 1, 1, 2), (1, 1, 1, 1, 514), (1, 65536, 1, 1, 8), (1, 1, 1, 1 << 22, 8)):
        assert q(*bad) == 0, bad
    assert hip.lib.ldc_rollout_spectrum.restype is not None and callable(hip.rollout_spectrum)


# ---- the driver's flag with stubbed scores ----------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
NEW = ("spec_members", "spec_mean", "spec_truth", "spec_n_invalid")


def _run(tmp_path, spectrum, out_name):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    res.mkdir(exist_ok=True)
    for ts in (2018123000, 2018123118):
        np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    C, T, K = 3, 4, 5
    calls = []

    def score(path, time_str, t_slots, c_slots):
        calls.append(time_str)
        n = len(calls)
        out = {k: np.full((C, T), float(n + i), dtype=np.float32) for i, k in enumerate(SCORES)}
        if spectrum:
            out.update({k: torch.full((C, T, K), float(10 * n + i)) for i, k in enumerate(NEW[:3])}, spec_n_invalid=torch.full((C, T), n, dtype=torch.int32))
        return out

    out_dir = tmp_path / out_name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + (["--spectrum"] if spectrum else []), score=score)
    return out, out_dir, (C, T, K)


def test_driver_gathers_the_spectra_per_initial_time(tmp_path):
    plain, plain_dir, _ = _run(tmp_path, False, "plain")
    out, out_dir, (C, T, K) = _run(tmp_path, True, "spec")
    assert sorted(p.name for p in out_dir.iterdir()) == sorted([p.name for p in plain_dir.iterdir()] + [f"{k}.npy" for k in NEW])
    for p in plain_dir.iterdir():  # the files of a run without the flag, byte for byte
        assert (out_dir / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(out_dir / f"{k}.npy") for k in NEW}
    for i, k in enumerate(NEW[:3]):
        assert a[k].shape == (2, C, T, K) and a[k].dtype == np.float32 and (a[k][0] == 10 + i).all() and (a[k][1] == 20 + i).all()
    assert a["spec_n_invalid"].shape == (2, C, T) and a["spec_n_invalid"].dtype == np.int32 and (a["spec_n_invalid"][1] == 2).all()
    assert not any(k in plain for k in NEW)


def test_driver_refuses_a_scorer_without_spectra(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    res.mkdir()
    np.save(res / "latent_2018010100.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    plain = {k: np.zeros((3, 4), dtype=np.float32) for k in SCORES}
    with pytest.raises(ValueError, match="spectrum"):
        EG.main(["--result_path", str(res), "--output", str(tmp_path / "o"), "--end_date", "2018-02-01", "--total_lead_time_hour", "24", "--spectrum"],
                score=lambda *a: plain)


def test_latitude_band_weights():
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    w = EG.lat_weights_for(120)
    lat = EG.row_latitudes(120)
    b = EG.spectrum_band_weights(w, lat, (30.0, 60.0))
    inside = (lat >= 30) & (lat <= 60)
    assert inside.sum() == 21 and torch.equal(b[torch.from_numpy(inside)], w[torch.from_numpy(inside)]) and float(b[torch.from_numpy(~inside)].abs().sum()) == 0.0
    assert EG.spectrum_band_weights(w, lat, None) is w
    with pytest.raises(ValueError):
        EG.spectrum_band_weights(w, lat, (95.0, 99.0))
    assert len(EG.row_latitudes(48)) == 48 and EG.row_latitudes(48)[-1] == 90.0
