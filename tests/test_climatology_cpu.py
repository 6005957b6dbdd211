"""CPU checks of the day-of-year climatology (ladcast_amd.preprocess.climatology / compute_climatology, C ABI ldc_climatology_accumulate
and ldc_climatology_smooth): the new C ABI entries and what they refuse before touching the device, the slot and window helpers against
the scorer's own indexing, the float64 reference of tests/climatology_refs.py against exact rational arithmetic under the accuracy rule
(so a GPU failure is the kernel's), and what the command line refuses before touching the device."""
import os
import re
from ctypes import c_void_p
from datetime import datetime, timedelta
from fractions import Fraction

import numpy as np
import pytest

from tests import climatology_refs as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ldc_climatology_accumulate", "ldc_climatology_smooth")
ARG, ALIGN, UNSUPPORTED = -1, -2, -3


def test_header_declares_library_exports_and_binding_lists_the_entries():
    from ladcast_amd import hip

    with open(os.path.join(ROOT, "include", "ladcast_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in hip.SIGNATURES and hasattr(hip.lib, name)
    assert re.search(r"#define\s+LDC_ABI_VERSION\s+5\b", header) and hip.ABI_VERSION == 5 and hip.lib.ldc_abi_version() == 5
    assert callable(hip.climatology_accumulate) and callable(hip.climatology_smooth)


def test_makefile_builds_the_source_without_contraction():
    with open(os.path.join(ROOT, "ladcast_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "climatology.hip" in srcs
    assert re.search(r"^EXTRA_climatology\s*=\s*-ffp-contract=off\s*$", mk, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "ladcast_amd", "csrc", "climatology.hip"))


def test_argument_errors_return_before_the_device():
    """pointers that are never dereferenced: every one of these calls returns from the host-side checks"""
    from ladcast_amd import hip

    acc, smooth = hip.lib.ldc_climatology_accumulate, hip.lib.ldc_climatology_smooth
    P, st = c_void_p(1 << 20), None  # an aligned non-null address; the null stream
    ok_acc = dict(x=P, sb=96, sc=32, sr=8, B=2, C=3, H=4, W=8, slots=P, n_slots=4, sum=P, count=P)
    call_acc = lambda **kw: acc(*[{**ok_acc, **kw}[k] for k in ok_acc], st)  # noqa: E731
    for name in ("x", "slots", "sum", "count"):
        assert call_acc(**{name: None}) == ARG, name
    for kw in (dict(B=0), dict(C=-1), dict(H=0), dict(W=0), dict(n_slots=0), dict(sr=7)):  # sr = 7 < W: rows overlap
        assert call_acc(**kw) == ARG, kw
    assert call_acc(x=c_void_p((1 << 20) + 2)) == ALIGN and call_acc(sum=c_void_p((1 << 20) + 4)) == ALIGN
    assert call_acc(count=c_void_p((1 << 20) + 1)) == ALIGN and call_acc(slots=c_void_p((1 << 20) + 2)) == ALIGN
    assert call_acc(C=1 << 16, H=1 << 16, sr=8) == UNSUPPORTED  # C * H = 2^32 rows

    ok_sm = dict(sum=P, count=P, weights=P, window=3, n_days=7, n_hours=4, C=2, plane=33, out=P, n_empty=P)
    call_sm = lambda **kw: smooth(*[{**ok_sm, **kw}[k] for k in ok_sm], st)  # noqa: E731
    for name in ("sum", "count", "weights", "out"):
        assert call_sm(**{name: None}) == ARG, name
    for kw in (dict(window=4), dict(window=0), dict(window=-1), dict(window=9), dict(n_days=0), dict(n_hours=0), dict(C=0), dict(plane=0)):
        assert call_sm(**kw) == ARG, kw  # even, < 1, > n_days, non-positive sizes
    assert call_sm(sum=c_void_p((1 << 20) + 4)) == ALIGN and call_sm(out=c_void_p((1 << 20) + 2)) == ALIGN
    assert call_sm(weights=c_void_p((1 << 20) + 4)) == ALIGN and call_sm(n_empty=c_void_p((1 << 20) + 4)) == ALIGN
    assert call_sm(n_days=418, window=61) == UNSUPPORTED  # above the staged column's capacity (417 days)
    assert call_sm(n_days=366, window=61, plane=1 << 40, C=1 << 30) == UNSUPPORTED


SWEEP = [("2019-03-01", 59 * 4), ("2020-02-29", 59 * 4), ("2020-03-01", 60 * 4), ("2020-12-31T18", 365 * 4 + 3), ("2021-12-31T18", 364 * 4 + 3),
         ("2021-01-01T06", 1), (2018010112, 2), (np.datetime64("2020-07-04T18"), None), (datetime(2019, 12, 31, 0), 364 * 4)]


def test_slot_of_is_the_scorers_index():
    from ladcast_amd.evaluate.evaluate_ens_gpu import CLIMATOLOGY_HOURS, climatology_slots
    from ladcast_amd.preprocess import frame_slots, slot_of

    assert tuple(CLIMATOLOGY_HOURS) == CR.HOURS
    for t, want in SWEEP:
        got = slot_of(t)
        assert got == climatology_slots(t, 0, exclude_start=False)[0], t
        assert want is None or got == want, (t, got, want)
    t0 = datetime(2019, 12, 30)
    for k in range(0, 4 * 800):  # every 6-hourly time of more than two years, a leap year among them
        t = t0 + timedelta(hours=6 * k)
        assert slot_of(t) == climatology_slots(t, 0, exclude_start=False)[0] == CR.ref_slot(t)
    assert frame_slots("2020-12-31T12", 4, 6) == [365 * 4 + 2, 365 * 4 + 3, 0, 1]
    assert frame_slots("2020-02-28", 3, 24) == [58 * 4, 59 * 4, 60 * 4] and frame_slots("2020-01-01", 0, 6) == []
    for bad in ("2020-01-01T03", "2020-01-01T06:30", datetime(2020, 1, 1, 6, 0, 1), 2020010105):
        with pytest.raises(ValueError):
            slot_of(bad)
    with pytest.raises(ValueError):
        frame_slots("2020-01-01", 3, 4)  # 04:00 is off the grid


def test_window_weights():
    from ladcast_amd.preprocess import window_weights

    for w, sigma in ((1, 10.0), (3, 1.5), (7, 2.0), (61, 10.0)):
        g = window_weights(w, sigma)
        assert g.dtype == np.float64 and g.shape == (w,) and g[w // 2] == 1.0 and np.array_equal(g, g[::-1])
        assert np.allclose(g, CR.ref_weights(w, sigma), rtol=1e-15, atol=0) and bool((np.diff(g[: w // 2 + 1]) > 0).all())
    assert window_weights(61, 10.0)[0] == pytest.approx(np.exp(-900.0 / 200.0), rel=1e-15)
    for sigma in (0.0, -1.0):
        assert np.array_equal(window_weights(5, sigma), np.ones(5))
    for bad in (0, 2, 60, -3):
        with pytest.raises(ValueError):
            window_weights(bad, 10.0)


@pytest.mark.parametrize("kind", ["plain", "offset", "cancel"])
@pytest.mark.parametrize("window,sigma", [(1, 1.0), (3, 1.5), (5, 0.0), (7, 2.0)])
def test_reference_agrees_with_rational_arithmetic(kind, window, sigma):
    """the float64 reference is within the rule's fp64 term of exact arithmetic (hence the doubled term when a kernel is held
    against the reference), and its fp32 rounding within the whole rule"""
    n_days, n_hours, tail = 7, 2, (3,)
    frames, slots = CR.dataset(11, n_days, n_hours, tail, kind=kind, empty_day=3, empty_points=[(2,)])
    s, n, a = CR.accumulate_ref(frames, slots, n_days * n_hours)
    g = CR.ref_weights(window, sigma)
    ref, term2, empty = CR.smooth_ref(s, n, a, g, n_days, n_hours)
    assert empty[:, :, 2].all() and (window < 7 or not empty[:, :, :2].any())
    worst = 0.0
    for d in range(n_days):
        for h in range(n_hours):
            for p in range(tail[0]):
                by_day = [[x[p] for x, sl in zip(frames, slots) if sl == dd * n_hours + h and not np.isnan(x[p])] for dd in range(n_days)]
                ex = CR.exact_point(by_day, g, d)
                assert (ex is None) == bool(empty[d, h, p]) == bool(np.isnan(ref[d, h, p]))
                if ex is None:
                    continue
                val, a_over_den, m = ex
                t2 = Fraction(m + 2 * window + 4) * Fraction(CR.U64) * a_over_den
                assert abs(Fraction(float(ref[d, h, p])) - val) <= t2, (d, h, p)
                assert abs(Fraction(float(term2[d, h, p])) - t2) <= t2 * Fraction(1, 1 << 40)  # the reference states the same bound
                err32 = abs(Fraction(float(np.float32(ref[d, h, p]))) - val)
                bound = Fraction(CR.U32) * abs(val) + t2
                assert err32 <= bound
                worst = max(worst, float(err32 / bound))
    print(f"\n{kind} window {window}: fp32(reference) at {worst:.3g} of the rule's bound")


def test_reference_window_one_is_the_slot_mean_and_the_day_axis_wraps():
    frames, slots = CR.dataset(5, 7, 1, (2,), kind="plain", max_per_slot=2, nan_frac=0.0)
    s, n, a = CR.accumulate_ref(frames, slots, 7)
    ref, _, empty = CR.smooth_ref(s, n, a, CR.ref_weights(1, 0.0), 7, 1)
    with np.errstate(all="ignore"):
        assert np.array_equal(ref[:, 0], np.where(n > 0, s / n, np.nan), equal_nan=True)
    ref3, _, _ = CR.smooth_ref(s, n, a, CR.ref_weights(3, 0.0), 7, 1)
    assert np.allclose(ref3[0, 0], (s[6] + s[0] + s[1]) / (n[6] + n[0] + n[1]), rtol=1e-14)
    assert np.allclose(ref3[6, 0], (s[5] + s[6] + s[0]) / (n[5] + n[6] + n[0]), rtol=1e-14)


def test_climatology_class_and_command_line_refuse_before_the_device(tmp_path):
    from ladcast_amd.preprocess import Climatology
    from ladcast_amd.preprocess import compute_climatology as CC

    with pytest.raises(RuntimeError):
        Climatology(3, 4, 8, device="cpu")
    with pytest.raises(ValueError):
        Climatology(0, 4, 8)
    np.save(tmp_path / "a.npy", np.zeros((4, 3, 4, 8), dtype=np.float32))
    np.save(tmp_path / "b.npy", np.zeros((4, 3, 5, 8), dtype=np.float32))
    np.save(tmp_path / "f64.npy", np.zeros((4, 3, 4, 8), dtype=np.float64))
    out = str(tmp_path / "clim.npy")
    a, b, f64 = (str(tmp_path / n) for n in ("a.npy", "b.npy", "f64.npy"))
    cases = [
        (["--frames", a], "malformed START=PATH"),
        (["--frames", "=" + a], "empty START"),
        (["--frames", "someday=" + a], "START is no date"),
        (["--frames", "2020-01-01T03=" + a], "off the 0 / 6 / 12 / 18 grid"),
        (["--frames", "2020-01-01=" + a, "--step_size_hour", "4"], "the second frame is at 04:00"),
        (["--frames", "2020-01-01=" + a, "--window_days", "60"], "even window"),
        (["--frames", "2020-01-01=" + a, "--window_days", "367"], "window longer than the year"),
        (["--frames", "2020-01-01=" + a, "2020-01-02=" + b], "mismatched shapes"),
        (["--frames", "2020-01-01=" + f64], "not float32"),
        (["--frames", "2020-01-01=" + a, "--start_date", "2020-02-01"], "no frames left"),
        (["--frames", "2020-01-01=" + a, "--end_date", "2019-12-31T18"], "no frames left"),
        (["--frames", "2020-01-01=" + a, "--batch_size", "0"], "batch size"),
    ]
    for argv, why in cases:
        with pytest.raises(SystemExit) as e:
            CC.main(argv + ["--output", out])
        assert e.value.code not in (0, None), why
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "clim.json"))
    # the date filter keeps the frames in [start, end], both ends included
    t0 = datetime(2020, 1, 1)
    ranges, slots, times = CC.select_frames([t0, t0 + timedelta(days=1)], [4, 4], 6, datetime(2020, 1, 1, 12), datetime(2020, 1, 2, 6))
    assert ranges == [(2, 4), (0, 2)] and slots == [2, 3, 4, 5] and min(times) == datetime(2020, 1, 1, 12) and max(times) == datetime(2020, 1, 2, 6)
    assert CC.select_frames([t0], [4], 6, datetime(2020, 1, 1, 1), None)[0] == [(1, 4)]
    assert CC.pick_channel_block(84, 121 * 240, 32, 1 << 40) == 84 and CC.pick_channel_block(84, 121 * 240, 32, 1 << 20) == 0
    per = 366 * 4 * 121 * 240 * 16 + 2 * 32 * 121 * 240 * 4
    assert CC.pick_channel_block(84, 121 * 240, 32, (12 * per) * 10 // 9 + 10) == 12
