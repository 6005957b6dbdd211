"""HIP day-of-year climatology (C ABI ldc_climatology_accumulate / ldc_climatology_smooth, ladcast_amd.preprocess.Climatology and the
compute_climatology command line) against the float64 reference of tests/climatology_refs.py under its accuracy rule
    |out - ref| <= 2^-24 |ref| + 2 (m + 2 window + 4) 2^-53 A / den
(tests/test_climatology_cpu.py holds the reference to exact rational arithmetic, so a failure here is the kernel's).  The raw state is
compared bit for bit: the kernel adds a point's samples in frame order in fp64, as the reference does.  NaN entries and n_empty are exact.

Shapes: the smallest at which each path runs - a single value; the 16-byte and the scalar path; views whose strides differ from the dense
ones (first row cropped and last channel dropped; a column window, aligned and not); a 7-day year for the window's wrap-around with tiles of
31, 32 and 33 points per channel (the 32-point tile then straddles the channel boundary) and 1 point per channel; one case at production
length, 366 days x 4 hours.  sum, count, out and n_empty sit between guard bands; the frames sit inside a larger buffer of finite 1e30
values, so a read outside the view changes a sum."""
import json
from ctypes import c_void_p
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

from tests import climatology_refs as CR
from tests.redzone import UNWRITTEN32, assert_untouched, guarded

pytestmark = pytest.mark.gpu

ARG, ALIGN, UNSUPPORTED = -1, -2, -3
TILE = 32  # points per workgroup of the smooth kernel


@pytest.fixture(scope="module")
def hip():
    from ladcast_amd import hip
    return hip


def _embed(x):
    """the storage array inside a larger device buffer of finite values (16-byte aligned start)"""
    pad = 1024
    flat = torch.full((x.size + 2 * pad,), 1.0e30, dtype=torch.float32, device="cuda")
    flat[pad : pad + x.size] = torch.from_numpy(np.array(x)).reshape(-1).cuda()
    return flat[pad : pad + x.size].view(*x.shape)


def _state(n_slots, shape):
    """zeroed guarded sum (fp64) and count (int32) of n_slots x shape"""
    n = n_slots * int(np.prod(shape))
    S, N = guarded(1, n, dtype=torch.float64), guarded(1, n, dtype=torch.int32)
    S.fill(torch.zeros(n, dtype=torch.float64))
    N.fill(torch.zeros(n, dtype=torch.int32))
    return S, N


def _accumulate(hip, xv, slots, n_slots, S, N, expect=0):
    B, C, H, W = xv.shape
    assert xv.stride(3) == 1 or W == 1
    sl = torch.tensor(slots, dtype=torch.int32, device="cuda")
    st = hip.lib.ldc_climatology_accumulate(hip._p(xv), xv.stride(0), xv.stride(1), max(xv.stride(2), W), B, C, H, W, hip._p(sl), n_slots,
                                            hip._p(S.t), hip._p(N.t), hip._stream())
    torch.cuda.synchronize()
    assert st == expect, st
    assert_untouched(S, "sum")
    assert_untouched(N, "count")


def _frames(seed, shape, kind="offset"):
    """storage frames (B, C, H, W): channel 1 (when there is one) all NaN, frame 0 / channel 0 a NaN checkerboard, a few NaNs elsewhere"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * 3 + (280 if kind == "offset" else 0)
    x = x.astype(np.float32)
    B, C, H, W = shape
    if B * C * H * W > 1:
        x[rng.random(shape) < 0.05] = np.nan
        hh, ww = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        x[0, 0][(hh + ww) % 2 == 0] = np.nan
    if C > 1:
        x[:, 1] = np.nan
    return x


# name -> (storage shape, view, slots, n_slots): frames 0 and 2 share slot 2; -1 and n_slots are skipped; slot 1 and 3 stay empty
SLOTS5 = [2, 0, 2, -1, 4]
ACC_CASES = {
    "one": ((1, 1, 1, 1), np.s_[:], [0], 1),
    "vector": ((5, 3, 4, 8), np.s_[:], SLOTS5, 4),
    "scalar": ((5, 3, 4, 7), np.s_[:], SLOTS5, 4),
    "crop": ((5, 4, 5, 8), np.s_[:, :3, 1:, :], SLOTS5, 4),  # row 0 cropped, the last channel dropped: 16-byte path
    "columns_aligned": ((5, 3, 4, 16), np.s_[:, :, :, 4:12], SLOTS5, 4),  # 16-byte path with a row stride of 16
    "columns_misaligned": ((5, 3, 4, 16), np.s_[:, :, :, 3:11], SLOTS5, 4),  # W % 4 == 0 but a misaligned base: scalar path
    "two_blocks": ((3, 2, 9, 36), np.s_[:], [1, 1, 0], 2),  # 648 points: more than one 256-thread block on the scalar path
    "two_blocks_vector": ((3, 5, 9, 32), np.s_[:], [1, 1, 0], 2),  # 360 groups of 4
}


def _same_bits(S, N, s_ref, n_ref, what):
    got_s, got_n = S.payload().reshape(-1).numpy(), N.payload().reshape(-1).numpy()
    assert np.array_equal(got_n, n_ref.reshape(-1).astype(np.int32)), (what, "count")
    assert np.array_equal(got_s.view(np.int64), s_ref.reshape(-1).view(np.int64)), (what, "sum")


@pytest.mark.parametrize("name", list(ACC_CASES))
def test_accumulate_matches_the_reference_bit_for_bit(hip, name):
    shape, view, slots, n_slots = ACC_CASES[name]
    x = _frames(21, shape)
    xv = _embed(x)[view]
    s_ref, n_ref, _ = CR.accumulate_ref(x[view], slots, n_slots)
    S, N = _state(n_slots, xv.shape[1:])
    _accumulate(hip, xv, slots, n_slots, S, N)
    _same_bits(S, N, s_ref, n_ref, name)
    if name == "one":
        assert S.payload().reshape(-1)[0] == float(x.reshape(-1)[0]) and int(N.payload().reshape(-1)[0]) == 1
    else:
        n4 = n_ref.reshape((n_slots,) + tuple(xv.shape[1:]))
        assert not n4[:, 1].any()  # the all-NaN channel
        B = xv.shape[0]
        used = sum(1 for s in slots if 0 <= s < n_slots)
        assert n4.max() == 2 and used == B - (2 if slots is SLOTS5 else 0)
        if slots is SLOTS5:
            assert not n4[1].any() and not n4[3].any()  # the skipped frames touched nothing
            hh, ww = np.meshgrid(np.arange(xv.shape[2]), np.arange(xv.shape[3]), indexing="ij")
            board = np.isnan(x[view][0, 0])  # the checkerboard of frame 0 (slot 2): counts are exact there
            assert board.sum() >= hh.size // 2 and (n4[2, 0][board] <= 1).all()
    # a second identical call doubles the counts and adds in order
    _accumulate(hip, xv, slots, n_slots, S, N)
    s2, n2, _ = CR.accumulate_ref(np.concatenate([x[view], x[view]]), list(slots) * 2, n_slots)
    _same_bits(S, N, s2, n2, name + " twice")


@pytest.mark.parametrize("W", [8, 7])
def test_batching_does_not_change_the_state(hip, W):
    x = _frames(22, (9, 3, 4, W))
    slots, n_slots = [0, 1, 0, 2, 1, 0, 3, 3, 0], 4
    xv = _embed(x)
    s_ref, n_ref, _ = CR.accumulate_ref(x, slots, n_slots)
    states = []
    for split in ([1] * 9, [4, 5], [9]):
        S, N = _state(n_slots, (3, 4, W))
        i = 0
        for b in split:
            _accumulate(hip, xv[i : i + b], slots[i : i + b], n_slots, S, N)
            i += b
        _same_bits(S, N, s_ref, n_ref, split)
        states.append((S.payload().view(torch.int64), N.payload()))
    for s, n in states[1:]:
        assert torch.equal(s, states[0][0]) and torch.equal(n, states[0][1])


def test_accumulate_argument_errors_write_nothing(hip):
    x = torch.randn(2, 3, 4, 8, device="cuda")
    S, N = guarded(1, 4 * 96, dtype=torch.float64), guarded(1, 4 * 96, dtype=torch.int32)
    sl = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    f = hip.lib.ldc_climatology_accumulate
    X, SL, Sp, Np, st = hip._p(x), hip._p(sl), hip._p(S.t), hip._p(N.t), hip._stream()
    assert f(None, 96, 32, 8, 2, 3, 4, 8, SL, 4, Sp, Np, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, None, 4, Sp, Np, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, SL, 4, None, Np, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, SL, 4, Sp, None, st) == ARG
    assert f(X, 96, 32, 8, 0, 3, 4, 8, SL, 4, Sp, Np, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, SL, 0, Sp, Np, st) == ARG
    assert f(X, 96, 32, 7, 2, 3, 4, 8, SL, 4, Sp, Np, st) == ARG  # rows overlap
    assert f(X, 96, 32, 8, 2, 3, 4, 8, SL, 4, c_void_p(S.t.data_ptr() + 4), Np, st) == ALIGN
    assert f(c_void_p(x.data_ptr() + 2), 96, 32, 8, 2, 3, 4, 8, SL, 4, Sp, Np, st) == ALIGN
    assert f(X, 0, 0, 8, 2, 1 << 16, 1 << 16, 8, SL, 4, Sp, Np, st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert_untouched(S, "sum")
    assert_untouched(N, "count")
    assert bool((N.payload().view(torch.int32) == UNWRITTEN32).all())
    with pytest.raises(RuntimeError):
        hip.climatology_accumulate(torch.zeros(1, 1, 2, 2), sl, S.t, N.t, B=1, C=1, H=2, W=2, n_slots=4, batch_stride=4, channel_stride=4, row_stride=2)


# ---- smooth ----------------------------------------------------------------------------------------------------------------
def _smooth(hip, s, n, g, n_days, n_hours, C, plane, expect=0, with_empty=True):
    """run ldc_climatology_smooth on the reference state (s, n: (n_days * n_hours, C, plane)) between guard bands -> (out, n_empty)"""
    total = n_days * n_hours * C * plane
    S, N = guarded(1, total, dtype=torch.float64), guarded(1, total, dtype=torch.int32)
    S.fill(torch.from_numpy(s.reshape(-1)))
    N.fill(torch.from_numpy(n.reshape(-1).astype(np.int32)))
    O, E = guarded(1, total, dtype=torch.float32), guarded(1, C, dtype=torch.int64)
    E.fill(torch.zeros(C, dtype=torch.int64))
    w = torch.from_numpy(np.asarray(g, dtype=np.float64)).cuda()
    st = hip.lib.ldc_climatology_smooth(hip._p(S.t), hip._p(N.t), hip._p(w), len(g), n_days, n_hours, C, plane, hip._p(O.t),
                                        hip._p(E.t) if with_empty else None, hip._stream())
    torch.cuda.synchronize()
    assert st == expect, st
    for buf, what in ((S, "sum"), (N, "count"), (O, "out"), (E, "n_empty")):
        assert_untouched(buf, what)
    assert np.array_equal(S.payload().reshape(-1).numpy().view(np.int64), s.reshape(-1).view(np.int64))  # the state is only read
    assert np.array_equal(N.payload().reshape(-1).numpy(), n.reshape(-1).astype(np.int32))
    return O, E


def _check_smooth(hip, s, n, a, g, n_days, n_hours, C, plane, what):
    ref, term2, empty = CR.smooth_ref(s, n, a, g, n_days, n_hours)
    O, E = _smooth(hip, s, n, g, n_days, n_hours, C, plane)
    out = O.payload().reshape(ref.shape).numpy()
    r = CR.worst_ratio(out, ref, term2)
    print(f"\nclimatology smooth {what}: worst |out - ref| at {r:.3g} of the rule's bound")
    assert r <= 1.0, (what, r)
    assert E.payload().reshape(-1).tolist() == empty.reshape(n_days * n_hours, C, plane).sum(axis=(0, 2)).tolist(), what
    return out, empty


@pytest.mark.parametrize("plane", [1, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("n_hours", [1, 4])
def test_smooth_seven_day_year(hip, plane, n_hours):
    n_days, C = 7, 2
    empty_point = (1, plane // 2)  # no sample ever: NaN on every day, counted in channel 1
    frames, slots = CR.dataset(31 + plane, n_days, n_hours, (C, plane), kind="offset", empty_day=3, empty_points=[empty_point])
    s, n, a = CR.accumulate_ref(frames, slots, n_days * n_hours)
    assert not n.reshape(n_days, n_hours, C, plane)[3].any()  # a day without a sample inside the windows
    for window, sigma in ((1, 1.0), (3, 1.5), (3, 0.0), (5, 2.0), (7, 2.5), (7, 0.0)):
        g = CR.ref_weights(window, sigma)
        out, empty = _check_smooth(hip, s, n, a, g, n_days, n_hours, C, plane, f"7 days x {n_hours} h, plane {plane}, window {window}, sigma {sigma}")
        assert np.isnan(out[:, :, 1, plane // 2]).all() and empty[:, :, 1, plane // 2].all()
        if window == 1:
            assert np.isnan(out[3]).all()  # the empty day stays empty without neighbours
        if window == 3 and sigma == 0.0:  # the wrap-around, spelled out: day 0 reads day 6, day 6 reads day 0
            s7, n7 = s.reshape(n_days, n_hours, C, plane), n.reshape(n_days, n_hours, C, plane).astype(np.float64)
            with np.errstate(all="ignore"):
                first = (s7[6] + s7[0] + s7[1]) / (n7[6] + n7[0] + n7[1])
                last = (s7[5] + s7[6] + s7[0]) / (n7[5] + n7[6] + n7[0])
            assert np.allclose(out[0], first, rtol=1e-6, atol=0, equal_nan=True) and np.allclose(out[6], last, rtol=1e-6, atol=0, equal_nan=True)


def test_smooth_window_one_returns_a_single_sample_bit_for_bit(hip):
    n_days, n_hours, C, plane = 7, 4, 2, TILE + 1
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((n_days * n_hours, C, plane)) * 50 + 280).astype(np.float32)
    O, E = _smooth(hip, x.astype(np.float64), np.ones(x.shape, np.int64), [1.0], n_days, n_hours, C, plane)
    assert np.array_equal(O.payload().reshape(x.shape).numpy().view(np.int32), x.view(np.int32))
    assert E.payload().reshape(-1).tolist() == [0, 0]
    # without n_empty the output is the same and the counter is left alone
    O2, E2 = _smooth(hip, x.astype(np.float64), np.ones(x.shape, np.int64), [1.0], n_days, n_hours, C, plane, with_empty=False)
    assert torch.equal(O2.payload().view(torch.int32), O.payload().view(torch.int32)) and E2.payload().reshape(-1).tolist() == [0, 0]


@pytest.mark.parametrize("kind", ["offset", "cancel"])
def test_smooth_production_length(hip, kind):
    """366 days x 4 hours, 70 points (two whole tiles and a ragged one; the channel boundary at 35 inside the second), the default window
    (61 days, sigma 10) and the 61-day boxcar; day 366 holds half the samples of the others"""
    n_days, n_hours, C, plane = 366, 4, 2, 35
    rng = np.random.default_rng(9)
    shape = (n_days * n_hours, C, plane)
    base = 280.0 if kind == "offset" else 0.0
    scale = 3.0 if kind == "offset" else 1.0e3
    y1, y2 = ((rng.standard_normal(shape) * scale + base).astype(np.float32) for _ in range(2))
    y1[rng.random(shape) < 0.05] = np.nan
    y1[:, 1, 7] = y2[:, 1, 7] = np.nan  # a land point
    slots = list(range(n_days * n_hours))
    s, n, a = CR.accumulate_ref(np.concatenate([y1, y2[: 365 * n_hours]]), slots + slots[: 365 * n_hours], n_days * n_hours)
    assert n[365 * n_hours :].max() == 1 and n[: 365 * n_hours].max() == 2
    for sigma in (10.0, 0.0):
        out, empty = _check_smooth(hip, s, n, a, CR.ref_weights(61, sigma), n_days, n_hours, C, plane, f"366 days, {kind}, window 61, sigma {sigma}")
        assert empty.sum() == n_days * n_hours and np.isnan(out[:, :, 1, 7]).all()


def test_smooth_argument_errors_write_nothing(hip):
    n_days, n_hours, C, plane = 7, 4, 2, 33
    total = n_days * n_hours * C * plane
    S, N = guarded(1, total, dtype=torch.float64), guarded(1, total, dtype=torch.int32)
    S.fill(torch.ones(total, dtype=torch.float64))
    N.fill(torch.ones(total, dtype=torch.int32))
    O, E = guarded(1, total, dtype=torch.float32), guarded(1, C, dtype=torch.int64)
    E.fill(torch.zeros(C, dtype=torch.int64))
    w = torch.ones(7, dtype=torch.float64, device="cuda")
    f = hip.lib.ldc_climatology_smooth
    Sp, Np, Wp, Op, Ep, st = hip._p(S.t), hip._p(N.t), hip._p(w), hip._p(O.t), hip._p(E.t), hip._stream()
    assert f(None, Np, Wp, 3, n_days, n_hours, C, plane, Op, Ep, st) == ARG
    assert f(Sp, None, Wp, 3, n_days, n_hours, C, plane, Op, Ep, st) == ARG
    assert f(Sp, Np, None, 3, n_days, n_hours, C, plane, Op, Ep, st) == ARG
    assert f(Sp, Np, Wp, 3, n_days, n_hours, C, plane, None, Ep, st) == ARG
    assert f(Sp, Np, Wp, 4, n_days, n_hours, C, plane, Op, Ep, st) == ARG  # even
    assert f(Sp, Np, Wp, 0, n_days, n_hours, C, plane, Op, Ep, st) == ARG
    assert f(Sp, Np, Wp, 9, n_days, n_hours, C, plane, Op, Ep, st) == ARG  # longer than the year
    assert f(Sp, Np, Wp, 3, n_days, 0, C, plane, Op, Ep, st) == ARG
    assert f(c_void_p(S.t.data_ptr() + 4), Np, Wp, 3, n_days, n_hours, C, plane, Op, Ep, st) == ALIGN
    assert f(Sp, Np, Wp, 3, n_days, n_hours, C, plane, c_void_p(O.t.data_ptr() + 2), Ep, st) == ALIGN
    assert f(Sp, Np, Wp, 3, 418, n_hours, C, plane, Op, Ep, st) == UNSUPPORTED  # above the staged column's capacity
    torch.cuda.synchronize()
    for buf, what in ((S, "sum"), (N, "count"), (O, "out"), (E, "n_empty")):
        assert_untouched(buf, what)
    assert bool((O.payload().view(torch.int32) == UNWRITTEN32).all()) and E.payload().reshape(-1).tolist() == [0, 0]
    assert f(Sp, Np, Wp, 7, n_days, n_hours, C, plane, Op, Ep, st) == 0  # and the same buffers are served once the arguments are right
    torch.cuda.synchronize()
    assert bool((O.payload() == 1.0).all()) and E.payload().reshape(-1).tolist() == [0, 0]
    assert_untouched(O, "out")


# ---- the class and the command line ----------------------------------------------------------------------------------------------
def test_climatology_class_two_updates_without_a_synchronisation(hip):
    from ladcast_amd.preprocess import Climatology

    x = _frames(23, (6, 3, 4, 8))
    xv = _embed(x)
    slots = [0, 5, 0, 27, 5, 13]
    clim = Climatology(3, 4, 8, "cuda", n_days=7)
    clim.update(xv[:4], slots[:4]).update(xv[4:], slots[4:])  # back to back on one stream
    s_ref, n_ref, a_ref = CR.accumulate_ref(x, slots, 28)
    torch.cuda.synchronize()
    assert np.array_equal(clim.sum.cpu().numpy().view(np.int64), s_ref.view(np.int64)) and np.array_equal(clim.count.cpu().numpy(), n_ref.astype(np.int32))
    fps = clim.frames_per_slot()
    assert fps.shape == (7, 4) and fps.sum() == 6 and fps[0, 0] == 2 and fps[1, 1] == 2 and fps[6, 3] == 1 and fps[3, 1] == 1
    out = clim.finish(window_days=3, sigma_days=1.0)
    assert out.shape == (7, 4, 3, 4, 8) and out.dtype == torch.float32
    ref, term2, empty = CR.smooth_ref(s_ref, n_ref, a_ref, CR.ref_weights(3, 1.0), 7, 4)
    assert CR.worst_ratio(out.cpu().numpy(), ref, term2) <= 1.0
    assert clim.n_empty().tolist() == empty.sum(axis=(0, 1, 3, 4)).tolist()
    # a channel-sliced, row-cropped view is read in place
    part = Climatology(2, 3, 8, "cuda", n_days=7).update(xv[:, 1:, 1:], slots)
    s2, n2, _ = CR.accumulate_ref(x[:, 1:, 1:], slots, 28)
    assert np.array_equal(part.sum.cpu().numpy().view(np.int64), s2.view(np.int64)) and np.array_equal(part.count.cpu().numpy(), n2.astype(np.int32))
    for bad in (lambda: clim.update(xv[:2], [0]), lambda: clim.update(xv[:1], [28]), lambda: clim.update(xv[:1], [-1]),
                lambda: clim.update(xv[:1, :2], [0]), lambda: clim.update(xv[:1].double(), [0]), lambda: clim.update(xv[:1, :, :, ::2], [0]),
                lambda: clim.finish(window_days=4), lambda: clim.finish(window_days=9)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        clim.update(torch.zeros(1, 3, 4, 8), [0])  # a host tensor


C_E2E, H_E2E, W_E2E = 3, 6, 10


def _exact_frame(t):
    """a frame that is an exact function of (day of year, hour): small integers and halves, exact in fp32 and in every sum"""
    doy, hi = int(t.strftime("%j")), t.hour // 6
    c, h, w = np.meshgrid(np.arange(C_E2E), np.arange(H_E2E), np.arange(W_E2E), indexing="ij")
    return (doy * 4 + hi + 0.5 * c + 8.0 * h - 3.0 * w).astype(np.float32)


@pytest.fixture(scope="module")
def two_years(tmp_path_factory):
    """2020 (leap) and 2021, 6-hourly, in two files, the second starting in 2021: random frames with NaNs, and exact (day, hour) frames"""
    d = tmp_path_factory.mktemp("clim")
    rng = np.random.default_rng(40)
    t0, t1 = datetime(2020, 1, 1), datetime(2021, 1, 1)
    n0, n1 = 366 * 4, 365 * 4
    x = (rng.standard_normal((n0 + n1, C_E2E, H_E2E, W_E2E)) * 5 + 280).astype(np.float32)
    x[rng.random(x.shape) < 0.03] = np.nan
    x[:, 2, 1, 4] = np.nan  # a land point of the last channel
    np.save(d / "y2020.npy", x[:n0])
    np.save(d / "y2021.npy", x[n0:])
    ex = CR.year_frames(t0, n0 + n1, _exact_frame)
    np.save(d / "e2020.npy", ex[:n0])
    np.save(d / "e2021.npy", ex[n0:])
    times = [t0 + timedelta(hours=6 * k) for k in range(n0 + n1)]
    assert times[n0] == t1
    return d, x, ex, times


def test_command_line_on_two_years(hip, two_years):
    from ladcast_amd.evaluate.evaluate_ens_gpu import CLIMATOLOGY_HOURS
    from ladcast_amd.preprocess import compute_climatology as CC

    d, x, _, times = two_years
    frames = ["--frames", f"2020-01-01={d / 'y2020.npy'}", f"2021-01-01T00={d / 'y2021.npy'}"]
    outs = {}
    for block in (2, 0):
        path = d / f"clim_b{block}.npy"
        meta = CC.main(frames + ["--output", str(path), "--channel_block", str(block), "--batch_size", "64"])
        clim = np.load(path, mmap_mode="r")
        assert clim.dtype == np.float32 and clim.shape == (366, 4, C_E2E, H_E2E, W_E2E)
        assert clim.ndim == 5 and clim.shape[:2] == (366, len(CLIMATOLOGY_HOURS))  # the check evaluate_ens_gpu.main applies
        on_disk = json.load(open(d / f"clim_b{block}.json"))
        assert on_disk == json.loads(json.dumps(meta)) and on_disk["channel_block"] == (2 if block else C_E2E)
        fps = np.array(on_disk["frames_per_slot"])
        assert fps.shape == (366, 4) and (fps[:365] == 2).all() and (fps[365] == 1).all()
        assert on_disk["window_days"] == 61 and on_disk["window_sigma_days"] == 10.0 and on_disk["hours"] == [0, 6, 12, 18]
        assert on_disk["first_time"] == "2020-01-01T00:00:00" and on_disk["last_time"] == "2021-12-31T18:00:00" and on_disk["frames"] == len(times)
        assert [f["start"] for f in on_disk["files"]] == ["2020-01-01T00:00:00", "2021-01-01T00:00:00"] and on_disk["step_size_hour"] == 6
        outs[block] = (np.array(clim), on_disk["n_empty"])
    assert np.array_equal(outs[2][0].view(np.int32), outs[0][0].view(np.int32)) and outs[2][1] == outs[0][1]
    s, n, a = CR.accumulate_ref(x, [CR.ref_slot(t) for t in times], 366 * 4)
    ref, term2, empty = CR.smooth_ref(s, n, a, CR.ref_weights(61, 10.0), 366, 4)
    r = CR.worst_ratio(outs[0][0], ref, term2)
    print(f"\ncompute_climatology on two years: worst |out - ref| at {r:.3g} of the rule's bound")
    assert r <= 1.0, r
    assert outs[0][1] == empty.sum(axis=(0, 1, 3, 4)).tolist() == [0, 0, 366 * 4]


def test_command_line_table_plugs_into_the_scorers_indexing(hip, two_years):
    from ladcast_amd.evaluate.evaluate_ens_gpu import climatology_slots
    from ladcast_amd.preprocess import compute_climatology as CC

    d, _, ex, times = two_years
    path = d / "clim_exact.npy"
    meta = CC.main(["--frames", f"2020-01-01={d / 'e2020.npy'}", f"2021-01-01={d / 'e2021.npy'}", "--output", str(path), "--window_days", "1",
                    "--batch_size", "64"])
    assert meta["n_empty"] == [0, 0, 0] and meta["window_days"] == 1
    flat = np.load(path).reshape(-1, C_E2E, H_E2E, W_E2E)
    for init in ("2021-02-28T12", "2020-02-28T12", "2020-12-31T06", "2021-12-30T18"):
        k = times.index(datetime.fromisoformat(init))
        truth = ex[k + 1 : k + 5]  # the four frames after the initial time
        got = flat[climatology_slots(init, 24)]
        assert np.array_equal(got.view(np.int32), truth.view(np.int32)), init
    # the date filter: 2021 alone leaves day 366 without a sample
    sub = d / "clim_2021.npy"
    meta = CC.main(["--frames", f"2020-01-01={d / 'e2020.npy'}", f"2021-01-01={d / 'e2021.npy'}", "--output", str(sub), "--window_days", "1",
                    "--start_date", "2021-01-01", "--end_date", "2021-12-31T18", "--channel_block", "1"])
    assert meta["frames"] == 365 * 4 and [f["frames_used"] for f in meta["files"]] == [0, 365 * 4] and meta["n_empty"] == [4 * H_E2E * W_E2E] * 3
    t2021 = np.load(sub)
    assert np.isnan(t2021[365]).all() and np.array_equal(t2021[:365].view(np.int32), flat.reshape(366, 4, C_E2E, H_E2E, W_E2E)[:365].view(np.int32))
