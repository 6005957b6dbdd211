"""HIP streaming moments (C ABI ldc_field_moments, ladcast_amd.preprocess.FieldMoments) against the exact-arithmetic oracle of
tests/preprocess_oracle.py under its accuracy rule: |mean - exact| and |std - exact| <= 2^-34 std_exact, counts exact, a constant
channel's std exactly 0.  tests/test_preprocess_cpu.py holds numpy's float64 statistics to the same rule on every input used here, so a
failure is the kernel's.

Shapes: the smallest at which each path of the kernel runs - a single value; the scalar and the 16-byte path; a plane smaller than one
4096-value chunk; several chunks of whole rows with a ragged last one (both paths); a row longer than a chunk, cut into pieces (both
paths); views whose strides differ from the dense ones (first row cropped and last channel dropped; a column window, aligned and not).
`state` and the workspace sit between guard bands; the input sits inside a larger buffer of finite 1e30 values, so a read outside the
view changes a count."""
import math
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from tests import preprocess_oracle as PO
from tests.redzone import UNWRITTEN64, assert_untouched, guarded

pytestmark = pytest.mark.gpu

WORST = {}  # case -> worst ratio to the rule's bound (printed; tools/field_moments_bench.py records its own)


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


def _device_view(name):
    x, view, want = PO.case(name)
    return _embed(x)[view], want


def _call(hip, xv, state, accumulate, ws=None, check=True):
    B, C, H, W = xv.shape
    nbytes = hip.lib.ldc_field_moments_workspace_bytes(B, C, H, W)
    assert nbytes == (nbytes // 32) * 32 > 0
    ws = ws if ws is not None else guarded(1, nbytes // 8, dtype=torch.float64)
    assert xv.stride(3) == 1 or W == 1
    st = hip.lib.ldc_field_moments(hip._p(xv), xv.stride(0), xv.stride(1), max(xv.stride(2), W), B, C, H, W, hip._p(state.t), accumulate,
                                   c_void_p(ws.t.data_ptr()), nbytes, hip._stream())
    torch.cuda.synchronize()
    if check:
        assert st == 0, st
        assert_untouched(state, "state")
        assert_untouched(ws, "workspace")
    return st


def _stats(state, C):
    s = state.payload().reshape(C, 3).numpy()
    with np.errstate(all="ignore"):
        return s[:, 0], s[:, 1], np.sqrt(s[:, 2] / s[:, 0]), s[:, 2]


def _check(name, state, want, what=""):
    n, mean, std, m2 = _stats(state, len(want))
    assert [float(v) for v in n] == [float(w["n"]) for w in want], (name, what, n)
    for c, w in enumerate(want):
        if w["n"] == 0:
            assert math.isnan(mean[c]) and math.isnan(m2[c]), (name, c)
        if w["std"] == 0.0:
            assert m2[c] == 0.0 and not np.signbit(m2[c]), (name, c, m2[c])  # bitwise +0
    ratios = [PO.rule_ratios(float(m), float(s), w) for m, s, w in zip(mean, std, want)]
    r = max(max(p) for p in ratios)
    WORST[name + what] = max(r, WORST.get(name + what, 0.0))
    print(f"\nfield moments {name}{what}: worst |mean - exact| {max(p[0] for p in ratios):.3g}, |std - exact| {max(p[1] for p in ratios):.3g} of the 2^-34 std bound")
    assert r <= 1.0, (name, what, ratios)
    return r


@pytest.mark.parametrize("name", [k for k in PO.CASES if k != "stream"])
def test_against_the_exact_oracle_with_guard_bands(hip, name):
    xv, want = _device_view(name)
    C = xv.shape[1]
    state = guarded(1, 3 * C, dtype=torch.float64)
    _call(hip, xv, state, 0)
    _check(name, state, want)
    if name == "one":
        s = state.payload().reshape(3)
        assert s[0] == 1.0 and s[1] == float(PO.case("one")[0].reshape(-1)[0]) and s[2] == 0.0
    if name == "nan_mix":
        n, mean, std, _ = _stats(state, C)
        x = PO.case(name)[0]
        assert n[0] == 0 and n[2] == 1 and mean[2] == float(x[1, 2, 5, 7]) and std[2] == 0.0
        assert std[3] == 0.0 and mean[3] == float(x[0, 3, 0, 0])  # the constant channel: the value itself, std exactly 0
        assert n[1] == 2 * (16 * 24 - 112)  # 112 of 384 points (29 %) are land, and one of the three frames is all NaN
    # accumulate = 0 over a state prefilled with garbage: the garbage is ignored (same bits as over the NaN-patterned fresh state)
    state2 = guarded(1, 3 * C, dtype=torch.float64)
    state2.fill(torch.tensor([7.0, -1.0e300, 123.0] * C, dtype=torch.float64))
    _call(hip, xv, state2, 0)
    assert torch.equal(state.payload().view(torch.int64), state2.payload().view(torch.int64))


def _stream_sequence(hip, xv, C):
    state = guarded(1, 3 * C, dtype=torch.float64)
    i = 0
    for k, b in enumerate(PO.STREAM_SPLIT):
        _call(hip, xv[i : i + b], state, 0 if k == 0 else 1)
        i += b
    return state


def test_streaming_matches_one_call_and_repeats_bit_equal(hip):
    xv, want = _device_view("stream")
    C = xv.shape[1]
    whole = guarded(1, 3 * C, dtype=torch.float64)
    _call(hip, xv, whole, 0)
    _check("stream", whole, want, " (one call)")
    s1 = _stream_sequence(hip, xv, C)
    _check("stream", s1, want, " (batches of 1, 3, 2)")
    s2 = _stream_sequence(hip, xv, C)
    assert torch.equal(s1.payload().view(torch.int64), s2.payload().view(torch.int64))
    # a batch without a valid value leaves the state alone; an empty state takes the batch
    nan = torch.full_like(xv[:1], float("nan"))
    _call(hip, nan, s2, 1)
    assert torch.equal(s1.payload().view(torch.int64), s2.payload().view(torch.int64))
    s3 = guarded(1, 3 * C, dtype=torch.float64)
    _call(hip, nan, s3, 0)
    assert s3.payload().reshape(C, 3)[:, 0].tolist() == [0.0] * C and bool(torch.isnan(s3.payload().reshape(C, 3)[:, 1:]).all())
    _call(hip, xv, s3, 1)
    assert torch.equal(s3.payload().view(torch.int64), whole.payload().view(torch.int64))


def test_field_moments_class(hip):
    from ladcast_amd.preprocess import FieldMoments

    x, view, want = PO.case("stream")
    xv = _embed(x)
    fm = FieldMoments(3, "cuda")
    assert fm.count().tolist() == [0, 0, 0] and np.isnan(fm.mean()).all() and np.isnan(fm.std()).all()
    fm.update(xv[0]).update(xv[1:4]).update(xv[4:])  # (C, H, W), then two batches
    assert fm.count().tolist() == [w["n"] for w in want]
    assert PO.worst_ratio(fm.mean(), fm.std(), want) <= 1.0
    n = fm.count().astype(np.float64)
    assert np.allclose(fm.std(ddof=1), fm.std() * np.sqrt(n / (n - 1)), rtol=1e-14)
    # the cropped, channel-sliced view of the physical case through the class: no copy is made
    xp, pview, pwant = PO.case("physical")
    fp = FieldMoments(84, "cuda").update(_embed(xp)[pview])
    assert fp.count().tolist() == [w["n"] for w in pwant] and PO.worst_ratio(*fp.mean_std(), pwant) <= 1.0
    with pytest.raises(ValueError):
        fm.update(xv[:, :2])  # channel count
    with pytest.raises(ValueError):
        fm.update(xv.double())
    with pytest.raises(ValueError):
        fm.update(xv[..., ::2])  # last dimension not contiguous
    with pytest.raises(RuntimeError):
        fm.update(torch.zeros(1, 3, 2, 2))  # a host tensor
    with pytest.raises(RuntimeError):
        FieldMoments(3, "cpu")


def test_argument_errors_write_nothing(hip):
    x = torch.randn(2, 3, 4, 8, device="cuda")
    state = guarded(1, 9, dtype=torch.float64)
    ws = guarded(1, 64, dtype=torch.float64)
    nbytes = hip.lib.ldc_field_moments_workspace_bytes(2, 3, 4, 8)
    assert nbytes == 2 * 3 * 32
    f = hip.lib.ldc_field_moments
    X, S, Wp, st = hip._p(x), hip._p(state.t), c_void_p(ws.t.data_ptr()), hip._stream()
    ARG, ALIGN, UNSUPPORTED = -1, -2, -3
    assert f(None, 96, 32, 8, 2, 3, 4, 8, S, 0, Wp, nbytes, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, None, 0, Wp, nbytes, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 4, 8, S, 0, None, nbytes, st) == ARG
    assert f(X, 96, 32, 8, -2, 3, 4, 8, S, 0, Wp, nbytes, st) == ARG
    assert f(X, 96, 32, 8, 2, 3, 0, 8, S, 0, Wp, nbytes, st) == ARG
    assert f(X, 96, 32, 7, 2, 3, 4, 8, S, 0, Wp, nbytes, st) == ARG  # rows overlap
    assert f(X, 96, 32, 8, 2, 3, 4, 8, S, 0, Wp, nbytes - 1, st) == ARG  # short workspace
    assert f(X, 96, 32, 8, 2, 3, 4, 8, S, 0, c_void_p(ws.t.data_ptr() + 8), nbytes, st) == ALIGN
    assert f(X, 96, 32, 8, 2, 3, 4, 8, c_void_p(state.t.data_ptr() + 4), 0, Wp, nbytes, st) == ALIGN
    assert f(X, 0, 0, 1, 1 << 12, 1 << 12, 1, 1, S, 0, Wp, 1 << 40, st) == UNSUPPORTED  # 2^24 chunk records
    torch.cuda.synchronize()
    unwritten = UNWRITTEN64  # (a positive int64)
    assert bool((state.payload().view(torch.int64) == unwritten).all()) and bool((ws.payload().view(torch.int64) == unwritten).all())
    assert_untouched(state, "state")
    assert_untouched(ws, "workspace")
    with pytest.raises(RuntimeError):
        hip.field_moments(torch.zeros(1, 1, 2, 2), state.t, B=1, C=1, H=2, W=2, batch_stride=4, channel_stride=4, row_stride=2, accumulate=False)
