"""The three scores of the validation hook in one launch (ladcast_amd.evaluate.validation_scores, C ABI ldc_validation_scores) against the
restatement of train_AR.py:281-312 (tests/validation_oracle.py, pinned to the reference's code by tests/test_validation_cpu.py) at the
project's 1e-5 with the `_close` rule of tests/test_gpu_rollout_scores.py, and against the entry point it shares its point body with
(rollout_scores without climatology: `ens_mse` and `crps` bit for bit).  Shapes and data as in tests/test_gpu_rollout_scores.py: the arms
of the sort network, seeded members randn * 2 + 0.5, independent truth."""
import ctypes
import functools

import pytest
import torch

from oracle import scoring as S
from tests import validation_oracle as VO
from tests.redzone import assert_untouched, guarded

pytestmark = pytest.mark.gpu

KEYS = ("ens_mse", "single_mse", "crps")
TOL = 1e-5

# (M, C, L, H, W)
CASES = [
    (1, 2, 2, 5, 4),  # no sort
    (2, 1, 3, 3, 3),  # plane smaller than one wave
    (5, 3, 3, 6, 8),  # 48 points, a partial workgroup
    (9, 2, 2, 33, 17),  # 16 arm, 561 points = 3 workgroups with the last partial, odd W
    (17, 2, 2, 6, 8),  # pruned <32, 24> arm
    (50, 3, 2, 33, 17),  # the workload's ensemble
    (64, 2, 2, 30, 60),  # full <64, 64> arm
]
SMALL = [(5, 3, 3, 6, 8), (9, 2, 2, 33, 17)]


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate as ev
    return ev


def _close(a, b, tol):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape
    nan_a, nan_b = torch.isnan(a), torch.isnan(b)
    assert bool((nan_a == nan_b).all()), "NaN pattern differs"
    a, b = a[~nan_a], b[~nan_b]
    if a.numel() == 0:
        return
    assert ((a - b).abs() <= tol * (b.abs() + b.abs().mean())).all(), float(((a - b).abs() / (b.abs() + b.abs().mean())).max())


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))


@functools.lru_cache(maxsize=None)
def _case(M, C, L, H, W):
    """host data, lat weights and the oracle's scores of one case, made once and left unchanged"""
    g = torch.Generator().manual_seed(3)
    dec = torch.randn(M, C, L, H, W, generator=g) * 2 + 0.5
    ref = torch.randn(C, L, H, W, generator=g)
    w = S.get_normalized_lat_weights_based_on_cos(torch.linspace(-89.0, 89.0, H))
    return dec, ref, w, VO.validation_scores(dec, ref, w)


@pytest.mark.parametrize("M,C,L,H,W", CASES)
def test_validation_scores_equal_the_oracle_and_the_shared_body(E, M, C, L, H, W):
    dec, ref, w, want = _case(M, C, L, H, W)
    dd, dr, dw = dec.cuda(), ref.cuda(), w.cuda()
    got = E.validation_scores(dd, dr, dw)
    assert tuple(got) == KEYS == E.VALIDATION_SCORE_NAMES and all(got[k].shape == (C, L) and got[k].is_cuda for k in KEYS)
    assert got._buffer.shape == (3, C, L) and got._buffer.is_contiguous() and all(got[k].data_ptr() == got._buffer[i].data_ptr() for i, k in enumerate(KEYS))
    for k in KEYS:  # 1. the oracle restatement
        _close(got[k], want[k], TOL)
        assert bool(torch.isfinite(got[k]).all())
    roll = E.rollout_scores(dd, dr, None, dw, -1)  # 2. the shared point body: the same bits
    assert _same_bits(got["ens_mse"], roll["ens_mse"]) and _same_bits(got["crps"], roll["crps"])
    if M == 1:  # 3. sum = v, v / 1 = v, the same reduction
        assert _same_bits(got["single_mse"], got["ens_mse"])
    else:
        assert bool((got["single_mse"] > got["ens_mse"]).all())
    again = E.validation_scores(dd, dr, dw)  # 4. two runs, the same bits
    for k in KEYS:
        assert _same_bits(got[k], again[k]), k


@pytest.mark.parametrize("M,C,L,H,W", SMALL)
def test_fused_inverse_normalisation(E, M, C, L, H, W):
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D

    dec, ref, w, _ = _case(M, C, L, H, W)
    g = torch.Generator().manual_seed(17)
    mean, std = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    dd, dr, dw = dec.cuda(), ref.cuda(), w.cuda()
    fused = E.validation_scores(dd, dr, dw, mean=mean.cuda(), std=std.cuda(), target_std=0.5)
    plain = E.validation_scores(inverse_normalize_transform_3D(dd, mean, std, 0.5), dr, dw)
    for k in KEYS:
        assert _same_bits(fused[k], plain[k]), k
    want = VO.validation_scores((dec / 0.5) * std.view(1, C, 1, 1, 1) + mean.view(1, C, 1, 1, 1), ref, w)
    for k in KEYS:
        _close(fused[k], want[k], TOL)
    fused1 = E.validation_scores(dd, dr, dw, mean=mean.cuda(), std=std.cuda())  # target_std = 1: the division is skipped, x / 1 == x
    plain1 = E.validation_scores(inverse_normalize_transform_3D(dd, mean, std), dr, dw)
    for k in KEYS:
        assert _same_bits(fused1[k], plain1[k]), k


@pytest.mark.parametrize("M,C,L,H,W", SMALL)
def test_frame_major_layout(E, M, C, L, H, W):
    """the decoder's output for a batch laid out lead-major then member, viewed (L, ens, C, H, W), against its (ens, C, L, H, W) copy"""
    dec, ref, w, _ = _case(M, C, L, H, W)
    dd, dr, dw = dec.cuda(), ref.cuda(), w.cuda()
    frames = dd.permute(2, 0, 1, 3, 4).reshape(L * M, C, H, W).contiguous()
    a = E.validation_scores(frames.view(L, M, C, H, W), dr, dw, lead_dim=0)
    b = E.validation_scores(dd, dr, dw)
    for k in KEYS:
        assert _same_bits(a[k], b[k]), k


@pytest.mark.parametrize("M,C,L,H,W", SMALL)
def test_slot_tables(E, M, C, L, H, W):
    dec, ref, w, _ = _case(M, C, L, H, W)
    t_tab = torch.randn(7, C, H, W, generator=torch.Generator().manual_seed(23))  # entries 1, 2, 3, 4, 6 are decoys
    t_slots = [5, 0, 5][:L]  # repeated, not monotone
    dd, dw = dec.cuda(), w.cuda()
    got = E.validation_scores(dd, t_tab.cuda(), dw, truth_slots=t_slots)
    want = E.validation_scores(dd, t_tab[t_slots].permute(1, 0, 2, 3).contiguous().cuda(), dw)
    for k in KEYS:
        assert _same_bits(got[k], want[k]), k
    _close(got["single_mse"], VO.validation_scores(dec, t_tab[t_slots].permute(1, 0, 2, 3), w)["single_mse"], TOL)
    out = torch.full((3, C, L), -7.0, device="cuda")  # a slot outside the table is refused on the host, before anything is launched
    for ts in ([7] + t_slots[1:], [-1] + t_slots[1:], t_slots[:-1]):
        with pytest.raises(ValueError):
            E.validation_scores(dd, t_tab.cuda(), dw, truth_slots=ts, out=out)
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("M,C,L,H,W", SMALL)
def test_partial_fills_write_their_columns_only(E, M, C, L, H, W):
    """L - 1 lead times, then the last one, into one out of L + 2 columns at offsets 1 and L: the single call's columns, a sentinel in
    columns 0 and L + 1, and guard bands (tests/redzone.py) around out and around a workspace of exactly the stated size"""
    from ladcast_amd import hip

    dec, ref, w, _ = _case(M, C, L, H, W)
    dd, dr, dw = dec.cuda(), ref.cuda(), w.cuda()
    whole = E.validation_scores(dd, dr, dw)
    Lt = L + 2
    out = torch.full((3, C, Lt), -7.0, device="cuda")  # through the public function
    r = E.validation_scores(dd[:, :, : L - 1], dr[:, : L - 1], dw, out=out, lead_offset=1)
    r = E.validation_scores(dd[:, :, L - 1 :], dr[:, L - 1 :], dw, out=r, lead_offset=L)
    for i, k in enumerate(KEYS):
        assert r[k].data_ptr() == out[i].data_ptr()
        assert _same_bits(out[i, :, 1 : L + 1], whole[k]), k
    assert bool((out[:, :, 0] == -7.0).all()) and bool((out[:, :, L + 1] == -7.0).all())
    fresh = E.validation_scores(dd[:, :, :1], dr[:, :1], dw, lead_offset=2)  # a fresh buffer: unwritten columns are NaN
    assert fresh["crps"].shape == (C, 3) and bool(torch.isnan(fresh._buffer[:, :, :2]).all()) and _same_bits(fresh._buffer[:, :, 2], whole._buffer[:, :, 0])
    go = guarded(3 * C, Lt)  # through the C ABI, with guarded out and workspace
    go.view.fill_(-7.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for l0, nl in ((0, L - 1), (L - 1, 1)):
        nbytes = int(hip.lib.ldc_validation_scores_workspace_bytes(C, nl, H, W))
        assert nbytes == nl * C * ((H * W + 255) // 256) * 7 * 4
        gw = guarded(1, nbytes // 4, unwritten=False)
        slots = torch.arange(l0, l0 + nl, dtype=torch.int32, device="cuda")
        args = (p(dd[:, :, l0:]), dd.stride(0), dd.stride(2), dd.stride(1), None, None, 1.0, p(dr), dr.stride(1), dr.stride(0), p(slots), p(dw), M, C, nl,
                H, W, p(go.view), Lt, 1 + l0, p(gw.view))
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert hip.lib.ldc_validation_scores(*args, nbytes - 1, stream) != 0  # one byte less of workspace is refused
        assert hip.lib.ldc_validation_scores(*args, nbytes, stream) == 0
        torch.cuda.synchronize()
        assert_untouched(gw, f"workspace of leads {l0}..{l0 + nl - 1}")
    assert_untouched(go, "out")
    raw = go.view[0].reshape(3, C, Lt)
    for i, k in enumerate(KEYS):
        assert _same_bits(raw[i, :, 1 : L + 1], whole[k]), k
    assert bool((raw[:, :, 0] == -7.0).all()) and bool((raw[:, :, L + 1] == -7.0).all())


@pytest.mark.parametrize("where", ["member", "truth"])
@pytest.mark.parametrize("M,C,L,H,W", [(5, 3, 3, 6, 8), (50, 3, 2, 33, 17)])
def test_one_nan_turns_exactly_its_channel_and_lead_nan(E, M, C, L, H, W, where):
    dec, ref, w, _ = _case(M, C, L, H, W)
    dec, ref = dec.clone(), ref.clone()
    c, l = C - 1, 1
    if where == "member":
        dec[M // 2, c, l, H - 1, W // 2] = float("nan")
    else:
        ref[c, l, 0, W - 1] = float("nan")
    got = E.validation_scores(dec.cuda(), ref.cuda(), w.cuda())
    clean = E.validation_scores(_case(M, C, L, H, W)[0].cuda(), _case(M, C, L, H, W)[1].cuda(), w.cuda())
    hit = torch.zeros(C, L, dtype=torch.bool)
    hit[c, l] = True
    for k in KEYS:
        assert torch.equal(torch.isnan(got[k]).cpu(), hit), k
        assert torch.equal(got[k].cpu()[~hit], clean[k].cpu()[~hit]), k
    want = VO.validation_scores(dec, ref, w)  # the reference's plain means do the same
    for k in KEYS:
        assert torch.equal(torch.isnan(want[k]), hit), k


def test_refusals(E):
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    ok = (z(2, 1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), torch.ones(4).cuda())
    with pytest.raises(RuntimeError):  # host tensors
        E.validation_scores(z(2, 1, 2, 4, 4), z(1, 2, 4, 4), torch.ones(4))
    with pytest.raises(RuntimeError):  # more than 64 members: LDC_ERR_UNSUPPORTED
        E.validation_scores(z(65, 1, 2, 4, 4).cuda(), ok[1], ok[2])
    out = torch.full((3, 1, 2), -7.0, device="cuda")
    with pytest.raises(RuntimeError):  # lead_offset + L > L_total
        E.validation_scores(*ok, out=out, lead_offset=1)
    with pytest.raises(NotImplementedError):  # fp32 only
        E.validation_scores(ok[0].double(), ok[1], ok[2])
    with pytest.raises(NotImplementedError):
        E.validation_scores(ok[0], ok[1].double(), ok[2])
    for bad in (dict(forecast=z(2, 1, 2, 4).cuda()), dict(truth=z(1, 3, 4, 4).cuda()), dict(lat_weight=torch.ones(5).cuda()),
                dict(out=torch.zeros(5, 1, 2, device="cuda")), dict(mean=torch.zeros(1).cuda()), dict(mean=torch.zeros(2).cuda(), std=torch.ones(2).cuda())):
        a = dict(forecast=ok[0], truth=ok[1], lat_weight=ok[2], out=out)
        a.update(bad)
        with pytest.raises(ValueError):
            E.validation_scores(a.pop("forecast"), a.pop("truth"), a.pop("lat_weight"), **a)
    with pytest.raises(ValueError):  # slots outside the table
        E.validation_scores(ok[0], z(3, 1, 4, 4).cuda(), ok[2], truth_slots=[0, 3], out=out)
    assert bool((out == -7.0).all())
