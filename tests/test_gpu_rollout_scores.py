"""All lead times of a forecast in one launch (ladcast_amd.evaluate.rollout_scores, C ABI ldc_rollout_scores) against the per-lead-time
path it shares its point body with (ensemble_scores: bit for bit - same arms, same reduction order) and against the pinned oracle
(oracle/scoring.py, looped over the lead times; the project's 1e-5 with the `_close` rule of tests/test_gpu_scoring.py).  Data as in
tests/test_gpu_scoring.py: seeded members randn * 2 + 0.5, independent truth, climatology * 0.3, 30 % land NaNs in the NaN channel."""
import ctypes
import functools

import pytest
import torch

from oracle import scoring as S
from tests.redzone import assert_untouched, guarded

pytestmark = pytest.mark.gpu

KEYS = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
TOL = 1e-5

# (M, C, L, H, W, nan_channel)
CASES = [
    (1, 2, 2, 5, 4, 1),  # no sort
    (2, 1, 3, 3, 3, 0),  # plane smaller than one wave
    (5, 3, 3, 6, 8, 1),  # 48 points, a partial workgroup
    (9, 2, 2, 33, 17, -1),  # 16 arm, 561 points = 3 workgroups with the last partial, odd W
    (17, 2, 2, 6, 8, 0),  # pruned <32, 24> arm
    (50, 3, 2, 33, 17, 2),  # the workload's ensemble
    (64, 2, 2, 30, 60, -1),  # full <64, 64> arm
]
SMALL = [(5, 3, 3, 6, 8, 1), (9, 2, 2, 33, 17, -1)]


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


def _oracle(dec, ref, clim, w, sst):
    """oracle.scoring.ensemble_scores per lead time -> {key: (C, L)}"""
    per = [S.ensemble_scores(dec[:, :, l], ref[:, l], clim[:, l], w, sst_channel=max(sst, 0)) for l in range(dec.shape[2])]
    return {k: torch.stack([p[k] for p in per], dim=1) for k in KEYS}


@functools.lru_cache(maxsize=None)
def _case(M, C, L, H, W, sst):
    """host data, lat weights and the oracle's scores of one case, made once and left unchanged"""
    g = torch.Generator().manual_seed(3)
    dec = torch.randn(M, C, L, H, W, generator=g) * 2 + 0.5
    ref = torch.randn(C, L, H, W, generator=g)
    clim = torch.randn(C, L, H, W, generator=g) * 0.3
    if sst >= 0:
        land = torch.rand(H, W, generator=g) < 0.3
        dec[:, sst][:, :, land] = float("nan")
        ref[sst][:, land] = float("nan")
    w = S.get_normalized_lat_weights_based_on_cos(torch.linspace(-89.0, 89.0, H))
    return dec, ref, clim, w, _oracle(dec, ref, clim, w, sst)


@pytest.mark.parametrize("M,C,L,H,W,sst", CASES)
def test_rollout_scores_equal_the_per_lead_path_and_the_oracle(E, M, C, L, H, W, sst):
    dec, ref, clim, w, want = _case(M, C, L, H, W, sst)
    dd, dr, dc, dw = dec.cuda(), ref.cuda(), clim.cuda(), w.cuda()
    got = E.rollout_scores(dd, dr, dc, dw, sst)
    assert set(got) == set(KEYS) and all(got[k].shape == (C, L) and got[k].is_cuda for k in KEYS)
    for l in range(L):  # 1. the untouched per-lead-time kernel, bit for bit
        one = E.ensemble_scores(dd[:, :, l], dr[:, l], dc[:, l], dw, sst)
        for k in KEYS:
            assert torch.equal(torch.nan_to_num(got[k][:, l]), torch.nan_to_num(one[k])), (k, l)
            assert torch.equal(torch.isnan(got[k][:, l]), torch.isnan(one[k])), (k, l)
    for k in KEYS:  # 2. the pinned oracle
        _close(got[k], want[k], TOL)
    again = E.rollout_scores(dd, dr, dc, dw, sst)  # 3. two runs, the same bits
    for k in KEYS:
        assert _same_bits(got[k], again[k]), k


@pytest.mark.parametrize("M,C,L,H,W,sst", SMALL)
def test_fused_inverse_normalisation(E, M, C, L, H, W, sst):
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D

    dec, ref, clim, w, _ = _case(M, C, L, H, W, sst)
    g = torch.Generator().manual_seed(17)
    mean, std = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    dd, dr, dc, dw = dec.cuda(), ref.cuda(), clim.cuda(), w.cuda()
    fused = E.rollout_scores(dd, dr, dc, dw, sst, mean=mean.cuda(), std=std.cuda(), target_std=0.5)
    plain = E.rollout_scores(inverse_normalize_transform_3D(dd, mean, std, 0.5), dr, dc, dw, sst)
    for k in KEYS:
        assert _same_bits(fused[k], plain[k]), k
    phys = (dec / 0.5) * std.view(1, C, 1, 1, 1) + mean.view(1, C, 1, 1, 1)
    want = _oracle(phys, ref, clim, w, sst)
    for k in KEYS:
        _close(fused[k], want[k], TOL)
    # target_std = 1: the division is skipped, x / 1 == x
    fused1 = E.rollout_scores(dd, dr, dc, dw, sst, mean=mean.cuda(), std=std.cuda())
    plain1 = E.rollout_scores(inverse_normalize_transform_3D(dd, mean, std), dr, dc, dw, sst)
    for k in KEYS:
        assert _same_bits(fused1[k], plain1[k]), k


@pytest.mark.parametrize("M,C,L,H,W,sst", SMALL)
def test_frame_major_layout(E, M, C, L, H, W, sst):
    """the decoder's output for a batch laid out lead-major then member, viewed (L, ens, C, H, W), against its (ens, C, L, H, W) copy"""
    dec, ref, clim, w, _ = _case(M, C, L, H, W, sst)
    dd, dr, dc, dw = dec.cuda(), ref.cuda(), clim.cuda(), w.cuda()
    frames = dd.permute(2, 0, 1, 3, 4).reshape(L * M, C, H, W).contiguous()
    a = E.rollout_scores(frames.view(L, M, C, H, W), dr, dc, dw, sst, lead_dim=0)
    b = E.rollout_scores(dd, dr, dc, dw, sst)
    for k in KEYS:
        assert _same_bits(a[k], b[k]), k


@pytest.mark.parametrize("M,C,L,H,W,sst", SMALL)
def test_slot_tables(E, M, C, L, H, W, sst):
    dec, ref, clim, w, _ = _case(M, C, L, H, W, sst)
    g = torch.Generator().manual_seed(23)
    t_tab, c_tab = torch.randn(7, C, H, W, generator=g), torch.randn(4, C, H, W, generator=g) * 0.3
    if sst >= 0:
        t_tab[:, sst][:, torch.isnan(ref[sst, 0])] = float("nan")
    t_slots, c_slots = [5, 0, 5][:L], [3, 3, 1][:L]  # repeated, not monotone
    dd, dw = dec.cuda(), w.cuda()
    got = E.rollout_scores(dd, t_tab.cuda(), c_tab.cuda(), dw, sst, truth_slots=t_slots, clim_slots=c_slots)
    want = E.rollout_scores(dd, t_tab[t_slots].permute(1, 0, 2, 3).contiguous().cuda(), c_tab[c_slots].permute(1, 0, 2, 3).contiguous().cuda(), dw, sst)
    for k in KEYS:
        assert _same_bits(got[k], want[k]), k
    # a slot outside the table is refused on the host, before anything is launched
    out = torch.full((5, C, L), -7.0, device="cuda")
    for ts, cs in (([7] + t_slots[1:], c_slots), (t_slots, c_slots[:-1] + [4]), ([-1] + t_slots[1:], c_slots)):
        with pytest.raises(ValueError):
            E.rollout_scores(dd, t_tab.cuda(), c_tab.cuda(), dw, sst, truth_slots=ts, clim_slots=cs, out=out)
    assert bool((out == -7.0).all())


@pytest.mark.parametrize("M,C,L,H,W,sst", SMALL)
def test_partial_fills_write_their_columns_only(E, M, C, L, H, W, sst):
    """L - 1 lead times, then the last one, into one out of L + 2 columns at offsets 1 and L: the single call's columns, a sentinel in
    columns 0 and L + 1, and guard bands (tests/redzone.py) around out and around a workspace of exactly the stated size"""
    from ladcast_amd import hip

    dec, ref, clim, w, _ = _case(M, C, L, H, W, sst)
    dd, dr, dc, dw = dec.cuda(), ref.cuda(), clim.cuda(), w.cuda()
    whole = E.rollout_scores(dd, dr, dc, dw, sst)
    Lt = L + 2
    # through the public function
    out = torch.full((5, C, Lt), -7.0, device="cuda")
    r = E.rollout_scores(dd[:, :, : L - 1], dr[:, : L - 1], dc[:, : L - 1], dw, sst, out=out, lead_offset=1)
    r = E.rollout_scores(dd[:, :, L - 1 :], dr[:, L - 1 :], dc[:, L - 1 :], dw, sst, out=r, lead_offset=L)
    for i, k in enumerate(KEYS):
        assert r[k].data_ptr() == out[i].data_ptr()
        assert _same_bits(out[i, :, 1 : L + 1], whole[k]), k
    assert bool((out[:, :, 0] == -7.0).all()) and bool((out[:, :, L + 1] == -7.0).all())
    # through the C ABI, with guarded out and workspace
    go = guarded(5 * C, Lt)
    go.view.fill_(-7.0)
    HW = H * W
    for l0, nl in ((0, L - 1), (L - 1, 1)):
        nbytes = int(hip.lib.ldc_rollout_scores_workspace_bytes(C, nl, H, W))
        assert nbytes == nl * C * ((HW + 255) // 256) * 15 * 4
        gw = guarded(1, nbytes // 4, unwritten=False)
        slots = torch.arange(l0, l0 + nl, dtype=torch.int32, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        fc = dd[:, :, l0:]  # the forecast pointer starts at this call's first lead time; truth / clim are reached through the slots
        st = hip.lib.ldc_rollout_scores(p(fc), dd.stride(0), dd.stride(2), dd.stride(1), None, None, 1.0, p(dr), dr.stride(1), dr.stride(0), p(slots),
                                        p(dc), dc.stride(1), dc.stride(0), p(slots), p(dw), M, C, nl, H, W, sst, p(go.view), Lt, 1 + l0, p(gw.view),
                                        nbytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        # one byte less of workspace is refused
        assert hip.lib.ldc_rollout_scores(p(fc), dd.stride(0), dd.stride(2), dd.stride(1), None, None, 1.0, p(dr), dr.stride(1), dr.stride(0),
                                          p(slots), p(dc), dc.stride(1), dc.stride(0), p(slots), p(dw), M, C, nl, H, W, sst, p(go.view), Lt, 1 + l0,
                                          p(gw.view), nbytes - 1, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0
        torch.cuda.synchronize()
        assert_untouched(gw, f"workspace of leads {l0}..{l0 + nl - 1}")
    assert_untouched(go, "out")
    raw = go.view[0].reshape(5, C, Lt)
    for i, k in enumerate(KEYS):
        assert _same_bits(raw[i, :, 1 : L + 1], whole[k]), k
    assert bool((raw[:, :, 0] == -7.0).all()) and bool((raw[:, :, L + 1] == -7.0).all())


def test_refusals(E):
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    with pytest.raises(RuntimeError):  # host tensors
        E.rollout_scores(z(2, 1, 2, 4, 4), z(1, 2, 4, 4), z(1, 2, 4, 4), torch.ones(4), 0)
    with pytest.raises(RuntimeError):  # more than 64 members
        E.rollout_scores(z(65, 1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), torch.ones(4).cuda(), 0)
    out = torch.full((5, 1, 2), -7.0, device="cuda")
    with pytest.raises(RuntimeError):  # lead_offset + L > L_total
        E.rollout_scores(z(2, 1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), torch.ones(4).cuda(), 0, out=out, lead_offset=1)
    assert bool((out == -7.0).all())
    with pytest.raises(NotImplementedError):  # fp32 only, as ensemble_scores
        E.rollout_scores(z(2, 1, 2, 4, 4).double().cuda(), z(1, 2, 4, 4).cuda(), z(1, 2, 4, 4).cuda(), torch.ones(4).cuda(), 0)
