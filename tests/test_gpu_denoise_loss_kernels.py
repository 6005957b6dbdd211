"""The three kernels of ladcast_amd/csrc/denoise_loss.hip through `hip.py` against torch CPU evaluation of the same expressions.

`noisy`, `x_in` and `denoised` are the same IEEE operations without contraction: BIT-EQUAL.  Every `table` entry: within 1 fp32 ulp of
the float64 mean of the fp32 terms - fp64 accumulation of at most 5200 terms is exact to far below half an fp32 ulp, then one division
and one rounding.  Every input and output lies between guard bands (tests/redzone.py): a read past an input pulls a NaN into a result,
a write past an output changes a guard word.  Shapes: the smallest; planes shorter than a wave with every plane start unaligned; the
model's 450-element plane (a tail, odd planes off 16 bytes); an exact multiple of every vector / wave width; several passes per lane."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.redzone import UNWRITTEN32, _signed, assert_untouched, guarded  # noqa: E402

SHAPES = [(1, 1, 1, 1, 1), (2, 3, 2, 3, 5), (3, 4, 1, 15, 30), (2, 2, 3, 16, 64), (1, 2, 1, 40, 130)]


def index_sets(B):
    """schedule indices per sample: distinct, always with the ends 0 and 999 (one sample: each end in turn)"""
    return [[0], [999]] if B == 1 else [[0, 999, 500][:B]]


def gbuf(shape, values=None):
    """(Guarded, (B, C, T, H, W) view): an input filled with `values`, or an output whose payload starts as the UNWRITTEN NaN pattern"""
    g = guarded(1, math.prod(shape), unwritten=values is None)
    if values is not None:
        g.fill(values)
    return g, g.view[0, 0].view(*shape)


def coefficients(indices, pred="epsilon"):
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    s = EDMDPMSolverMultistepScheduler(prediction_type=pred)
    sigma = s.sigmas[indices].clone()
    return (sigma,) + s.edm_coefficients(sigma)


def inputs(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    clean, target_noise, F = (torch.randn(shape, generator=g) for _ in range(3))
    return 0.5 * clean, target_noise, F


def col(v):
    return v.reshape(-1, 1, 1, 1, 1)


def ulp32(x64):
    return torch.from_numpy(np.spacing(np.abs(x64.numpy()).astype(np.float32)).astype(np.float64))


def assert_table(got, terms32, what):
    """every entry within 1 fp32 ulp of the float64 mean of the fp32 terms over its plane"""
    want = terms32.double().mean(dim=(3, 4))
    got = got.detach().cpu().double().reshape(want.shape)
    assert torch.isfinite(got).all(), what
    excess = ((got - want).abs() / ulp32(want)).max().item()
    print(f"{what}: worst table error {excess:.3f} ulp")
    assert excess <= 1.0, (what, excess)


@pytest.mark.parametrize("shape", SHAPES)
def test_noise_inputs_bit_equal(shape):
    import ladcast_amd.hip as hip

    B = shape[0]
    clean, noise, _ = inputs(shape)
    for indices in index_sets(B):
        sigma, c_in, _, _, _ = coefficients(indices)
        want_noisy = clean + noise * col(sigma)
        want_x = want_noisy * col(c_in)
        (gc, dc), (gn, dn) = gbuf(shape, clean), gbuf(shape, noise)
        (g1, noisy), (g2, x_in) = gbuf(shape), gbuf(shape)
        hip.edm_noise_inputs(dc, dn, sigma.cuda(), c_in.cuda(), noisy, x_in)
        assert torch.equal(noisy.cpu(), want_noisy) and torch.equal(x_in.cpu(), want_x), indices
        # each output alone; without noise: precondition_inputs of an already noised tensor
        (g3, only_noisy), (g4, only_x) = gbuf(shape), gbuf(shape)
        hip.edm_noise_inputs(dc, dn, sigma.cuda(), None, only_noisy, None)
        hip.edm_noise_inputs(noisy, None, None, c_in.cuda(), None, only_x)
        assert torch.equal(only_noisy.cpu(), want_noisy) and torch.equal(only_x.cpu(), want_x)
        for g in (gc, gn, g1, g2, g3, g4):
            assert_untouched(g, f"edm_noise_inputs {shape}")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pred", ["epsilon", "v_prediction"])
def test_denoise_bit_equal_on_t_slices(shape, pred):
    import ladcast_amd.hip as hip

    B, C, T, H, W = shape
    noisy, _, F = inputs(shape, seed=1)
    for indices in index_sets(B):
        _, _, c_skip, c_out, _ = coefficients(indices, pred)
        want = col(c_skip) * noisy + col(c_out) * F
        # contiguous
        (ga, da), (gf, df), (go, out) = gbuf(shape, noisy), gbuf(shape, F), gbuf(shape)
        hip.edm_denoise(da, df, c_skip.cuda(), c_out.cuda(), out)
        assert torch.equal(out.cpu(), want), indices
        for g in (ga, gf, go):
            assert_untouched(g, f"edm_denoise {shape}")
        # T-slices of larger tensors, another number of frames and another offset for each
        big = lambda extra: (B, C, T + extra, H, W)  # noqa: E731
        pa, pf = torch.full(big(2), float("nan")), torch.full(big(1), float("nan"))
        pa[:, :, 1 : 1 + T], pf[:, :, 0:T] = noisy, F
        (ga, da), (gf, df), (go, dout) = gbuf(big(2), pa), gbuf(big(1), pf), gbuf(big(3))
        hip.edm_denoise(da[:, :, 1 : 1 + T], df[:, :, 0:T], c_skip.cuda(), c_out.cuda(), dout[:, :, 2 : 2 + T])
        host = dout.cpu()
        assert torch.equal(host[:, :, 2 : 2 + T], want), indices
        rest = torch.ones(big(3), dtype=torch.bool)
        rest[:, :, 2 : 2 + T] = False
        assert (host.view(torch.int32)[rest] == _signed(UNWRITTEN32, 32)).all(), "frames outside the slice were written"
        for g in (ga, gf, go):
            assert_untouched(g, f"edm_denoise slices {shape}")
    with pytest.raises(ValueError):
        hip.edm_denoise(da.transpose(3, 4), df[:, :, 0:T], c_skip.cuda(), c_out.cuda(), dout[:, :, 2 : 2 + T])  # not a T-slice


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lat", [False, True])
@pytest.mark.parametrize("with_denoised", [False, True])
def test_denoise_loss_table(shape, lat, with_denoised):
    import ladcast_amd.hip as hip

    B, C, T, H, W = shape
    noisy, target, F = inputs(shape, seed=2)
    lat_w = (0.25 + torch.arange(H, dtype=torch.float32) * 0.173).contiguous() if lat else None  # a distinct weight per row
    for indices in index_sets(B):
        _, _, c_skip, c_out, weight = coefficients(indices)
        den = col(c_skip) * noisy + col(c_out) * F
        q = (den - target) ** 2
        terms = (lat_w.view(1, 1, 1, H, 1) * col(weight)) * q if lat else col(weight) * q
        assert terms.dtype == torch.float32
        (ga, da), (gf, df), (gt, dt) = gbuf(shape, noisy), gbuf(shape, F), gbuf(shape, target)
        gtab = guarded(1, B * C * T)
        table = gtab.view[0, 0]
        gd, dden = gbuf(shape) if with_denoised else (None, None)
        args = (da, df, dt, c_skip.cuda(), c_out.cuda(), weight.cuda(), table)
        kw = dict(lat_weight=None if lat_w is None else lat_w.cuda(), denoised=dden)
        hip.edm_denoise_loss(*args, **kw)
        first = table.cpu().clone()
        assert_table(first, terms, f"{shape} lat={lat} indices={indices}")
        if with_denoised:
            assert torch.equal(dden.cpu(), den)
        hip.edm_denoise_loss(*args, **kw)  # a second launch: the same bits
        assert torch.equal(table.cpu().view(torch.int32), first.view(torch.int32))
        for g in (ga, gf, gt, gtab) + ((gd,) if with_denoised else ()):
            assert_untouched(g, f"edm_denoise_loss {shape}")


@pytest.mark.parametrize("shape", SHAPES[1:4])
def test_nan_stays_in_its_plane(shape):
    import ladcast_amd.hip as hip

    B, C, T, H, W = shape
    noisy, target, F = inputs(shape, seed=3)
    _, _, c_skip, c_out, weight = coefficients(index_sets(B)[0])
    co = [v.cuda() for v in (c_skip, c_out, weight)]
    clean_table, table = torch.empty(B, C, T, device="cuda"), torch.empty(B, C, T, device="cuda")
    hip.edm_denoise_loss(noisy.cuda(), F.cuda(), target.cuda(), *co, clean_table)
    b, c, t = B - 1, C // 2, T - 1
    bad = F.clone()
    bad[b, c, t, H - 1, W - 1] = float("nan")  # the last element of the plane: a tail lane's
    hip.edm_denoise_loss(noisy.cuda(), bad.cuda(), target.cuda(), *co, table)
    got, base = table.cpu(), clean_table.cpu()
    assert math.isnan(got[b, c, t]) and torch.isfinite(base).all()
    keep = torch.ones(B, C, T, dtype=torch.bool)
    keep[b, c, t] = False
    assert torch.equal(got[keep], base[keep])


def test_argument_errors():
    import ladcast_amd.hip as hip

    x = torch.zeros(2, 1, 1, 3, 5, device="cuda")
    v, tab = torch.ones(2, device="cuda"), torch.zeros(2, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    lib = hip.lib
    assert lib.ldc_edm_noise_inputs(None, p(x), p(v), p(v), p(x), p(x), 2, 15, None) == -1
    assert lib.ldc_edm_noise_inputs(p(x), p(x), None, p(v), p(x), p(x), 2, 15, None) == -1  # noise without sigma
    assert lib.ldc_edm_noise_inputs(p(x), p(x), p(v), None, p(x), p(x), 2, 15, None) == -1  # x_in without c_in
    assert lib.ldc_edm_noise_inputs(p(x), p(x), p(v), p(v), None, None, 2, 15, None) == -1  # no output
    assert lib.ldc_edm_noise_inputs(p(x), p(x), p(v), p(v), p(x), p(x), 0, 15, None) == -1
    assert lib.ldc_edm_noise_inputs(p(x), p(x), p(v), p(v), p(x), p(x), 2, 0, None) == -1
    assert lib.ldc_edm_denoise(p(x), p(x), p(v), None, p(x), 2, 1, 1, 15, 1, 1, 1, None) == -1
    assert lib.ldc_edm_denoise(p(x), p(x), p(v), p(v), p(x), 2, 1, 0, 15, 1, 1, 1, None) == -1
    assert lib.ldc_edm_denoise(p(x), p(x), p(v), p(v), p(x), 2, 1, 2, 15, 1, 2, 2, None) == -1  # a view longer than its tensor
    assert lib.ldc_edm_denoise_loss(p(x), p(x), p(x), p(v), p(v), None, None, p(tab), None, 2, 1, 1, 3, 5, None) == -1
    assert lib.ldc_edm_denoise_loss(p(x), p(x), p(x), p(v), p(v), p(v), None, None, None, 2, 1, 1, 3, 5, None) == -1
    assert lib.ldc_edm_denoise_loss(p(x), p(x), p(x), p(v), p(v), p(v), None, p(tab), None, 2, 1, 1, 0, 5, None) == -1
    with pytest.raises(ValueError):
        hip.edm_denoise_loss(x, x, x, v, v, torch.ones(3, device="cuda"), tab)  # a coefficient vector of the wrong length
    torch.cuda.synchronize()
    assert torch.count_nonzero(x) == 0 and torch.count_nonzero(tab) == 0  # nothing was launched
