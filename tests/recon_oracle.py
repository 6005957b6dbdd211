"""Seeded inputs and a float64 restatement of the DC-AE reconstruction scores (a helper module, not a conftest).

The reference's own outputs for these inputs are in tests/golden/recon_ref.npz (made by tests/golden/make_recon_golden.py from
ladcast.metric.loss / ladcast.metric.utils and weather_dataset_preprocess_batch); tests/test_recon_cpu.py pins this restatement to
them.  The restatement takes every POINT value in fp32, operation by operation as the reference's torch ops do (so the
cancellation in (p sigma + mu) - (t sigma + mu) is the reference's), and every SUM in float64.
"""
import math

import torch

SST_FILL = -2.0

# (B, C_in, H_in, W) of the raw batches; each runs with crop on / off and the last channel dropped / kept; SST = channel 1
PRE_SHAPES = [(1, 3, 2, 1), (2, 5, 4, 6), (3, 4, 8, 10)]
PRE_SST = 1

# name -> (B, C, S, H, W, static batch); "stored": the inputs are in the fixture, otherwise regenerated from the seed (checksummed)
SCORE_CASES = {
    "point": dict(shape=(1, 2, 0, 1, 1, 0), seed=11, stored=True),  # single point; C = 2: the SST channel is the zero one, nothing masked
    "point_all": dict(shape=(1, 4, 1, 1, 1, 1), seed=12, stored=True),  # single point with every ingredient (masked SST, static)
    "odd": dict(shape=(1, 3, 1, 3, 3, 1), seed=13, stored=True),  # odd everything, scalar load path
    "w6": dict(shape=(3, 4, 2, 5, 6, 1), seed=14, stored=True),  # W % 4 != 0, static batch 1 broadcast
    "vec": dict(shape=(2, 4, 2, 6, 8, 2), seed=15, stored=True),  # vector load path, static batch = B
    "chunks": dict(shape=(2, 7, 5, 33, 68, 1), seed=16, stored=False),  # several row chunks per plane, ragged last chunk
    "full": dict(shape=(2, 84, 5, 120, 240, 1), seed=17, stored=False),  # the real size
}
GEO, ZERO = 0, 1  # channel with ERA5-like geopotential statistics; all-zero target channel


def pre_inputs(shape, seed):
    """raw frames (B, C_in, H_in, W) with NaN in the SST plane - every point of batch element 0 (B > 1), none of element 1, ~30 %
    otherwise (at least the last point, which no crop removes) - and per-channel mean / std for all C_in channels"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 3.0 + 1.5
    mean = torch.randn(C, generator=g) * 2.0
    std = torch.rand(C, generator=g) + 0.5
    for b in range(B):
        if B > 1 and b == 0:
            x[b, PRE_SST] = float("nan")
        elif B > 1 and b == 1:
            continue
        else:
            m = torch.rand(H, W, generator=g) < 0.3
            m[-1, -1] = True
            x[b, PRE_SST][m] = float("nan")
    return x, mean, std


def preprocess(x, mean, std, crop_south_pole, sst_channel_idx, incl_sur_pressure):
    """weather_dataset_preprocess_batch restated (fp32, the same two ops): -> (batch, nan_mask)"""
    if crop_south_pole:
        x = x[..., 1:, :]
    if not incl_sur_pressure:
        x = x[:, :-1]
    y = (x - mean.view(-1, 1, 1)) / std.view(-1, 1, 1)
    mask = torch.isnan(y[:, sst_channel_idx])
    y = y.clone()
    y[:, sst_channel_idx] = torch.where(mask, torch.full_like(y[:, sst_channel_idx], SST_FILL), y[:, sst_channel_idx])
    return y, mask


def score_inputs(name):
    """dict(pred (B, Cp, H, W), target (B, C, H, W), static (Bs, S, H, W) | None, mask (B, H, W) bool, w (H,), mean / std (Cp,), sst)"""
    B, C, S, H, W, Bs = SCORE_CASES[name]["shape"]
    g = torch.Generator().manual_seed(SCORE_CASES[name]["seed"])
    Cp = C + S
    target = torch.randn(B, C, H, W, generator=g)
    static = torch.randn(Bs, S, H, W, generator=g) if S else None
    err = 0.1 * torch.randn(B, Cp, H, W, generator=g)
    err[:, GEO] *= 0.1  # reconstruction error ~1e-2 in the geopotential-like channel
    target[:, ZERO] = 0.0
    full = target if S == 0 else torch.cat([target, static.expand(B, -1, -1, -1)], dim=1)
    pred = full + err
    pred[: B - 1, ZERO] = 0.0  # zero numerator too: NaN; the last batch element keeps its error: inf
    sst = 2 if C >= 3 else ZERO
    mask = torch.rand(B, H, W, generator=g) < 0.3
    if C < 3:
        mask[:] = False
    elif B >= 2 or H * W == 1:
        mask[0] = True  # one batch element fully masked
    mean = torch.randn(Cp, generator=g) * 10.0
    std = torch.rand(Cp, generator=g) + 0.5
    mean[GEO], std[GEO] = 199873.4, 3127.7
    w = (torch.cos(torch.deg2rad(torch.linspace(-60.0, 75.0, H, dtype=torch.float64))) * 1.3).float()
    return dict(pred=pred, target=target, static=static, mask=mask, w=w, mean=mean, std=std, sst=sst)


def checksum(d):
    return torch.stack([d["pred"].double().sum(), d["target"].double().sum(), d["pred"].double().abs().sum()])


def scores(pred, target, static, mask, sst, w, mean, std):
    """float64 (rel (B, Cp), abs (B, Cp), lw_mse (Cp,)): fp32 point values, float64 sums"""
    B, Cp, H, W = pred.shape
    t = target if static is None else torch.cat([target, static.expand(B, -1, -1, -1)], dim=1)
    p = pred.clone()
    t = t.clone()
    if mask is not None and sst >= 0:
        p[:, sst][mask] = SST_FILL
        t[:, sst][mask] = SST_FILL
    wv = w.float().view(1, 1, H, 1)
    wd, wt = wv * (p - t), wv * t
    num, den = wd.double().square().sum(dim=(2, 3)), wt.double().square().sum(dim=(2, 3))
    sd, mu = std.float().view(1, Cp, 1, 1), mean.float().view(1, Cp, 1, 1)
    e = (p * sd + mu) - (t * sd + mu)
    lw = ((e * e) * wv).double().mean(dim=(0, 2, 3))
    return num.sqrt() / den.sqrt(), num.sqrt(), lw


def close(a, b, tol, what=""):
    """the `_close` rule of tests/test_gpu_scoring.py - |a - b| <= tol (|b| + mean |b|) over the finite entries, the NaN pattern
    equal - and, for the zero-target channels, the +-inf pattern equal as well; returns the largest |a - b| / (|b| + mean |b|)"""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert bool((torch.isnan(a) == torch.isnan(b)).all()), f"{what}: NaN pattern differs"
    inf_a, inf_b = torch.isinf(a), torch.isinf(b)
    assert bool((inf_a == inf_b).all()) and bool((a[inf_a] == b[inf_b]).all()), f"{what}: inf pattern differs"
    fin = torch.isfinite(b)
    a, b = a[fin], b[fin]
    if a.numel() == 0:
        return 0.0
    ratio = (a - b).abs() / (b.abs() + b.abs().mean()).clamp_min(1e-300)
    worst = float(ratio.max())
    assert worst <= tol, (what, worst)
    return worst


def evaluate(forward, batches, mean, std, static_raw, w, sst, crop_south_pole=True, incl_sur_pressure=False):
    """evaluate_encdec_model.py:114-239 for one year, restated: `forward(x, static (B, S, H, W))` is the autoencoder's
    forward(..., return_static=True).  -> (val_loss_fn_loss, val_lw_rmse (Cp,)) in float64"""
    static = smean = sstd = None
    if static_raw is not None:
        smean, sstd = static_raw.mean((1, 2), keepdim=True), static_raw.std((1, 2), keepdim=True)
        static = ((static_raw - smean) / sstd).unsqueeze(0)
    pm = mean if static is None else torch.cat([mean, smean.flatten()])
    ps = std if static is None else torch.cat([std, sstd.flatten()])
    loss, lw_acc, n = 0.0, 0.0, 0
    for raw in batches:
        x, mask = preprocess(raw, mean, std, crop_south_pole, sst, incl_sur_pressure)
        B = x.shape[0]
        pred = forward(x, None if static is None else static.expand(B, -1, -1, -1))
        rel, _, lw = scores(pred, x, static, mask, sst, w, pm, ps)
        loss += float(rel.mean(dim=0, keepdim=True).mean(dim=1)) * B
        lw_acc = lw_acc + lw * B
        n += B
    return loss / n, torch.sqrt(lw_acc / n)


def lat_weights(H_in, crop_south_pole):
    """evaluate/utils.py get_normalized_lat_weights_based_on_cos on the cropped equiangular grid, float64 -> fp32"""
    lat = torch.linspace(-90.0, 90.0, H_in, dtype=torch.float64)
    if crop_south_pole:
        lat = lat[1:]
    wgt = torch.cos(lat * (math.pi / 180.0))
    return (wgt / wgt.mean()).float()
