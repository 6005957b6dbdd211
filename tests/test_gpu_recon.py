"""HIP DC-AE reconstruction scoring (C ABI ldc_recon_preprocess / ldc_recon_scores, ladcast_amd.metric) against the reference's own
outputs in tests/golden/recon_ref.npz (made by tests/golden/make_recon_golden.py from ladcast.metric and
weather_dataset_preprocess_batch).

Preprocess: output and mask bit-equal.  Scores: point values are bit-equal to the reference's by construction, so a single point
(B = H = W = 1) must give lw_mse bit for bit - the reference's geopotential-channel values there are 311.03515625 and
752.7818603515625 where the shortcut sigma^2 (p - t)^2 w gives 311.1669921875 and 753.3043212890625, so a contracted or reordered
chain fails; everything else uses the `_close` rule and the 1e-5 bound of tests/test_gpu_scoring.py (fp32 sums in another order).
Measured when the fixture was made: the reference's fp32 outputs lie within 4.3e-7 (largest case, 2 x 89 x 120 x 240; 1.3e-7 and
below for the others) of a float64 summation of the same fp32 point values, on that `_close` scale - 23 times inside the bound."""
import numpy as np
import pytest
import torch

from tests import recon_oracle as RO
from tests.redzone import assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/recon_ref.npz")


@pytest.fixture(scope="module")
def hip():
    from ladcast_amd import hip
    return hip


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("i", range(len(RO.PRE_SHAPES)))
def test_preprocess_bit_equal_with_guard_bands(ref, hip, i):
    B, C_in, H_in, W = RO.PRE_SHAPES[i]
    x = torch.from_numpy(ref[f"pre{i}_x"]).cuda()
    for crop in (0, 1):
        for keep in (0, 1):
            C, H = C_in - (0 if keep else 1), H_in - crop
            mean, std = torch.from_numpy(ref[f"pre{i}_mean"])[:C].cuda(), torch.from_numpy(ref[f"pre{i}_std"])[:C].cuda()
            out = guarded(1, B * C * H * W)
            mwords = (B * H * W + 3) // 4
            mask = guarded(1, mwords, dtype=torch.int32)
            mbytes = mask.t.view(torch.uint8).reshape(-1)
            xv = x[:, :, 1:] if crop else x
            hip.recon_preprocess(xv, mean, std, out.t, mbytes, B=B, C=C, H=H, W=W, batch_stride=xv.stride(0), channel_stride=xv.stride(1),
                                 row_stride=xv.stride(2), sst_channel=RO.PRE_SST)
            torch.cuda.synchronize()
            want = torch.from_numpy(ref[f"pre{i}_c{crop}k{keep}_y"])
            assert torch.equal(_bits(out.t.reshape(B, C, H, W)), _bits(want)), (crop, keep)
            got_mask = mbytes.cpu()
            assert torch.equal(got_mask[: B * H * W].reshape(B, H, W), torch.from_numpy(ref[f"pre{i}_c{crop}k{keep}_mask"]).to(torch.uint8))
            assert_untouched(out, "preprocess out")
            assert_untouched(mask, "preprocess mask")
            if B * H * W % 4:  # bytes of the last mask word behind the (B, H, W) extent keep the UNWRITTEN pattern
                tail = mask.t.reshape(-1)[-1:].cpu().view(torch.uint8)[B * H * W % 4 :]
                assert torch.equal(tail, torch.tensor([0xBEEF & 0xFF, 0xBEEF >> 8, 0xC0, 0x7F], dtype=torch.uint8)[B * H * W % 4 :])
            # the package-level call: same bits, a bool mask
            from ladcast_amd.evaluate.evaluate_encdec_model import preprocess_batch

            y2, m2 = preprocess_batch(x, mean, std, crop_south_pole=bool(crop), sst_channel_idx=RO.PRE_SST, incl_sur_pressure=bool(keep))
            assert m2.dtype == torch.bool and torch.equal(_bits(y2), _bits(want)) and torch.equal(m2.cpu().to(torch.uint8), got_mask[: B * H * W].reshape(B, H, W))
    # sst_channel = -1: no mask, NaNs stay
    y3 = preprocess_batch(x, torch.from_numpy(ref[f"pre{i}_mean"]).cuda(), torch.from_numpy(ref[f"pre{i}_std"]).cuda(), crop_south_pole=False,
                          sst_channel_idx=None, incl_sur_pressure=True)
    assert torch.equal(torch.isnan(y3).cpu(), torch.isnan(torch.from_numpy(ref[f"pre{i}_x"])))


_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        _INPUTS[name] = RO.score_inputs(name)
    return _INPUTS[name]


@pytest.mark.parametrize("name", list(RO.SCORE_CASES))
def test_scores_against_reference_outputs(ref, hip, name):
    d = _inputs(name)
    B, C, S, H, W, Bs = RO.SCORE_CASES[name]["shape"]
    Cp = C + S
    assert torch.equal(RO.checksum(d), torch.from_numpy(ref[f"{name}_checksum"]))
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    pred, target, static, w, mean, std = (dev(d[k]) for k in ("pred", "target", "static", "w", "mean", "std"))
    mask = d["mask"].to(torch.uint8).cuda()
    rel, absn, lw = guarded(1, B * Cp), guarded(1, B * Cp), guarded(1, Cp)
    nbytes = hip.lib.ldc_recon_scores_workspace_bytes(B, Cp, H, W)
    ws = guarded(1, nbytes // 4)
    from ctypes import c_void_p

    def run(r, a, l):
        st = hip.lib.ldc_recon_scores(hip._p(pred), hip._p(target), hip._p(static), 0 if Bs <= 1 else S * H * W, hip._p(mask), hip._p(w), hip._p(mean),
                                      hip._p(std), B, C, S, H, W, d["sst"], hip._p(r.t), hip._p(a.t), hip._p(l.t), c_void_p(ws.t.data_ptr()), nbytes,
                                      hip._stream())
        assert st == 0, st
        torch.cuda.synchronize()

    run(rel, absn, lw)
    worst = {k: RO.close(g.t.reshape(s), ref[f"{name}_{k}"], 1e-5, k) for k, g, s in (("rel", rel, (B, Cp)), ("abs", absn, (B, Cp)), ("lw", lw, (Cp,)))}
    print(f"\nrecon scores {name} {RO.SCORE_CASES[name]['shape']}: distance to the reference on the _close scale: " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for g, what in ((rel, "rel"), (absn, "abs_norm"), (lw, "lw_mse"), (ws, "workspace")):
        assert_untouched(g, what)
    if B * H * W == 1:  # nothing to sum: the reference's bits
        assert torch.equal(_bits(lw.t.reshape(Cp)), _bits(torch.from_numpy(ref[f"{name}_lw"]))), (lw.t.cpu(), ref[f"{name}_lw"])
    # a second call into fresh buffers: the same bits (fixed reduction order)
    rel2, abs2, lw2 = guarded(1, B * Cp), guarded(1, B * Cp), guarded(1, Cp)
    run(rel2, abs2, lw2)
    assert torch.equal(_bits(rel.t), _bits(rel2.t)) and torch.equal(_bits(lw.t), _bits(lw2.t)) and torch.equal(_bits(absn.t), _bits(abs2.t))

    # the reference's interface on the device: LpLoss / MSELoss / process_tensor_for_loss / remove_channel
    from ladcast_amd.metric import LpLoss, MSELoss, process_tensor_for_loss, remove_channel

    w4 = w.view(1, 1, -1, 1)
    pm, tm = process_tensor_for_loss(pred, target, mask.view(torch.bool), sst_chanel_idx=d["sst"])
    if S:
        tm = torch.cat([tm, static.expand(B, -1, -1, -1)], dim=1)
    RO.close(LpLoss(d=2, p=2, reduce_dims=None).rel(pm, tm, weight=w4), ref[f"{name}_rel"], 1e-5, "LpLoss.rel")
    RO.close(LpLoss(d=2, p=2, reduce_dims=None).abs(pm, tm, weight=w4), ref[f"{name}_abs"], 1e-5, "LpLoss.abs")
    loss_fn = LpLoss(d=2, p=2, reduce_dims=[0, 1], reductions="mean")
    RO.close(loss_fn(pm, tm, weight=w4), ref[f"{name}_loss"], 1e-5, "loss")
    RO.close(loss_fn(remove_channel(pm, RO.ZERO), remove_channel(tm, RO.ZERO), weight=w4), ref[f"{name}_loss_finite"], 1e-5, "loss without the zero channel")
    if name != "full":  # MSELoss against torch on the host (the small cases)
        want = torch.nn.functional.mse_loss(pm.cpu().double(), tm.cpu().double())
        RO.close(MSELoss()(pm, tm), want, 1e-5, "MSELoss")


def test_loss_per_var_grouping(ref, hip):
    """get_loss_per_var of both losses against the same lines of the reference run on the host in float64 (7 + 5 channels as 2 variables x 3
    levels + 6 others)"""
    from ladcast_amd.metric import LpLoss, MSELoss

    d = _inputs("chunks")
    full = torch.cat([d["target"], d["static"].expand(2, -1, -1, -1)], dim=1)
    full[:, RO.ZERO] = 1.0
    p, t, w4 = d["pred"], full, d["w"].view(1, 1, -1, 1)
    diff = (w4 * (p - t)).double().flatten(2).norm(dim=-1) / (w4 * t).double().flatten(2).norm(dim=-1)
    sq = (w4 * (p - t) ** 2).double()
    want_lp = torch.stack([diff[:, 0:3].mean(), diff[:, 3:6].mean()] + [diff[:, i].mean() for i in range(6)])
    want_mse = torch.stack([sq[:, 0:3].mean(), sq[:, 3:6].mean()] + [sq[:, i].mean() for i in range(6)])
    RO.close(LpLoss(d=2, p=2).get_loss_per_var(p.cuda(), t.cuda(), 2, num_levels=3, weight=w4.cuda()), want_lp, 1e-5, "LpLoss.get_loss_per_var")
    RO.close(MSELoss().get_loss_per_var(p.cuda(), t.cuda(), 2, num_levels=3, weight=w4.cuda()), want_mse, 1e-5, "MSELoss.get_loss_per_var")


def test_refusals(hip):
    from ladcast_amd.evaluate.evaluate_encdec_model import preprocess_batch
    from ladcast_amd.metric import LpLoss, MSELoss
    from ladcast_amd.metric.utils import recon_scores

    a, b = torch.zeros(1, 2, 3, 4), torch.ones(1, 2, 3, 4)
    with pytest.raises(RuntimeError):
        recon_scores(a, b)  # host tensors
    with pytest.raises(RuntimeError):
        LpLoss(d=2, p=2)(a, b)
    with pytest.raises(RuntimeError):
        preprocess_batch(a, torch.zeros(2), torch.ones(2))
    for kw in (dict(d=1, p=2), dict(d=2, p=1), dict(d=3, p=2)):
        with pytest.raises(NotImplementedError):
            LpLoss(**kw)(a.cuda(), b.cuda())
    with pytest.raises(NotImplementedError):
        LpLoss(d=2, p=2)(a.cuda(), b.cuda(), weight=torch.ones(1, 2, 3, 1).cuda())  # a weight per channel
    with pytest.raises(NotImplementedError):
        LpLoss(d=2, p=2)(a.cuda().double(), b.cuda().double())
    with pytest.raises(NotImplementedError):
        MSELoss(reduction="none")(a.cuda(), b.cuda())
    with pytest.raises(RuntimeError):  # a workspace that is too small is refused by the library, nothing is launched
        from ctypes import c_void_p

        z = torch.zeros(64).cuda()
        st = hip.lib.ldc_recon_scores(hip._p(z), hip._p(z), None, 0, None, hip._p(z), hip._p(z), hip._p(z), 1, 2, 0, 3, 4, -1, hip._p(z), None, hip._p(z),
                                      c_void_p(z.data_ptr()), 16, hip._stream())
        hip._check(st, "ldc_recon_scores")
