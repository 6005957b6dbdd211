"""The exact-fp32 mode feeds its matrix kernels the model's own fp32 numbers: the AR plan's fused weights are the parameters bit for bit, and
the DC-AE's first conv reads the frame and the static fields unrounded with the parameter's own packed weight.  A weight or an input
rounded to 16 significant bits (hi + lo of a bf16 split) moves an end-to-end result by less than the fp32 band of tests/precision_bands.py
when it touches one layer only; here it is caught where it happens."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.synth import make_ar, make_dcae, synth_field, synth_known, tiny_ar_config, tiny_dcae_config  # noqa: E402


def test_fp32_plan_weights_are_the_parameters_bit_for_bit():
    from ladcast_amd.models import LaDCastTransformer3DModel
    from ladcast_amd.models.LaDCast_3D_model import _AttentionP

    cfg = tiny_ar_config(heads=2, layers=1, single=1, refiner=1)
    m = LaDCastTransformer3DModel.from_config(cfg)
    m.load_state_dict(make_ar(cfg).state_dict(), strict=True)
    m = m.cuda().eval()
    m.set_gemm_precision("fp32")
    m(torch.randn(1, 84, 4, 15, 30).cuda(), torch.tensor([0.3]).cuda(), synth_known(1).cuda(), time_elapsed=torch.tensor([2018010100]).cuda())
    p = m._plan
    assert not p.split and p.packed == {}
    n = 0
    for mod in m.modules():
        if isinstance(mod, _AttentionP):
            e = p.attn[id(mod)]
            assert torch.equal(e.wqkv, torch.cat([mod.to_q.weight, mod.to_k.weight, mod.to_v.weight]))
            assert torch.equal(e.bqkv, torch.cat([mod.to_q.bias, mod.to_k.bias, mod.to_v.bias]))
            if mod.add_q_proj is not None:
                assert torch.equal(e.wqkv_c, torch.cat([mod.add_q_proj.weight, mod.add_k_proj.weight, mod.add_v_proj.weight]))
            n += 1
    assert n == len(p.attn) == 3
    assert torch.equal(p.wx, m.x_embedder.proj.weight.reshape(p.wx.shape[0], -1))
    assert torch.equal(p.wc, m.context_embedder.proj.weight.reshape(p.wc.shape[0], -1))


def test_fp32_dcae_first_conv_reads_the_frame_unrounded(monkeypatch):
    import ladcast_amd.hip as hip
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.models.sphere_conv import pack_dense_weight_f32ring

    cfg = tiny_dcae_config()
    g = AutoencoderDC.from_config(cfg)
    g.load_state_dict(make_dcae(cfg).state_dict(), strict=True)
    g = g.cuda().eval()
    f, st = synth_field(2, 8, 48, 64), synth_field(1, 5, 48, 64, seed=1)
    g.encode(f.cuda(), static_conditioning_tensor=st.cuda())  # plan and packed weights made outside the recorded call
    calls = []
    real = hip.sphere_conv_nhwc_split

    def record(X, Wp, Y, **kw):
        calls.append((X.clone(), Wp.clone(), kw))
        return real(X, Wp, Y, **kw)

    monkeypatch.setattr(hip, "sphere_conv_nhwc_split", record)
    g.encode(f.cuda(), static_conditioning_tensor=st.cuda())
    monkeypatch.undo()
    assert calls and all(kw["in_fmt"] == hip.FMT_F32 for _, _, kw in calls)
    X, Wp, kw = calls[0]
    rows = torch.cat([f, st.expand(2, -1, -1, -1)], dim=1).permute(0, 2, 3, 1).reshape(2 * 48 * 64, 13)
    assert kw["cin"] == 16 and torch.equal(X[:, :13].cpu(), rows)  # the frame and the static fields as they are
    assert torch.equal(Wp, pack_dense_weight_f32ring(g.encoder.conv_in.weight))
