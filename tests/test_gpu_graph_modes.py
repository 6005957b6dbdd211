"""Cached hipGraphs must never replay a configuration that no longer applies: (1) an arithmetic-mode switch with graphs on (AR forward,
edm chunk, DC-AE encode / decode: fp32 -> bf16x3 -> fp32, each result in its own band of tests/precision_bands.py, the two fp32 runs
bitwise equal); (2) a foreign DC-AE attention processor installed after a capture (a plain attribute: nothing tells the model)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import pipelines as OP  # noqa: E402
from oracle.scheduler import EDMDPMSolverMultistepScheduler as OracleScheduler  # noqa: E402
from tests.precision_bands import check as band_check  # noqa: E402
from tests.synth import make_ar, make_dcae, rel_l2, synth_field, synth_known, tiny_ar_config, tiny_dcae_config  # noqa: E402


def _hip_ar(o, cfg):
    from ladcast_amd.models import LaDCastTransformer3DModel

    m = LaDCastTransformer3DModel.from_config(cfg)
    m.load_state_dict(o.state_dict(), strict=True)
    return m.cuda().eval()


def _hip_ae(o, cfg):
    from ladcast_amd.models import AutoencoderDC

    g = AutoencoderDC.from_config(cfg)
    g.load_state_dict(o.state_dict(), strict=True)
    return g.cuda().eval()


def _fp32_bf16x3_fp32(model, run):
    """run() under fp32, bf16x3, fp32 with graphs enabled throughout; returns the three results"""
    outs = []
    model.enable_hip_graph(True)
    try:
        for mode in ("fp32", "bf16x3", "fp32"):
            model.set_gemm_precision(mode)
            outs.append(run().clone())
    finally:
        model.set_gemm_precision("fp32")
        model.enable_hip_graph(False)
    assert torch.equal(outs[0], outs[2])
    return outs


def test_mode_switch_with_graphs_ar_forward_and_edm_chunk():
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, ensemble_AR_sampler
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    cfg = tiny_ar_config(heads=2, layers=1, single=1, refiner=1)
    o = make_ar(cfg)
    g = _hip_ar(o, cfg)
    # the inputs of test_gpu_model.py::test_tiny_forward_matches_oracle[2-4-1] and ::test_tiny_sampler_chunk_matches_oracle[edm]
    x = torch.randn(2, 84, 4, 15, 30, generator=torch.Generator().manual_seed(3))
    known, t, ts = synth_known(2), torch.linspace(-1.2, 1.0, 1), torch.tensor([2018010100])
    with torch.no_grad():
        want = o(x, t, known, time_elapsed=ts).sample
    f32, b3, _ = _fp32_bf16x3_fp32(g, lambda: g(x.cuda(), t.cuda(), known.cuda(), time_elapsed=ts.cuda()).sample)
    band_check("tiny_forward", rel_l2(f32.cpu(), want), rel_l2(b3.cpu(), want))

    k1 = synth_known(1)
    want = OP.ensemble_AR_sampler(OP.AutoRegressive2DPipeline(o, OracleScheduler()), 3, 4, 6, known_latents=k1, timestamps=ts, sampler_type="edm")
    pipe = AutoRegressive2DPipeline(g, EDMDPMSolverMultistepScheduler())
    f32, b3, _ = _fp32_bf16x3_fp32(g, lambda: ensemble_AR_sampler(pipe, 3, 4, 6, known_latents=k1.cuda(), timestamps=ts.cuda(), sampler_type="edm",
                                                                  device="cuda"))
    band_check("tiny_chunk_edm", rel_l2(f32.cpu(), want), rel_l2(b3.cpu(), want))


def test_mode_switch_with_graphs_dcae():
    cfg = tiny_dcae_config()
    o = make_dcae(cfg)
    g = _hip_ae(o, cfg)
    f, st = synth_field(2, 8, 48, 64), synth_field(1, 5, 48, 64, seed=1)  # the inputs of test_gpu_dcae.py::test_tiny_dcae_matches_oracle_and_pin
    with torch.no_grad():
        zo = o.encode(f, static_conditioning_tensor=st.expand(2, -1, -1, -1)).latent
        yo = o.decode(zo).sample
    z32, z3, _ = _fp32_bf16x3_fp32(g, lambda: g.encode(f.cuda(), static_conditioning_tensor=st.cuda()).latent)
    band_check("tiny_dcae_encode", rel_l2(z32.cpu(), zo), rel_l2(z3.cpu(), zo))
    y32, y3, _ = _fp32_bf16x3_fp32(g, lambda: g.decode(zo.cuda()).sample)
    band_check("tiny_dcae_decode", rel_l2(y32.cpu(), yo), rel_l2(y3.cpu(), yo))


def test_foreign_processor_installed_after_capture_is_not_ignored():
    """graphs on, encode (captured), then `attn.processor = Foreign()`: the next encode must not replay the fused graph - it drops the
    cached graphs and raises what enable_hip_graph(True) raises for a foreign processor; with graphs off the processor is called"""
    from ladcast_amd.models.DCAE import SanaMultiscaleAttnProcessor2_0, SanaMultiscaleLinearAttention

    class Foreign:
        def __init__(self):
            self.calls = 0

        def __call__(self, attn, hidden_states, gate=None):
            self.calls += 1
            return hidden_states  # the attention branch dropped: only the residual passes

    cfg = tiny_dcae_config()
    g = _hip_ae(make_dcae(cfg), cfg)
    f, st = synth_field(2, 8, 48, 64).cuda(), synth_field(1, 5, 48, 64, seed=1).cuda()
    fused = g.encode(f, static_conditioning_tensor=st).latent
    attns = [m for m in g.modules() if isinstance(m, SanaMultiscaleLinearAttention)]
    g.enable_hip_graph(True)
    try:
        assert torch.equal(g.encode(f, static_conditioning_tensor=st).latent, fused) and g._graphs
        proc = Foreign()
        attns[0].processor = proc
        with pytest.raises(NotImplementedError, match="cannot be captured"):
            g.encode(f, static_conditioning_tensor=st)
        assert g._graphs == {} and proc.calls == 0
        with pytest.raises(NotImplementedError, match="cannot be captured"):
            g.decode(fused)
        g.enable_hip_graph(False)
        z = g.encode(f, static_conditioning_tensor=st).latent
        assert proc.calls == 1 and rel_l2(z, fused) > 1e-3  # the processor ran, and its arithmetic counts
    finally:
        g.enable_hip_graph(False)
        attns[0].processor = SanaMultiscaleAttnProcessor2_0()
    assert torch.equal(g.encode(f, static_conditioning_tensor=st).latent, fused)
