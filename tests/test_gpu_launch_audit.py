"""Launch audit per arithmetic mode: the kernels one eager forward of the tiny AR model, one encode + one decode of the tiny DC-AE and
one sampler step actually launch, classified by family and template arguments (tests/launch_audit.py).  An error band cannot tell
"fp32 everywhere" from "fp32 almost everywhere" when the split-bf16 mode is only a few times less accurate: the launch list can."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.launch_audit import classify, kernels_launched, violations  # noqa: E402
from tests.synth import make_ar, make_dcae, synth_field, synth_known, tiny_ar_config, tiny_dcae_config  # noqa: E402


def test_profiler_sees_the_library_launches():
    """positive control: a direct ctypes launch of the exact-fp32 ring GEMM shows up, classified as such (an empty trace never passes)"""
    import ladcast_amd.hip as hip

    A, W = torch.randn(256, 256, device="cuda"), torch.randn(256, 256, device="cuda")
    C = torch.empty(256, 256, device="cuda")
    names = kernels_launched(lambda: hip.gemm_sk(A, W, C, M=256, N=256, K=256))
    ks = [classify(n) for n in names]
    assert any(k.family == "gemm_bf16x3_v3_kernel" and k.args[:2] == ("128", "0") for k in ks), names


def test_each_mode_launches_only_its_own_arithmetic():
    from ladcast_amd.models import AutoencoderDC, LaDCastTransformer3DModel
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, ensemble_AR_sampler
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    cfg = tiny_ar_config(heads=2, layers=1, single=1, refiner=1)
    ar = LaDCastTransformer3DModel.from_config(cfg)
    ar.load_state_dict(make_ar(cfg).state_dict(), strict=True)
    ar = ar.cuda().eval()
    dcfg = tiny_dcae_config()
    ae = AutoencoderDC.from_config(dcfg)
    ae.load_state_dict(make_dcae(dcfg).state_dict(), strict=True)
    ae = ae.cuda().eval()
    x = torch.randn(2, 84, 4, 15, 30, generator=torch.Generator().manual_seed(3)).cuda()
    known, ts = synth_known(1).cuda(), torch.tensor([2018010100]).cuda()
    f, st = synth_field(1, 8, 48, 64).cuda(), synth_field(1, 5, 48, 64, seed=1).cuda()
    pipe = AutoRegressive2DPipeline(ar, EDMDPMSolverMultistepScheduler())
    seen = {}
    for mode in ("fp32", "bf16x3", "bf16"):
        ar.set_gemm_precision(mode)
        ae.set_gemm_precision(mode)
        bodies = {
            "ar_forward": lambda: ar(x, torch.tensor([0.3]).cuda(), known, time_elapsed=ts),
            "dcae_encode": lambda: ae.encode(f, static_conditioning_tensor=st),
            "dcae_decode": lambda: ae.decode(torch.randn(1, 8, 6, 8, device="cuda")),
            "sampler_step": lambda: ensemble_AR_sampler(pipe, 1, 4, 1, known_latents=known, timestamps=ts, sampler_type="edm", device="cuda"),
        }
        for what, body in bodies.items():
            body()  # plans, packed weights and workspaces are made outside the recorded window
            names = kernels_launched(body)
            ks = [classify(n) for n in names]  # a name outside the table fails here
            assert any(k.family not in ("torch", "copy") for k in ks), (mode, what, names)
            bad = violations(mode, names)
            assert not bad, (mode, what, sorted(set(bad)))
            seen[mode, what] = ks
    ar.set_gemm_precision("fp32")
    ae.set_gemm_precision("fp32")
    # ... and each mode's own arithmetic is really there
    for what in ("ar_forward", "dcae_encode", "dcae_decode"):
        assert any(k.family == "gemm_bf16x3_v3_kernel" and k.terms == 0 for k in seen["fp32", what]), what
        assert any(k.terms == 3 for k in seen["bf16x3", what]), what
        assert any(k.terms == 1 for k in seen["bf16", what]), what
    fams = sorted({(k.family, k.args) for v in seen.values() for k in v})
    print("\nlaunch audit, kernels seen: " + "; ".join(f"{f}<{', '.join(a)}>" if a else f for f, a in fams))
