"""CPU-side checks of the product package: the C-ABI library loads and exports every symbol that
include/ladcast_hip.h declares (no compute calls without a GPU), host-side schedule arithmetic is
bit-identical to the oracle's, argument/error conventions of the reference are kept."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import ladcast_amd.hip as hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    declared = set(re.findall(r"\b(ldc_[a-z0-9_]+)\s*\(", header))
    declared -= {"ldc_act"}
    assert len(declared) >= 30
    for name in sorted(declared):
        assert hasattr(hip.lib, name), f"{name} declared in the header but not exported"
    assert declared == set(hip.SIGNATURES), "binding and header disagree"
    # the shipped library carries no A/B arm (round 1's fp32-activation kernel and its conv entry point left the tree in round 6),
    # and no kernel source of the shipped build reads the environment
    assert not hasattr(hip.lib, "ldc_sphere_conv_nhwc_bf16x3")
    import glob

    for f in glob.glob(os.path.join(ROOT, "ladcast_amd", "csrc", "*.hip")):
        src = open(f).read()
        src = re.sub(r"#ifdef LDC_AB_BUILD.*?#endif", "", src, flags=re.S)
        assert "getenv(" not in src.replace("LDC_AB_GETENV(", ""), f
    abi = int(re.search(r"#define LDC_ABI_VERSION (\d+)", header).group(1))
    assert hip.lib.ldc_abi_version() == abi == hip.ABI_VERSION == 5 and hip.lib.ldc_build_arch() == b"gfx950"


def test_kernels_refuse_host_tensors():
    import ladcast_amd.hip as hip

    a = torch.zeros(8, 8)
    with pytest.raises(RuntimeError):
        hip.gemm(a, a, a, M=8, N=8, K=8)
    with pytest.raises(RuntimeError):
        hip.scale_f32(a, 2.0, a)


def test_scheduler_host_side_matches_oracle_bit_for_bit():
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler
    from oracle.scheduler import EDMDPMSolverMultistepScheduler as O

    for n in (1, 2, 18, 20, 50):
        a, b = EDMDPMSolverMultistepScheduler(), O()
        a.set_timesteps(n)
        b.set_timesteps(n)
        assert torch.equal(a.sigmas, b.sigmas) and torch.equal(a.timesteps, b.timesteps)
        assert a.init_noise_sigma == b.init_noise_sigma
        for s in b.sigmas[:-1]:
            assert torch.equal(a._c_in(s), 1 / ((s**2 + 0.25) ** 0.5))
            cs, co = a._c_skip_out(s)
            assert torch.equal(cs, 0.25 / (s**2 + 0.25)) and torch.equal(co, s * 0.5 / (s**2 + 0.25) ** 0.5)
        for i, t in enumerate(b.timesteps):
            assert a.index_for_timestep(t) == b.index_for_timestep(t) == i
    with pytest.raises(ValueError):
        EDMDPMSolverMultistepScheduler().step(None, None, None)  # set_timesteps not run


def test_model_surface_and_errors():
    from ladcast_amd.models import AutoencoderDC, LaDCastTransformer3DModel
    from oracle.ar_model import CONFIG_375M
    from oracle.ar_model import LaDCastTransformer3DModel as O
    from oracle.dcae import CONFIG_DCAE_84
    from oracle.dcae import AutoencoderDC as OA

    with torch.device("meta"):
        m, o = LaDCastTransformer3DModel.from_config(CONFIG_375M), O.from_config(CONFIG_375M)
        a, oa = AutoencoderDC.from_config(CONFIG_DCAE_84), OA.from_config(CONFIG_DCAE_84)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in o.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in oa.state_dict().items()}
    assert m.config.out_channels == 84 and m.config.num_attention_heads == 12 and a.config.latent_channels == 84
    assert len(m.attn_processors) == 7  # 1 refiner + 2 dual + 4 single attention layers
    with pytest.raises(ValueError):
        m.set_attn_processor({"x": None})
    tiny = LaDCastTransformer3DModel.from_config(dict(CONFIG_375M, num_attention_heads=1, num_layers=1, num_single_layers=1))
    with pytest.raises(RuntimeError):  # CPU weights: no fallback
        tiny(torch.zeros(1, 84, 1, 15, 30), torch.zeros(1), torch.zeros(1, 84, 1, 15, 30))


def test_sampler_argument_errors_follow_the_reference():
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, edm_AR_sampler, roll_out_serial
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    class Net:
        config = type("c", (), dict(out_channels=84))
        dtype = torch.float32
        device = torch.device("cpu")

    s = EDMDPMSolverMultistepScheduler()
    with pytest.raises(ValueError):
        edm_AR_sampler(Net(), s, batch_size=2, generator=[torch.Generator()], known_latents=torch.zeros(1, 84, 1, 15, 30))
    with pytest.raises(AssertionError):
        edm_AR_sampler(Net(), s, batch_size=1, known_latents=None)
    pipe = AutoRegressive2DPipeline(Net(), s)
    with pytest.raises(ValueError):
        pipe(batch_size=2, generator=[torch.Generator()], known_latents=torch.zeros(1, 84, 1, 15, 30))
    with pytest.raises(AssertionError):
        pipe(batch_size=1, known_latents=None)
    with pytest.raises(ValueError):
        roll_out_serial(None, [], pipe, total_lead_time_hour=7, step_size_hour=6)
    with pytest.raises(ValueError):
        roll_out_serial(None, [], pipe, return_ensemble_mean=True, return_latent=True)


def test_year_embedding_and_rope_tables_match_oracle():
    from ladcast_amd.models.embeddings import get_year_sincos_embedding, rope_tables_from_grid
    from oracle.ar_model import get_year_sincos_embedding as o_year
    from oracle.ar_model import rope_from_grid

    stamps = [2018010100, 2020022912, 1999123118]
    assert torch.equal(get_year_sincos_embedding(stamps, 256), o_year(torch.tensor(stamps), 256))
    grids = [torch.arange(1, 5).float(), torch.linspace(-8.7, 8.9, 15), torch.linspace(0.09, 6.17, 30)]
    a, b = rope_tables_from_grid((16, 56, 56), grids, 256.0), rope_from_grid((16, 56, 56), grids, 256.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (1800, 128)


def test_latent_npy_conventions(tmp_path):
    """file names, shapes and reader rules of the reference (evaluate/pred_rollout.py:421-430,
    evaluate/evaluate_ens_gpu.py:208-283, pipelines/utils.py:129-137); host-side, no device needed"""
    import datetime as dt

    import numpy as np

    from ladcast_amd.pipelines.io import latent_file_name, list_latent_files, load_latent_npy, save_latent_npy

    res = torch.arange(2 * 3 * 4 * 5 * 2 * 2, dtype=torch.float32).reshape(2, 3, 4, 5, 2, 2)
    stamps = [dt.datetime(2018, 1, 1, 0), np.datetime64("2018-01-03T12")]
    paths = save_latent_npy(res, stamps, str(tmp_path))
    assert [p.split("/")[-1] for p in paths] == ["latent_2018010100.npy", "latent_2018010312.npy"]
    assert latent_file_name(2018123118) == "latent_2018123118.npy"
    raw = np.load(paths[1])  # what the reference's np.load sees
    assert raw.shape == (3, 4, 5, 2, 2) and raw.dtype == np.float32 and np.array_equal(raw, res[1].numpy())
    t, ts = load_latent_npy(paths[0], crop_init=True, force_ens_size=2)
    assert ts == 2018010100 and torch.equal(t, res[0][:2, :, 1:])
    np.save(str(tmp_path / "latent_2018010500.npy"), res[:1].numpy())  # 6-D file: first entry is used
    t6, _ = load_latent_npy(str(tmp_path / "latent_2018010500.npy"))
    assert torch.equal(t6, res[0])
    listed = list_latent_files(str(tmp_path), end_date="2018-01-06T00:00:00", total_lead_time_hour=48)
    assert [s for s, _ in listed] == ["2018010100", "2018010312"]  # 2018-01-05 + 48 h is past the end date
    assert [s for s, _ in list_latent_files(str(tmp_path))] == ["2018010100", "2018010312", "2018010500"]
    with pytest.raises(ValueError):
        save_latent_npy(res[0], stamps, str(tmp_path))


def test_driver_input_preparation_follows_the_reference():
    """static fields: south-pole row dropped, land-sea mask first, per-channel z-score with the UNBIASED std (evaluate/pred_rollout.py:246-291);
    SST NaNs -> -2 in place (dataloader/utils.py:396-400); latent statistics get target_std 0.5 (pred_rollout.py:221-226)"""
    from ladcast_amd.evaluate.pred_rollout import build_static_conditioning, crop_south_pole, fill_sst_nan, load_latent_transform_args, run_rollout

    g = torch.Generator().manual_seed(4)
    lsm, oro = torch.rand(121, 240, generator=g), torch.randn(4, 121, 240, generator=g) * 30 + 7
    st = build_static_conditioning(lsm, oro)
    raw = torch.cat([lsm[1:].unsqueeze(0), oro[:, 1:]], dim=0)  # the reference's statements, spelled out
    want = (raw - raw.mean(dim=(1, 2), keepdim=True)) / raw.std(dim=(1, 2), keepdim=True)
    assert st.shape == (5, 120, 240) and torch.equal(st, want)
    assert abs(st[0].std().item() - 1) < 1e-6 and abs(st[0].std(unbiased=False).item() - 1) > 1e-6
    assert torch.equal(build_static_conditioning(None, oro), want_only := (raw[1:] - raw[1:].mean(dim=(1, 2), keepdim=True)) / raw[1:].std(dim=(1, 2), keepdim=True)) and want_only.shape[0] == 4
    assert build_static_conditioning() is None and crop_south_pole(lsm).shape == (120, 240)
    f = torch.randn(84, 2, 6, 8, generator=g)
    f[82, 1, 2, 3] = float("nan")
    f[5, 0, 0, 0] = float("nan")
    out = fill_sst_nan(f)
    assert out is f and f[82, 1, 2, 3] == -2 and torch.isnan(f[5, 0, 0, 0])  # only the SST channel is filled
    args = load_latent_transform_args({"mean": [0.0], "std": [1.0]})
    assert args == {"mean": [0.0], "std": [1.0], "target_std": 0.5}
    with pytest.raises(ValueError):
        run_rollout(None, [], None, None, args, total_lead_time_hour=7, step_size_hour=6)


def test_pipeline_loop_takes_a_duck_typed_ddim_scheduler():
    """north star: "the DDIM/DDPM scheduler loop ... diffusers-style scheduler surface" (pipelines/pipeline_AR.py:19-21,85-102): the
    loop is duck-typed.  A DDIM-shaped scheduler exposing only set_timesteps / timesteps / scale_model_input / step drives the
    PRODUCT's pipeline class (host loop; elementwise toy network on the CPU) and the oracle's: identical call sequence, identical
    bits.  (tests/test_gpu_model.py runs the same scheduler through the HIP model.)"""
    from ladcast_amd.pipelines import AutoRegressive2DPipeline
    from oracle.pipelines import AutoRegressive2DPipeline as OraclePipeline
    from tests.synth import ToyNet
    from tests.synth import DuckDDIMScheduler, synth_known

    known, ts = synth_known(2), torch.tensor([2018010106])
    outs, calls = [], []
    for cls in (AutoRegressive2DPipeline, OraclePipeline):
        sch = DuckDDIMScheduler()
        pipe = cls(ToyNet(84), sch)
        gen = [torch.Generator().manual_seed(k) for k in range(2)]
        outs.append(pipe(batch_size=2, return_seq_len=4, known_latents=known, timestamps=ts, generator=gen, num_inference_steps=7, return_dict=False)[0])
        calls.append(sch.calls)
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    assert calls[0] == calls[1] and len(calls[0]) == 14 and calls[0][0] == ("scale", 852) and calls[0][-1] == ("step", 0)
    # the dict form of the output object
    pipe = AutoRegressive2DPipeline(ToyNet(84), DuckDDIMScheduler())
    out = pipe(batch_size=1, return_seq_len=2, known_latents=synth_known(1), timestamps=ts, generator=torch.Generator().manual_seed(0), num_inference_steps=3)
    assert out.fields.shape == (1, 84, 2, 15, 30)


def test_attention_processor_surface_is_honest():
    """models/LaDCast_3D_model.py:763-827: the default processors are `LaDCastAttnProcessor2_0` markers of the fused path; a foreign
    processor is registered (and will be CALLED by the forward - tests/test_gpu_model.py), it switches hipGraph capture off / refuses
    it; the attention containers follow diffusers' attribute conventions (absent projections are None); the DCAE refuses a foreign
    linear-attention processor instead of ignoring it."""
    from ladcast_amd.models import AutoencoderDC, LaDCastAttnProcessor2_0, LaDCastTransformer3DModel, SanaMultiscaleAttnProcessor2_0
    from tests.synth import tiny_ar_config, tiny_dcae_config

    m = LaDCastTransformer3DModel.from_config(tiny_ar_config(heads=2, layers=1, single=1, refiner=1))
    procs = m.attn_processors
    assert sorted(procs) == ["context_refiner.token_refiner.refiner_blocks.0.attn.processor", "single_transformer_blocks.0.attn.processor",
                             "transformer_blocks.0.attn.processor"]
    assert all(isinstance(p, LaDCastAttnProcessor2_0) for p in procs.values()) and not m._foreign_processors()
    single, dual = m.single_transformer_blocks[0].attn, m.transformer_blocks[0].attn
    assert single.add_q_proj is None and single.to_out is None and single.to_add_out is None and single.norm_added_q is None
    assert dual.add_q_proj is not None and dual.to_out is not None and dual.to_add_out is not None
    x = torch.randn(2, 3, 5, 128)
    want = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-7)
    assert torch.allclose(dual.norm_q(x), want)  # callable for foreign processors

    class Foreign:
        def __call__(self, attn, hidden_states, encoder_hidden_states=None):
            return hidden_states, encoder_hidden_states

    with pytest.raises(ValueError):
        m.set_attn_processor({"x": Foreign()})
    m.enable_hip_graph(True)
    m.set_attn_processor(Foreign())
    assert len(m._foreign_processors()) == 3 and not m.use_hip_graph
    with pytest.raises(NotImplementedError):
        m.enable_hip_graph(True)
    m.set_attn_processor({k: (Foreign() if "single" in k else LaDCastAttnProcessor2_0()) for k in procs})
    assert len(m._foreign_processors()) == 1
    m.set_attn_processor(LaDCastAttnProcessor2_0())
    assert not m._foreign_processors()
    m.enable_hip_graph(True)
    with pytest.raises(RuntimeError):
        LaDCastAttnProcessor2_0()(None, None)  # the fused processor is a marker, never called

    ae = AutoencoderDC.from_config(tiny_dcae_config())
    attn = next(mod for mod in ae.modules() if hasattr(mod, "to_qkv_multiscale"))
    assert isinstance(attn.processor, SanaMultiscaleAttnProcessor2_0) and attn.foreign_processor is None
    # round 6 (models/DCAE.py:156,205-210): the DC-AE's plug-point is honoured like the transformer's - a foreign processor is kept and CALLED
    # (tests/test_gpu_dcae.py), and the graph mode refuses it; what such a processor reads from the module exists
    attn.processor = Foreign()
    assert attn.foreign_processor is attn.processor
    assert attn.norm_type == "rms_norm" and attn.residual_connection and callable(attn.apply_linear_attention) and callable(attn.nonlinearity)
    with pytest.raises(NotImplementedError):
        ae.enable_hip_graph(True)
    attn.processor = SanaMultiscaleAttnProcessor2_0()
    assert attn.foreign_processor is None
    ae.enable_hip_graph(True)
    # torch arithmetic of the helpers a foreign processor calls (CPU tensors): linear attention == quadratic attention on the same q, k, v
    q, k, v = (torch.rand(1, 2, 32, 40, generator=torch.Generator().manual_seed(i)) for i in range(3))
    lin = attn.apply_linear_attention(q, k, v)
    scores = torch.matmul(k.transpose(-1, -2), q)
    quad = torch.matmul(v, scores) / (scores.sum(dim=2, keepdim=True) + attn.eps)
    assert torch.allclose(lin, quad, rtol=1e-4, atol=1e-5)


def test_gemv_first_read_guard_is_in_the_shipped_kernels():
    """the AdaLN GEMV reads x.y / x.w once before their use (csrc/rowops.hip ls_first_read) - without it the kernel loses
    products when it shares a SIMD with an MFMA-streaming wave (measured: profiles/r04_z_gpu_sharing_first_read.log).  The guard may only be
    compiled out in the A/B build; the 8-rank GPU test is what checks its effect."""
    src = open(os.path.join(ROOT, "ladcast_amd", "csrc", "rowops.hip")).read()
    assert "ls_first_read(xv);" in src
    assert "#if !(defined(LDC_AB_BUILD) && defined(LDC_LS_NO_FIRST_READ))" in src
    mk = open(os.path.join(ROOT, "ladcast_amd", "csrc", "Makefile")).read()
    # the only place the Makefile names the switch is the UNGUARDED build of the reproducer (a test program, `make repro`), never a library object
    uses = [ln for ln in mk.splitlines() if "LDC_LS_NO_FIRST_READ" in ln and not ln.lstrip().startswith("#")]
    assert len(uses) == 1 and "first_read_repro" not in uses[0] and "$(REPRO_F)" in uses[0] and "$@" in uses[0]
    assert "first_read_repro_unguarded:" in mk


def test_bare_make_builds_the_library():
    """`__graft_entry__.build()` runs `make -C ladcast_amd/csrc` with no target: the FIRST rule of the Makefile must lead to the shared
    library (an earlier revision had put the reproducer's rule first - a bare make then left a stale libladcast_hip.so in place)."""
    import re
    import subprocess

    mk = open(os.path.join(ROOT, "ladcast_amd", "csrc", "Makefile")).read()
    first = next(ln for ln in mk.splitlines() if re.match(r"^[A-Za-z_$(][^=\t]*:(?!=)", ln))
    assert first.startswith("default: all"), first
    plan = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "ladcast_amd", "csrc")], capture_output=True, text=True, check=True).stdout
    assert "-o ../libladcast_hip.so" in plan and "attn_f32.hip" in plan and "conv_halo.hip" in plan


def test_bench_plain_run_defaults_and_output_dump(tmp_path, monkeypatch):
    """bench.py: a plain run skips every secondary leg unless --full (an explicit value still holds); --dump-outputs writes float32
    .npy files, and an array above the 64 MB budget becomes a seeded sample that is the same on every call"""
    import numpy as np

    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.cpu_forwards == 0 and a.sustained_seconds == 0 and a.steps == 3 and a.dump_outputs is None
    a = bench.parse_args(["--full"])
    assert a.full and a.cpu_forwards == 5 and a.sustained_seconds == 10.0
    a = bench.parse_args(["--full", "--cpu-forwards", "0", "--sustained-seconds", "0"])
    assert a.cpu_forwards == 0 and a.sustained_seconds == 0
    x = torch.randn(2, 3, 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), "latents", x)
    y = np.load(tmp_path / "d" / "latents.npy")
    assert y.dtype == np.float64 and np.array_equal(y, x.numpy())
    bench.dump_outputs(str(tmp_path / "d"), "half", x.half())
    assert np.load(tmp_path / "d" / "half.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", (1 << 20) + 4096)
    big = torch.arange(1 << 20, dtype=torch.float32)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), "fields", big)
        assert sorted(os.listdir(tmp_path / d)) == ["fields_sample.npy"]
    s1, s2 = np.load(tmp_path / "s1" / "fields_sample.npy"), np.load(tmp_path / "s2" / "fields_sample.npy")
    assert s1.dtype == np.float32 and s1.size == 1024 and np.array_equal(s1, s2) and (np.diff(s1) >= 0).all()


def test_dcae_graph_cache_refuses_a_processor_installed_after_capture():
    """a foreign DC-AE attention processor assigned while hipGraph mode is on (after a capture: a plain attribute, nothing tells the model) -
    the next graphed call drops every cached graph and raises what enable_hip_graph(True) raises, before it captures or replays anything"""
    from ladcast_amd.models import AutoencoderDC, SanaMultiscaleAttnProcessor2_0
    from ladcast_amd.models.DCAE import SanaMultiscaleLinearAttention
    from tests.synth import tiny_dcae_config

    g = AutoencoderDC.from_config(tiny_dcae_config())
    g.enable_hip_graph(True)
    g._graphs = {("enc", 1): "a captured graph"}
    attn = next(m for m in g.modules() if isinstance(m, SanaMultiscaleLinearAttention))
    attn.processor = lambda attn, hidden_states, gate=None: hidden_states
    ran = []
    with pytest.raises(NotImplementedError, match="cannot be captured"):
        g._graphed(("enc", 1), lambda *a: ran.append(a), [])
    assert g._graphs == {} and not ran
    with pytest.raises(NotImplementedError, match="cannot be captured"):
        g.enable_hip_graph(True)
    attn.processor = SanaMultiscaleAttnProcessor2_0()
    g.enable_hip_graph(False)
