"""`python bench.py --gpus N` launches its own ranks: the parent touches no GPU API, starts N fresh processes through
`python -m torch.distributed.run` as a child and exits with its code.  Dry run of the N = 2 path on the one GPU of the test box: gloo backend,
both ranks mapped onto GPU 0 (`--share-gpus`); on an 8-GPU node the driver's `python bench.py --gpus 8` takes the same path with RCCL."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launches_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpus", "--steps", "2", "--warmup", "1",
           "--cpu-forwards", "0", "--sustained-seconds", "0", "--no-kernel-timers", "--no-strong-cfg3", "--precision", "bf16x3"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 prints the one JSON line
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks"]["world_size"] == 2 and line["ranks"]["backend"] == "gloo"
    assert line["strong_cfg3"] is None  # (--no-strong-cfg3; the leg itself is asserted in the two tests below)
    # the line explains itself: the GPU's clock / power during the timed region, every rank's device
    assert [d["rank"] for d in line["ranks"]["devices"]] == [0, 1] and all(d["pci_bus_id"] for d in line["ranks"]["devices"])
    assert line["gpu"]["during_timed_region"]["samples"] >= 1 and "before" in line["gpu"] and "after" in line["gpu"]
    assert line["scaling"] == "weak" and line["steps"] == 2 and line["value"] > 0
    assert line["config"]["members_per_gpu"] == 1  # weak scaling: 2 members in all, one per rank


def test_bench_strong_scaling_fixed_ensemble_over_two_ranks():
    """`--ensemble-size E` (north star: ">= 6x at 8 GPUs vs 1" is quoted on a FIXED ensemble, BASELINE configs[2]): 3 members dealt to 2
    ranks (2 + 1), and a 1-member ensemble on 2 ranks (rank 1 owns nothing: launches nothing, joins the gather)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for E, want in ((3, [2, 1]), (1, [1, 0])):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpus", "--steps", "1", "--warmup", "0",
               "--cpu-forwards", "0", "--sustained-seconds", "0", "--no-kernel-timers", "--ensemble-size", str(E), "--solver-steps", "4", "--precision", "bf16x3",
               "--full"]  # (strong_cfg3 is a secondary leg: --full)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["scaling"] == "strong" and line["n_gpus"] == 2 and line["value"] > 0
        # north_star's strong-scaling point rides on every N > 1 line: 16 members x 40 lead steps dealt to the ranks
        s3 = line["strong_cfg3"]
        assert s3["members_on_rank"] == [8, 8] and s3["scaling"] == "strong" and s3["steps"] == 1 and s3["per_rank"]["members"] == [8, 8]
        assert abs(s3["value"] - 16 * 40 / (s3["ms_per_step"] * 1e-3)) / s3["value"] < 1e-3 and len(s3["per_rank"]["rollout_ms"]) == 2
        assert s3["speedup_vs_n1"] is None  # 4 solver steps here: not the workload of the committed N = 1 figure, no ratio is printed
        assert line["config"]["ensemble_size"] == E and line["config"]["members_on_rank"] == want and line["config"]["members_per_gpu"] is None
        assert abs(line["value"] - E * 1 * 1 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3  # value = E x lead steps x steps / time


def test_default_line_carries_like_for_like_dcae_cfg5_and_rccl_blocks():
    """the `--gpus 1 --full` line (every leg of the default configuration) must carry (i) `value` in the reference's own
    arithmetic (exact fp32) with the split-bf16 fast mode as its own block, `like_for_like` saying which is which; (ii) a `dcae` block (BASELINE
    configs[0] on the GPU in the three arithmetic modes, the dominant conv's roofline row, configs[0]'s cpu_baseline); (iii) a `cfg5` block; and
    `ranks.rccl_version` from the world-size-1 RCCL child.  Reduced step counts here; every leg runs (`--full`)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--cpu-forwards", "1", "--sustained-seconds", "0", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "ensemble-member-steps/sec" and line["n_gpus"] == 1 and line["vs_baseline"] is None and line["value"] > 0
    # (i) arithmetic: the top level is exact fp32; the fast mode has its own block and is faster, the two are never confusable
    assert line["dtype"] == "f32" and "bf16x3_mode" in line["value_dtype_note"] and line["config"]["workload"].endswith("arithmetic fp32")
    lfl = line["like_for_like"]
    assert lfl["dtype"] == "f32" and lfl["source"] == "top level" and lfl["value"] == line["value"] and lfl["roofline"] == line["roofline"]
    fast = line["bf16x3_mode"]
    assert fast["dtype"].startswith("bf16x3") and fast["value"] > 1.5 * line["value"] and fast["steps"] >= 10 and len(fast["step_ms"]) == fast["steps"]
    for roof, peak in ((line["roofline"], 157.3), (fast["roofline"], 2500.0)):
        assert roof["bound"] == "mfma" and roof["peak"] == peak and roof["unit"] == "TFLOP/s" and 0 < roof["frac"] < 1
        assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and "traffic" in roof and roof["variants"]
        dom = [v for v in roof["variants"] if v["kernel"] == roof["kernel"]][0]
        assert abs(dom["flops_per_launch"] / (dom["avg_launch_us"] * 1e-6) / 1e12 - dom["achieved"]) / dom["achieved"] < 2e-3  # achieved = measured, not modelled
    assert line["roofline"]["kernel"] == "gemm_bf16x3_v3_kernel<128, 0, false>" and "frac_of_attainable" in fast["roofline"]
    assert line["attention_kernel"]["kernel"] == "attn_fwd_f32_kernel" and fast["attention_kernel"]["kernel"] == "attn_fwd_split_kernel"
    # (ii) the autoencoder: BASELINE configs[0]
    d = line["dcae"]
    for prec in ("fp32", "bf16x3", "bf16"):
        for k in ("frames_1", "frames_8", "frames_1_graph"):
            assert d[prec][k]["encode_ms"] > 0 and d[prec][k]["decode_ms"] > 0, (prec, k)
    assert d["bf16x3"]["frames_1"]["encode_ms"] < d["fp32"]["frames_1"]["encode_ms"]
    assert d["roofline"]["bound"] == "mfma" and d["roofline"]["flops_per_launch"] > 1e9 and d["roofline"]["avg_launch_us"] > 0 and "traffic" in d["roofline"]
    cb1 = d["cpu_baseline"]
    assert cb1["kind"] == "port" and cb1["cores"] >= 1 and cb1["encode_ms"] > 0 and cb1["decode_ms"] > 0 and line["cpu_baseline_cfg1"] == cb1 and d["gpu_over_cpu_fp32"] > 1
    # (iii) cfg 5: encode -> chunk -> decode in both reduced-precision modes; the AR cpu_baseline of cfg 2
    for prec in ("bf16x3", "bf16"):
        c = line["cfg5"][prec]
        assert c["value"] > 0 and c["ms_per_step"] > c["chunk_only_ms"] > 0
    assert line["cfg5"]["bf16"]["ms_per_step"] < line["cfg5"]["bf16x3"]["ms_per_step"]
    assert line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["value"] > 0 and line["gpu_over_cpu"] > 20  # north_star: >= 20x the CPU reference
    # RCCL ran for real at world size 1
    assert line["rccl_world1"]["ok"] and line["ranks"]["rccl_version"] == line["rccl_world1"]["rccl_version"] and line["ranks"]["backend"] == "none"


def test_plain_line_times_the_steps_and_dumps_the_last_output(tmp_path):
    """a plain run (no --full): the headline fields only, the secondary blocks null; --dump-outputs writes what the last timed step
    returned, the same tensor --dump-output saves"""
    import numpy as np
    import torch

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out, pt = tmp_path / "out", str(tmp_path / "last.pt")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out), "--dump-output", pt]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "ensemble-member-steps/sec" and line["unit"] == "member-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and len(line["step_ms"]) == 3 and abs(line["value"] - 1 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    for k in ("sustained", "strong_cfg3", "other_sampler", "bf16x3_mode", "cfg5", "dcae", "rccl_world1", "roofline", "cpu_baseline", "instrumented_ms_per_step"):
        assert line[k] is None, k
    assert sorted(os.listdir(out)) == ["latents.npy"]
    got = np.load(out / "latents.npy")
    assert got.dtype == np.float32 and got.shape == (1, 1, 84, 2, 15, 30) and np.isfinite(got).all()
    assert np.array_equal(got, torch.load(pt).numpy())


def test_bench_rejects_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode != 0 and "WORLD_SIZE=3 does not match --gpus 2" in (r.stderr + r.stdout)


def test_eight_ranks_cfg3_shape_gather_equals_the_one_process_result(tmp_path):
    """BASELINE configs[2] in shape on the one GPU of the test box: `--gpus 8 --ensemble-size 16 --lead-steps 4` over gloo, every rank
    on GPU 0 - two members per rank (rank r owns members r and r + 8), one collective.  The gathered (1, 16, 84, 5, 15, 30) tensor must
    equal, BIT FOR BIT, what one process computes for the same member pairs (same kernels, same batch shape): the partition, the
    padding / trimming of the all_gather and the member order lose nothing.  Against the one-process run of all 16 members as ONE batch
    it agrees to rounding only (another stream-K cut: documented in pipelines/distributed.py).  The line carries the per-rank
    diagnostics a SCALE run is read from.

    Both arithmetic modes (75 s for the two at 3 solver steps, profiles/r04_z_gpu_sharing_first_read.log).  Eight PROCESSES on
    one GPU is also the configuration that exposed the first-read effect the wide AdaLN GEMV now guards against (csrc/rowops.hip
    ls_first_read): before that guard this comparison differed at the 1e-3 level from run to run in the split-bf16 mode."""
    import torch
    from datetime import datetime

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    sys.path.insert(0, ROOT)
    import bench
    from ladcast_amd.models import LaDCastTransformer3DModel
    from ladcast_amd.pipelines import AutoRegressive2DPipeline, roll_out_serial
    from ladcast_amd.pipelines.distributed import shard_members
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    torch.manual_seed(1234)
    model = LaDCastTransformer3DModel.from_config(bench.CONFIGS["375M"]).to("cuda").eval()
    model.enable_hip_graph(True)
    pipe = AutoRegressive2DPipeline(model, EDMDPMSolverMultistepScheduler())
    ic = (0.5 * torch.randn(84, 1, 15, 30, generator=torch.Generator().manual_seed(2))).cuda()
    kw = dict(num_inference_steps=3, return_seq_len=4, latent_transform_args={"mean": [0.0] * 84, "std": [1.0] * 84, "target_std": 0.5},
              total_lead_time_hour=24, sampler_type="edm", return_latent=True, known_latents_override=ic)
    for mode in ("bf16x3", "fp32"):
        dump = str(tmp_path / f"gathered_{mode}.pt")
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--backend", "gloo", "--share-gpus", "--ensemble-size", "16", "--lead-steps", "4",
               "--steps", "1", "--warmup", "0", "--cpu-forwards", "0", "--sustained-seconds", "0", "--no-kernel-timers", "--precision", mode, "--dump-output", dump,
               "--solver-steps", "3",  # 5 forwards per chunk: eight ranks share ONE GPU here, the literal 20 steps cost minutes of suite time
               "--no-strong-cfg3"]  # (the strong_cfg3 leg - 16 x 40 member-steps more on the shared GPU - is asserted in the two-rank test above)
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["n_gpus"] == 8 and line["scaling"] == "strong" and line["config"]["members_on_rank"] == [2] * 8
        pr = line["ranks"]["per_rank"]
        assert len(pr["ms_per_step"]) == 8 and pr["members"] == [2] * 8 and len(pr["gather_ms_per_step"]) == 8
        assert pr["ms_per_step_min"] <= pr["ms_per_step_max"] and all(v > 0 for v in pr["rollout_ms_per_step"])
        assert abs(line["value"] - 16 * 4 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        assert len(line["ranks"]["devices"]) == 8
        got = torch.load(dump)
        assert got.shape == (1, 16, 84, 5, 15, 30) and torch.isfinite(got).all()
        # the same work in ONE process: the eight member pairs one after the other, then all 16 members as one batch
        model.set_gemm_precision(mode)
        want = torch.empty_like(got)
        for rank in range(8):
            ids = shard_members(16, rank, 8)
            assert ids == [rank, rank + 8]
            want[:, ids] = roll_out_serial(None, [datetime(2018, 1, 1, 0)], pipe, ensemble_size=2, member_ids=ids, **kw)
        e_pairs = ((want.double() - got.double()).norm() / want.double().norm()).item()
        whole = roll_out_serial(None, [datetime(2018, 1, 1, 0)], pipe, ensemble_size=16, **kw)
        e_whole = ((whole.double() - got.double()).norm() / got.double().norm()).item()
        print(f"\n[{mode}] 8 ranks x 2 members vs one process pair by pair: {'bit for bit' if torch.equal(got, want) else f'rel-L2 {e_pairs:.2e}'}; "
              f"vs all 16 members as one batch: rel-L2 {e_whole:.2e}")
        assert torch.equal(got[:, :, :, 0], want[:, :, :, 0])  # slot 0: the IC latent, member order and padding of the gather
        assert torch.equal(got, want)
        assert e_whole < (1e-5 if mode == "fp32" else 1e-4)
