"""Times ldc_derive_fields (10 m wind speed, 500 - 1000 hPa thickness, 200 - 850 hPa shear of a (M, C, L, H, W) = (20, 84, 2, 120, 240) decode
batch) against (i) a plain device copy that moves the same number of bytes (the 8 distinct source planes read and the 3 planes written per
member and lead time), (ii) the torch composition of the same fields on the device, and times (iii) one initial time of
`score_latent_rollout` with and without `derived` on the same build, with device events around the calls and the host clock around the
driver -> profiles/derive_timing.json.  The kernel and the copy are timed as 10 calls enqueued back to back per sample (one call is a few
microseconds: a single one between two events measures the host's way to the launch), the kernel through the C ABI with its arguments
prepared; one call through the Python wrapper is timed beside them.  Source planes (37 MB) and copy buffers (2 x 25 MB) both fit the
last-level cache: both run warm.

    python tools/derive_bench.py [--out profiles/derive_timing.json] [--reps 20] [--no_driver]

The measurement runs in a child process under a time limit; the parent never opens the device.  The calls alternate (A, B, C, A, B, C, ...)
after a warm-up of each, so drift of the machine hits them alike; the figure reported is the median, with the minimum and the maximum
beside it.  The driver is timed on the DC_AE_84 architecture (benchlib/configs.py) with random weights in bf16x3, 2 lead times decoded in
one decoder call, truth and climatology resident on the device; 1 warm-up and 3 alternating repetitions of each variant."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (20, 84, 2, 120, 240)  # M, C, L, H, W
STEP_TIMEOUT_S = 420
BURST = 10  # kernel calls per timed sample


def _events(f):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def example_fields():
    sys.path.insert(0, ROOT)
    from ladcast_amd.evaluate.derived import parse_derived
    from ladcast_amd.evaluate.track import VARIABLE_NAMES
    from ladcast_amd.evaluate.validate_AR import column_names

    names = column_names(VARIABLE_NAMES)
    return parse_derived([["wind_speed_10m", "speed", "10m_u_component_of_wind", "10m_v_component_of_wind"],
                          ["thickness_500_1000", "diff", "geopotential_level500", "geopotential_level1000"],
                          ["shear_200_850", "shear", "u_component_of_wind_level200", "v_component_of_wind_level200", "u_component_of_wind_level850",
                           "v_component_of_wind_level850"]], names)


def torch_composition(x, fields, mean, std):
    """the same fields from torch ops on the device; x (M, C, L, H, W) normalised -> (M, D, L, H, W)"""
    import torch

    ch = lambda c: x[:, c] * std[c] + mean[c]  # noqa: E731
    out = []
    for f in fields:
        p = [ch(c) for c in f.channels]
        if f.kind == "diff":
            out.append(p[0] - p[1])
            continue
        a, b = p[0].double(), p[1].double()
        if f.kind == "shear":
            a, b = a - p[2].double(), b - p[3].double()
        out.append(torch.sqrt(a * a + b * b).float())
    return torch.stack(out, dim=1)


def worker(reps, driver):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip
    from ladcast_amd.evaluate.derived import KINDS, derive_forecast

    M, C, L, H, W = SHAPE
    dev = "cuda"
    fields = example_fields()
    D, planes = len(fields), len({c for f in fields for c in f.channels})
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(M, C, L, H, W, device=dev, generator=g)
    mean, std = torch.randn(C, device=dev, generator=g), torch.rand(C, device=dev, generator=g) + 0.5
    out = torch.empty(M, D, L, H, W, device=dev)
    moved = (planes + D) * M * L * H * W * 4  # bytes the kernel must read and write
    src, dst = torch.randn(moved // 8, device=dev, generator=g), torch.empty(moved // 8, device=dev)  # a copy reads and writes: half each
    desc = hip.derive_desc([(KINDS[f.kind], f.channels) for f in fields])
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():  # the C ABI with everything prepared, BURST calls back to back: the kernel, not the host's way to it
        for _ in range(BURST):
            st = hip.lib.ldc_derive_fields(p(x), x.stride(0), x.stride(2), x.stride(1), None, p(mean), p(std), 1.0, M, L, C, H * W, desc, D, p(out),
                                           out.stride(0), out.stride(2), out.stride(1), stream)
            assert st == 0, st

    def copy():
        for _ in range(BURST):
            dst.copy_(src)

    calls = dict(ldc_derive_fields=kernel, device_copy=copy, derive_forecast_wrapper=lambda: derive_forecast(x, fields, mean=mean, std=std, out=out),
                 torch_composition=lambda: torch_composition(x, fields, mean, std))
    per_sample = dict(ldc_derive_fields=BURST, device_copy=BURST)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    torch.testing.assert_close(out, torch_composition(x, fields, mean, std), rtol=1e-6, atol=1e-6)  # results must agree before a time means anything
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            times[k].append(_events(f) / per_sample.get(k, 1))
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), fields=[f.name for f in fields], source_planes=planes, bytes_moved=moved, reps=reps,
               device=torch.cuda.get_device_name(0))
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), gbytes_per_s=round(moved / 1e9 / (med * 1e-3), 1))
    res["ldc_derive_fields"]["note"] = res["device_copy"]["note"] = f"per call, {BURST} calls enqueued back to back between the two events"
    res["derive_forecast_wrapper"]["note"] = "one call through the Python wrapper: host-bound at this size (the device waits for the launch)"
    res["torch_composition"]["note"] = "GB/s over the bytes the algorithm must move, not over what the torch ops move"
    res["derive_over_copy"] = round(res["ldc_derive_fields"]["median_ms"] / res["device_copy"]["median_ms"], 3)
    res["torch_over_derive"] = round(res["torch_composition"]["median_ms"] / res["ldc_derive_fields"]["median_ms"], 2)
    if driver:
        from benchlib.configs import CONFIG_DCAE_84
        from ladcast_amd.evaluate.evaluate_ens_gpu import lat_weights_for, score_latent_rollout
        from ladcast_amd.models import AutoencoderDC

        del x, out, src, dst
        torch.manual_seed(1234)
        model = AutoencoderDC.from_config(CONFIG_DCAE_84).to(dev).eval()
        model.set_gemm_precision("bf16x3")
        lat = torch.randn(M, int(CONFIG_DCAE_84["latent_channels"]), L, H // 8, W // 8, device=dev, generator=g)
        truth, clim = torch.randn(L, C, H, W, device=dev, generator=g), torch.randn(L, C, H, W, device=dev, generator=g)
        lat_w = lat_weights_for(H)
        variants = dict(plain=None, derived=fields)

        def run(derived):
            t0 = time.perf_counter()
            r = score_latent_rollout(lat, model, mean.cpu(), std.cpu(), truth, list(range(L)), clim, list(range(L)), lat_w, sst_channel=82,
                                     decode_batch_frames=M * L, derived=derived)
            assert r["crps"].shape == (C + (len(derived) if derived else 0), L)
            return (time.perf_counter() - t0) * 1e3

        for d in variants.values():
            run(d)
        drv = {k: [] for k in variants}
        for _ in range(3):
            for k, d in variants.items():
                drv[k].append(run(d))
        res["score_latent_rollout"] = {k: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), reps=3)
                                       for k, v in drv.items()}
        res["score_latent_rollout"]["what"] = f"DC_AE_84, random weights, bf16x3, one decoder call of {M * L} frames, tables on the device; host clock"
        res["score_latent_rollout"]["derived_over_plain"] = round(statistics.median(drv["derived"]) / statistics.median(drv["plain"]), 4)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derive_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_driver", action="store_true", help="leave out the two score_latent_rollout runs")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args.reps, not args.no_driver)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(args.reps)] + (["--no_driver"] if args.no_driver else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        print(f"no result after {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
        return 124
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:], f"exit status {r.returncode}; stopping", sep="\n", file=sys.stderr)
        return r.returncode if r.returncode > 0 else 1
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/derive_bench.py", result=json.loads(line[len("RESULT "):])), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
