"""Times ldc_derive_sphere (850 hPa relative vorticity and 200 hPa divergence of a (M, C, L, H, W) = (20, 84, 2, 120, 240) decode batch on the
120-row grid, whose last row is the north pole) against (i) a plain device copy that moves the same number of bytes (the 4 source planes
read and the 2 planes written per member and lead time), (ii) the torch composition of the same formula in fp64 on the device (`roll` for
the longitude wrap, slicing for the row neighbours, a mean for the pole row), and times (iii) one initial time of `score_latent_rollout`
with and without the two fields on the same build, with device events around the calls and the host clock around the driver ->
profiles/sphere_derive_timing.json.  The method is that of tools/derive_bench.py: the kernel and the copy are timed as 10 calls enqueued back
to back per sample (one call is a few microseconds: a single one between two events measures the host's way to the launch), the kernel
through the C ABI with its arguments prepared; one call through the Python wrapper is timed beside them.  Source planes and copy buffers fit
the last-level cache: both run warm.

    python tools/sphere_derive_bench.py [--out profiles/sphere_derive_timing.json] [--reps 20] [--no_driver]

The measurement runs in a child process under a time limit; the parent never opens the device.  The calls alternate (A, B, C, A, B, C, ...)
after 3 warm-ups of each, so drift of the machine hits them alike; the figure reported is the median, with the minimum and the maximum
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
    return parse_derived([["vort850", "vorticity", "u_component_of_wind_level850", "v_component_of_wind_level850"],
                          ["div200", "divergence", "u_component_of_wind_level200", "v_component_of_wind_level200"]], names)


def torch_composition(x, fields, mean, std, tab, k):
    """the same fields from torch ops on the device, in fp64; x (M, C, L, H, W) normalised, tab (4, H) fp64 on the device -> (M, D, L, H, W)"""
    import torch

    c, q, r, pc = (t.view(-1, 1) for t in tab)
    H = x.shape[-2]
    pole = r.view(-1) == 0
    ch = lambda n: (x[:, n] * std[n] + mean[n]).double()  # noqa: E731
    out = []
    for f in fields:
        u, v = ch(f.channels[0]), ch(f.channels[1])
        a, b = (u, v) if f.kind == "vorticity" else (-v, u)
        ac = a * c
        north, south = torch.cat([ac[..., 1:, :], ac[..., -1:, :]], dim=-2), torch.cat([ac[..., :1, :], ac[..., :-1, :]], dim=-2)
        z = ((torch.roll(b, -1, -1) - torch.roll(b, 1, -1)) * k - (north - south) * q) * r
        for j in torch.nonzero(pole).view(-1).tolist():
            jp = 1 if j == 0 else H - 2
            z[..., j, :] = a[..., jp, :].mean(dim=-1, keepdim=True) * pc[j]
        out.append(z.float())
    return torch.stack(out, dim=1)


def worker(reps, driver):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip
    from ladcast_amd.evaluate.derived import KINDS, derive_forecast, sphere_row_tables
    from ladcast_amd.evaluate.rollout_metrics import row_latitudes

    M, C, L, H, W = SHAPE
    dev = "cuda"
    fields = example_fields()
    D, planes = len(fields), len({c for f in fields for c in f.channels})
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(M, C, L, H, W, device=dev, generator=g)
    mean, std = torch.randn(C, device=dev, generator=g), torch.rand(C, device=dev, generator=g) + 0.5
    out = torch.empty(M, D, L, H, W, device=dev)
    host_tab, k = sphere_row_tables(row_latitudes(H), W)
    tab = torch.from_numpy(host_tab).to(dev)
    moved = (planes + D) * M * L * H * W * 4  # bytes the kernel must read and write
    src, dst = torch.randn(moved // 8, device=dev, generator=g), torch.empty(moved // 8, device=dev)  # a copy reads and writes: half each
    desc = hip.sphere_desc([(KINDS[f.kind], f.channels) for f in fields])
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def kernel():  # the C ABI with everything prepared, BURST calls back to back: the kernel, not the host's way to it
        for _ in range(BURST):
            st = hip.lib.ldc_derive_sphere(p(x), x.stride(0), x.stride(2), x.stride(1), None, p(mean), p(std), 1.0, M, L, C, H, W, p(tab), k, desc, D,
                                           p(out), out.stride(0), out.stride(2), out.stride(1), stream)
            assert st == 0, st

    def copy():
        for _ in range(BURST):
            dst.copy_(src)

    calls = dict(ldc_derive_sphere=kernel, device_copy=copy, derive_forecast_wrapper=lambda: derive_forecast(x, fields, mean=mean, std=std, out=out),
                 torch_composition=lambda: torch_composition(x, fields, mean, std, tab, k))
    per_sample = dict(ldc_derive_sphere=BURST, device_copy=BURST)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything: fields of about 1e-5 1/s; torch de-normalises with a contracted multiply-add
    torch.testing.assert_close(out, torch_composition(x, fields, mean, std, tab, k), rtol=1e-4, atol=1e-9)
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, f in calls.items():
            times[name].append(_events(f) / per_sample.get(name, 1))
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), fields=[f.name for f in fields], source_planes=planes, bytes_moved=moved, reps=reps,
               device=torch.cuda.get_device_name(0), kernel="plain form: one wave per row, neighbours through the caches (no LDS tile was built)")
    for name, v in times.items():
        med = statistics.median(v)
        res[name] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), gbytes_per_s=round(moved / 1e9 / (med * 1e-3), 1))
    res["ldc_derive_sphere"]["note"] = res["device_copy"]["note"] = f"per call, {BURST} calls enqueued back to back between the two events"
    res["derive_forecast_wrapper"]["note"] = "one call through the Python wrapper: host-bound at this size (the device waits for the launch)"
    res["torch_composition"]["note"] = "GB/s over the bytes the algorithm must move, not over what the torch ops move"
    res["sphere_over_copy"] = round(res["ldc_derive_sphere"]["median_ms"] / res["device_copy"]["median_ms"], 3)
    res["torch_over_sphere"] = round(res["torch_composition"]["median_ms"] / res["ldc_derive_sphere"]["median_ms"], 2)
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
        drv = {name: [] for name in variants}
        for _ in range(3):
            for name, d in variants.items():
                drv[name].append(run(d))
        res["score_latent_rollout"] = {name: dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), reps=3)
                                       for name, v in drv.items()}
        res["score_latent_rollout"]["what"] = f"DC_AE_84, random weights, bf16x3, one decoder call of {M * L} frames, tables on the device; host clock"
        res["score_latent_rollout"]["derived_over_plain"] = round(statistics.median(drv["derived"]) / statistics.median(drv["plain"]), 4)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sphere_derive_timing.json"))
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
        json.dump(dict(tool="tools/sphere_derive_bench.py", result=json.loads(line[len("RESULT "):])), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
