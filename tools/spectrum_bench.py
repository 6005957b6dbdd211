"""Times ldc_rollout_spectrum against (i) ldc_rollout_reliability on the same input (the project's yardstick for one pass over the same
bytes), (ii) a torch composition of the same quantities (torch.fft.rfft in fp32 on the de-normalised fields, plus the reductions) and
(iii) the DC-AE decode of the same frame batch (the hook the spectrum rides on), with device events around every call
-> profiles/spectrum_timing.json; and records the accuracy of the kernel and of the torch composition -> profiles/spectrum_accuracy.json.

    python tools/spectrum_bench.py [--out profiles/spectrum_timing.json] [--accuracy_out profiles/spectrum_accuracy.json] [--reps 20]

Every step runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Inside a timing child the calls alternate (A, B, C, A, B, C, ...) after a warm-up of each, so drift of the
machine hits them alike; the figure reported is the median, with the minimum and the maximum beside it.  `gbytes` is what the algorithm
must read (the forecast and the truth once); `gfma` the folded transform's multiply-adds, (M + 2) sequences x W / 2 bins x (W / 2 + 1)
terms x 2 components per row.  The decode is that of the DC_AE_84 architecture (benchlib/configs.py) with random weights in bf16x3, one lead
time's members per decoder call as the driver runs it, timed after the alternating loop (1 warm-up, 3 repetitions); `--no_decode` leaves it out.

The accuracy child runs the cases of tests/spectrum_refs.py (the shapes of tests/test_gpu_spectrum.py and the pivot case: mean 2e5,
amplitude 1e-2 at wavenumber W / 2 - 1) and records the worst error / bound per case, for the kernel and for the torch composition."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 84, 4, 120, 240), (10, 84, 4, 120, 240))  # M, C, L, H, W
STEP_TIMEOUT_S = 300


def _events(f):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def worker(M, C, L, H, W, reps, decode):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip
    from tests import spectrum_refs as R

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    w = torch.cos(torch.deg2rad(torch.linspace(-88.5, 90.0, H, device=dev)))
    w = (w / w.mean()).contiguous()
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = W // 2 + 1
    spec, spec_n = torch.empty(3, C, L, K, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev)
    out, hist, hist_w, ninv = (torch.empty(3, C, L, device=dev), torch.empty(C, L, M + 1, dtype=torch.int32, device=dev),
                               torch.empty(C, L, M + 1, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev))
    nb_spec = int(hip.lib.ldc_rollout_spectrum_workspace_bytes(M, C, L, H, W))
    nb_rel = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    ws_spec, ws_rel = torch.empty(nb_spec // 4, device=dev), torch.empty(nb_rel // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def spectrum():
        st = hip.lib.ldc_rollout_spectrum(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, p(spec), p(spec_n),
                                          L, 0, p(ws_spec), nb_spec, stream)
        assert st == 0, st

    def reliability():
        st = hip.lib.ldc_rollout_reliability(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, -1, p(out),
                                             p(hist), p(hist_w), p(ninv), L, 0, p(ws_rel), nb_rel, stream)
        assert st == 0, st

    calls = dict(ldc_rollout_spectrum=spectrum, ldc_rollout_reliability=reliability, torch_composition=lambda: R.torch_composition(x, t, w))
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything: the kernel against the torch composition to fp32-FFT accuracy on this zero-mean input
    ref = R.torch_composition(x, t, w)
    for i, k in enumerate(R.NAMES):
        torch.testing.assert_close(spec[i], ref[k], rtol=2e-3, atol=1e-6)
    assert int(spec_n.abs().sum()) == 0
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            times[k].append(_events(f))
    note = {}
    if decode:  # the decode of the same frame batch, one lead time (M frames) per decoder call as the driver runs it; 1 warm-up, 3 repetitions
        from benchlib.configs import CONFIG_DCAE_84
        from ladcast_amd.models import AutoencoderDC

        torch.manual_seed(1234)
        model = AutoencoderDC.from_config(CONFIG_DCAE_84).to(dev).eval()
        model.set_gemm_precision("bf16x3")
        lat = torch.randn(L, M, int(CONFIG_DCAE_84["latent_channels"]), H // 8, W // 8, device=dev, generator=g)

        def decode_batch():
            with torch.no_grad():
                for l in range(L):
                    y = model.decode(lat[l]).sample
            assert tuple(y.shape) == (M, C, H, W), tuple(y.shape)

        decode_batch()
        torch.cuda.synchronize()
        v = [_events(decode_batch) for _ in range(3)]
        note["dcae_decode_same_batch"] = dict(median_ms=round(statistics.median(v), 2), min_ms=round(min(v), 2), max_ms=round(max(v), 2), reps=3,
                                              what=f"DC_AE_84, random weights, bf16x3, {L} decoder calls of {M} frames")
    else:
        note["dcae_decode_same_batch"] = "not measured (--no_decode)"
    gbytes = (x.numel() + t.numel()) * 4 / 1e9
    gfma = C * L * H * (M + 2) * (W // 2) * (W // 2 + 1) * 2 / 1e9
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), reps=reps, gbytes=round(gbytes, 4), gfma=round(gfma, 3), workspace_mb=round(nb_spec / 1e6, 3),
               device=torch.cuda.get_device_name(0), **note)
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), gbytes_per_s=round(gbytes / (med * 1e-3), 1))
    res["ldc_rollout_spectrum"]["tfma_per_s"] = round(gfma / res["ldc_rollout_spectrum"]["median_ms"], 3)
    print("RESULT " + json.dumps(res))


def accuracy_worker():
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd.evaluate import rollout_spectrum
    from tests import spectrum_refs as R

    def dev(a):
        return torch.from_numpy(np.array(a)).cuda()

    cases = [(str(s), R.case(s)) for s in R.SHAPES] + [("pivot: mean 2e5, amplitude 1e-2 at k0 = W / 2 - 1, W = 240", R.pivot_case())]
    rows = []
    for name, c in cases:
        ref = R.spectrum_ref(c["x"], c["t"], c["w"])
        xd, td, wd = dev(c["x"]), dev(c["t"]), dev(c["w"])
        got = {k: v.cpu().numpy() for k, v in rollout_spectrum(xd, td, wd).items()}
        tc = {k: v.cpu().numpy() for k, v in R.torch_composition(xd, td, wd).items()}
        row = dict(case=name, kernel_worst_err_over_bound={k: round(R.ratio_of(got[k], ref[k]), 5) for k in R.NAMES},
                   torch_fp32_composition_worst_err_over_bound={k: float(f"{R.ratio_of(tc[k], ref[k]):.4g}") for k in R.NAMES})
        if "k0" in c:
            k0 = c["k0"]
            row["at_k0"] = {k: dict(oracle=float(ref[k][0][0, 0, k0]), bound=float(ref[k][1][0, 0, k0]), kernel=float(got[k][0, 0, k0]),
                                    torch_fp32_composition=float(tc[k][0, 0, k0])) for k in R.NAMES}
        rows.append(row)
    print("RESULT " + json.dumps(dict(device=torch.cuda.get_device_name(0), measured_on="GPU", cases=rows)))


def _child(cmd, what):
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        print(f"{what}: no result after {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
        return 124, None
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-4000:], f"{what}: exit status {r.returncode}; stopping", sep="\n", file=sys.stderr)
        return (r.returncode if r.returncode > 0 else 1), None
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
    print(line)
    return 0, json.loads(line[len("RESULT "):])


def _write(path, obj):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_timing.json"))
    ap.add_argument("--accuracy_out", default=os.path.join(ROOT, "profiles", "spectrum_accuracy.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_decode", action="store_true", help="leave out the DC-AE decode of the same batch")
    ap.add_argument("--worker", type=int, nargs=5, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--accuracy_worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(*args.worker, args.reps, not args.no_decode)
        return 0
    if args.accuracy_worker:
        accuracy_worker()
        return 0
    me = [sys.executable, os.path.abspath(__file__)]
    st, acc = _child(me + ["--accuracy_worker"], "accuracy")
    if st:
        return st
    _write(args.accuracy_out, dict(tool="tools/spectrum_bench.py", **acc))
    results = []
    for shape in SHAPES:
        st, res = _child(me + ["--reps", str(args.reps), "--worker", *map(str, shape)] + (["--no_decode"] if args.no_decode else []),
                         str(shape))
        if st:
            return st
        results.append(res)
    _write(args.out, dict(tool="tools/spectrum_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
