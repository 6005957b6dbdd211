"""Times ldc_rollout_reliability against ldc_rollout_scores on the same input and against the plain torch expression of the same
quantities, with device events around every call -> profiles/reliability_timing.json.

    python tools/reliability_bench.py [--out profiles/reliability_timing.json] [--reps 20]

Every shape runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Inside a child the three calls alternate (A, B, C, A, B, C, ...) after a warm-up of each, so drift of the
machine hits them alike; the figure reported is the median, with the minimum and the maximum beside it.  `gbytes` is what the algorithm
must read (the forecast and the truth once), `gbytes_per_s` that over the median: an achieved rate of the call, not a share of peak."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 84, 2, 120, 240), (10, 84, 4, 120, 240))  # M, C, L, H, W
STEP_TIMEOUT_S = 240


def torch_expression(x, t, w, M):
    """the same quantities in plain torch: x (M, C, L, H, W), t (C, L, H, W), w (H,)"""
    import torch

    C, L = t.shape[:2]
    wv = w.view(1, 1, -1, 1)
    mse = ((x.mean(0) - t) ** 2 * wv).mean((-2, -1))
    var = (x.var(dim=0, unbiased=True) * wv).mean((-2, -1))
    ssr = ((M + 1) / M) ** 0.5 * torch.sqrt(var / mse)
    b = (x < t).sum(0) + (x == t).sum(0) // 2
    idx = (torch.arange(C * L, device=x.device).view(C, L, 1, 1) * (M + 1) + b).reshape(-1)
    hist = torch.bincount(idx, minlength=C * L * (M + 1))
    hist_w = torch.bincount(idx, weights=wv.expand_as(b).reshape(-1), minlength=C * L * (M + 1))
    return mse, var, ssr, hist, hist_w


def worker(M, C, L, H, W, reps):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    w = torch.cos(torch.deg2rad(torch.linspace(-88.5, 90.0, H, device=dev)))
    w = (w / w.mean()).contiguous()
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, hist, hist_w, ninv = (torch.empty(3, C, L, device=dev), torch.empty(C, L, M + 1, dtype=torch.int32, device=dev),
                               torch.empty(C, L, M + 1, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev))
    nb_rel = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    nb_sc = int(hip.lib.ldc_rollout_scores_workspace_bytes(C, L, H, W))
    ws_rel, ws_sc = torch.empty(nb_rel // 4, device=dev), torch.empty(nb_sc // 4, device=dev)
    out5 = torch.empty(5, C, L, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def reliability():
        st = hip.lib.ldc_rollout_reliability(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, -1, p(out),
                                             p(hist), p(hist_w), p(ninv), L, 0, p(ws_rel), nb_rel, stream)
        assert st == 0, st

    def scores():
        st = hip.lib.ldc_rollout_scores(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), None, 0, 0, None, p(w), M, C, L, H, W, -1,
                                        p(out5), L, 0, p(ws_sc), nb_sc, stream)
        assert st == 0, st

    calls = dict(ldc_rollout_reliability=reliability, ldc_rollout_scores=scores, torch_expression=lambda: torch_expression(x, t, w, M))
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything: the histogram exactly, the scores to fp32 accuracy
    ref = torch_expression(x, t, w, M)
    assert torch.equal(hist.reshape(-1).long(), ref[3]), "rank histogram differs from the torch expression"
    torch.testing.assert_close(out[1], ref[1], rtol=1e-4, atol=0)
    torch.testing.assert_close(out[0], out5[1], rtol=0, atol=0)
    times = {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    gbytes = (x.numel() + t.numel()) * 4 / 1e9
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), reps=reps, gbytes=round(gbytes, 4), workspace_mb=round(nb_rel / 1e6, 3), device=torch.cuda.get_device_name(0))
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), gbytes_per_s=round(gbytes / (med * 1e-3), 1))
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reliability_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--worker", type=int, nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(*args.worker, args.reps)
        return 0
    results = []
    for shape in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--worker", *map(str, shape)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"{shape}: no result after {STEP_TIMEOUT_S} s; stopping", file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], f"{shape}: exit status {r.returncode}; stopping", sep="\n", file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = next(ln for ln in r.stdout.splitlines() if ln.startswith("RESULT "))
        results.append(json.loads(line[len("RESULT "):]))
        print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/reliability_bench.py", results=results), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
