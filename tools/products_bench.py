"""Times ldc_rollout_products (stats + 5 quantiles + 2 thresholds) against (i) ldc_rollout_reliability on the same input (reliability.hip
is the code of the commit before the products kernel: the project's yardstick for a one-pass read of the members), (ii) a torch
composition of the same products on the device (sort / mean / std / gather-lerp / compare) and (iii) the DC-AE decode of the same frame
batch (the hook the products ride on), with device events around every call -> profiles/products_timing.json.

    python tools/products_bench.py [--out profiles/products_timing.json] [--reps 20] [--no_decode]

Every shape runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Inside a child the calls alternate (A, B, C, A, B, C, ...) after a warm-up of each, so drift of the machine
hits them alike; the figure reported is the median, with the minimum and the maximum beside it.  Bytes are what the algorithm must move,
computed from the shapes: products read the members once and write 4 + Q + P planes per (channel, lead time); reliability reads the
members and the truth once and writes next to nothing.  `expected_ms_if_bandwidth_bound` is reliability's median time x (bytes moved by
products / bytes moved by reliability).  The decode is that of the DC_AE_84 architecture (benchlib/configs.py) with random weights in
bf16x3, one lead time's members per decoder call as the driver runs it, timed after the alternating loop (1 warm-up, 3 repetitions)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 84, 4, 120, 240), (10, 84, 4, 120, 240))  # M, C, L, H, W
QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)
THRESHOLDS = ((0.5, 1), (-0.5, -1))  # (value on every channel, direction)
STEP_TIMEOUT_S = 300


def _events(f):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_composition(x, quantiles, thr, dirs):
    """the same products from torch ops on the device; x (M, C, L, H, W) -> (stats (4, ...), quant (Q, ...), exceed (P, ...))"""
    import math

    import torch

    M = x.shape[0]
    s = torch.sort(x, dim=0).values
    stats = torch.stack([x.mean(0), x.std(0, unbiased=True), s[0], s[M - 1]])
    planes = []
    for q in quantiles:
        pos = q * (M - 1)
        lo = min(int(math.floor(pos)), M - 1)
        t = pos - lo
        planes.append(s[lo] if t == 0 else torch.lerp(s[lo], s[min(lo + 1, M - 1)], t))
    Mf = torch.tensor(float(M), device=x.device)  # a tensor divisor: a true division, where a Python scalar would become a multiplication by 1 / M
    ex = [((x > v) if d > 0 else (x < v)).sum(0).float() / Mf for v, d in zip(thr, dirs)]
    return stats, torch.stack(planes), torch.stack(ex)


def worker(M, C, L, H, W, reps, decode):
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
    Q, P = len(QUANTILES), len(THRESHOLDS)
    dirs = [d for _, d in THRESHOLDS]
    desc = hip.products_desc(QUANTILES, M, dirs)
    thr = torch.tensor([[v] * C for v, _ in THRESHOLDS], device=dev)
    stats, quant, exceed = torch.empty(4, C, L, H, W, device=dev), torch.empty(Q, C, L, H, W, device=dev), torch.empty(P, C, L, H, W, device=dev)
    out, hist, hist_w, ninv = (torch.empty(3, C, L, device=dev), torch.empty(C, L, M + 1, dtype=torch.int32, device=dev),
                               torch.empty(C, L, M + 1, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev))
    nb_rel = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    ws_rel = torch.empty(nb_rel // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def products():
        st = hip.lib.ldc_rollout_products(p(x), ms, ls, cs, None, None, 1.0, None, M, C, C, L, H, W, ctypes.byref(desc), p(thr), p(stats), p(quant),
                                          p(exceed), L, 0, stream)
        assert st == 0, st

    def reliability():
        st = hip.lib.ldc_rollout_reliability(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, -1, p(out),
                                             p(hist), p(hist_w), p(ninv), L, 0, p(ws_rel), nb_rel, stream)
        assert st == 0, st

    thr_vals = [v for v, _ in THRESHOLDS]
    calls = dict(ldc_rollout_products=products, ldc_rollout_reliability=reliability,
                 torch_composition=lambda: torch_composition(x, QUANTILES, thr_vals, dirs))
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything
    r_stats, r_quant, r_ex = torch_composition(x, QUANTILES, thr_vals, dirs)
    torch.testing.assert_close(stats, r_stats, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(quant, r_quant, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(exceed, r_ex, rtol=1e-6, atol=0)
    assert bool((stats[2:] == r_stats[2:]).all())
    del r_stats, r_quant, r_ex
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
    points = C * L * H * W
    read_p, write_p = M * points * 4, (4 + Q + P) * points * 4
    read_r, write_r = (M + 1) * points * 4, (out.numel() + hist.numel() + hist_w.numel() + ninv.numel()) * 4
    gb = dict(ldc_rollout_products=(read_p + write_p) / 1e9, ldc_rollout_reliability=(read_r + write_r) / 1e9, torch_composition=(read_p + write_p) / 1e9)
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), products=dict(stats=4, quantiles=list(QUANTILES), thresholds=[list(v) for v in THRESHOLDS]), reps=reps,
               bytes=dict(products_read=read_p, products_written=write_p, reliability_read=read_r, reliability_written=write_r),
               device=torch.cuda.get_device_name(0), **note)
    for k, v in times.items():
        med = statistics.median(v)
        res[k] = dict(median_ms=round(med, 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), gbytes=round(gb[k], 4),
                      gbytes_per_s=round(gb[k] / (med * 1e-3), 1))
    res["torch_composition"]["note"] = "GB/s over the bytes the algorithm must move, not over what the torch ops move"
    expected = res["ldc_rollout_reliability"]["median_ms"] * gb["ldc_rollout_products"] / gb["ldc_rollout_reliability"]
    res["expected_ms_if_bandwidth_bound"] = round(expected, 4)
    res["products_over_expected"] = round(res["ldc_rollout_products"]["median_ms"] / expected, 3)
    res["torch_over_products"] = round(res["torch_composition"]["median_ms"] / res["ldc_rollout_products"]["median_ms"], 2)
    print("RESULT " + json.dumps(res))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "products_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_decode", action="store_true", help="leave out the DC-AE decode of the same batch")
    ap.add_argument("--worker", type=int, nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(*args.worker, args.reps, not args.no_decode)
        return 0
    me = [sys.executable, os.path.abspath(__file__)]
    results = []
    for shape in SHAPES:
        st, res = _child(me + ["--reps", str(args.reps), "--worker", *map(str, shape)] + (["--no_decode"] if args.no_decode else []), str(shape))
        if st:
            return st
        results.append(res)
    _write(args.out, dict(tool="tools/products_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
