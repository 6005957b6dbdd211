"""Times ldc_rollout_fss (8 events, 4 radii) beside ldc_rollout_events on the same events and forecast, with device events around the
C-ABI calls -> profiles/fss_timing.json.

    python tools/fss_bench.py [--out profiles/fss_timing.json] [--reps 20]

Every shape runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Two calls are timed: `ldc_rollout_fss` and `ldc_rollout_events` (the point-wise verification of the same 8
events, one per channel: it reads the same members and truth).  Each gets a warmed variant (the calls alternate A, B, A, B, ... after 3
warm-ups of each, so drift of the machine hits them alike) and a cold variant (a 1 GiB buffer is written before every timed call, which
leaves nothing of the forecast in L2 or in the memory-side cache).  The figure reported is the median, with the minimum and the maximum
beside it.  A torch composition of the same sums (circular padding in longitude, zero padding in latitude, `avg_pool2d` with divisor 1
per event, radius and lead time, float64) runs once after a warm-up, for scale; its sums must agree with the kernel's before a time
means anything.  The split of a call over its kernels comes from a separate run of one worker under a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/fss_bench.py --reps 5 --worker 50 8 4 120 240"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 8, 4, 120, 240), (10, 8, 4, 120, 240))  # M, E (= C), L, H, W
RADII = (0, 2, 6, 20)  # 1.5, 7.5, 19.5 and 61.5 degrees wide on the 1.5 degree grid
THRESHOLDS = (0.5, -0.5, 0.0, 1.0, -1.0, 0.25, -0.25, 1.5)
STEP_TIMEOUT_S = 300
FLUSH_BYTES = 1 << 30


def _events(f, before=None):
    import torch

    if before is not None:
        before()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_composition(x, t, w, events, radii):
    """the same sums from torch ops on the device; x (M, C, L, H, W), t (C, L, H, W), w (H,) -> (E, S, L, 6) float64.  No NaN in the
    inputs: every point is valid, N is the number of window points inside the grid"""
    import torch
    import torch.nn.functional as F

    M, C, L, H, W = x.shape
    wp = w.double().view(1, H, 1)
    ones = torch.ones(L, 1, H, W, dtype=torch.float64, device=x.device)
    out = torch.zeros(len(events), len(radii), L, 6, dtype=torch.float64, device=x.device)

    def window(a, r):  # (L, 1, H, W) -> sums over the clipped, periodic window
        a = F.pad(F.pad(a, (r, r, 0, 0), mode="circular"), (0, 0, r, r))
        return F.avg_pool2d(a, 2 * r + 1, stride=1, divisor_override=1)[:, 0]

    for e, (c, d, thr) in enumerate(events):
        n = ((x[:, c] > thr) if d > 0 else (x[:, c] < thr)).sum(0).double().unsqueeze(1)
        o = ((t[c] > thr) if d > 0 else (t[c] < thr)).double().unsqueeze(1)
        for s, r in enumerate(radii):
            N = window(ones, r)
            pf, po = window(n, r) / (M * N), window(o, r) / N
            dd = pf - po
            terms = torch.stack([wp.expand_as(pf), wp * pf, wp * po, wp * pf * pf, wp * po * po, wp * dd * dd], -1)
            out[e, s] = terms.sum((1, 2))
    return out


def worker(M, E, L, H, W, reps):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip

    dev = "cuda"
    C, S = E, len(RADII)
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    w = torch.cos(torch.deg2rad(torch.linspace(-88.5, 90.0, H, device=dev)))
    w = (w / w.mean()).contiguous()
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [(k, 1 if k % 2 == 0 else -1, THRESHOLDS[k % len(THRESHOLDS)]) for k in range(E)]  # one event per channel
    desc = hip.events_desc([(c, d, v, 0) for c, d, v in ev])
    radii = (ctypes.c_int * S)(*RADII)
    f_sums, f_inv = torch.empty(E, S, L, 6, dtype=torch.float64, device=dev), torch.empty(E, L, dtype=torch.int32, device=dev)
    nb_fss = int(hip.lib.ldc_rollout_fss_workspace_bytes(M, E, S, L, H, W))
    ws_fss = torch.empty(nb_fss // 4, device=dev)
    e_cnt, e_w = torch.empty(E, L, M + 1, 2, dtype=torch.int32, device=dev), torch.empty(E, L, M + 1, 2, device=dev)
    e_inv = torch.empty(E, L, dtype=torch.int32, device=dev)
    nb_ev = int(hip.lib.ldc_rollout_events_workspace_bytes(M, E, L, H, W))
    ws_ev = torch.empty(nb_ev // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def fss():
        st = hip.lib.ldc_rollout_fss(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), None, 0, 0, None, p(w), M, C, L, H, W,
                                     ctypes.byref(desc), radii, S, p(f_sums), p(f_inv), L, 0, p(ws_fss), nb_fss, stream)
        assert st == 0, st

    def events():
        st = hip.lib.ldc_rollout_events(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), None, 0, 0, None, p(w), M, C, L, H, W,
                                        ctypes.byref(desc), p(e_cnt), p(e_w), p(e_inv), L, 0, p(ws_ev), nb_ev, stream)
        assert st == 0, st

    calls = dict(ldc_rollout_fss=fss, ldc_rollout_events=events)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything
    torch_composition(x, t, w, ev, RADII)
    torch.cuda.synchronize()
    ref = None

    def comp():
        nonlocal ref
        ref = torch_composition(x, t, w, ev, RADII)

    torch_ms = round(_events(comp), 3)  # once, for scale
    fss()
    torch.cuda.synchronize()
    torch.testing.assert_close(f_sums, ref, rtol=1e-9, atol=1e-9)  # the composition multiplies in another order and sums in torch's
    assert int(f_inv.sum()) == 0 and int(e_inv.sum()) == 0
    flush = torch.empty(FLUSH_BYTES // 4, device=dev)
    warm, cold = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            warm[k].append(_events(f))
    for _ in range(reps):
        for k, f in calls.items():
            cold[k].append(_events(f, before=flush.zero_))
    res = dict(shape=dict(M=M, E=E, C=C, S=S, L=L, H=H, W=W), radii=list(RADII), reps=reps, thresholds=[list(e) for e in ev],
               plane_set_mbytes=round(M * H * W * 4 / 1e6, 2), workspace_bytes=dict(fss=nb_fss, events=nb_ev), device=torch.cuda.get_device_name(0),
               torch_composition_once_ms=torch_ms)
    for k in calls:
        res[k] = {}
        for variant, times in (("warm", warm[k]), ("cold_l2", cold[k])):
            med = statistics.median(times)
            res[k][variant] = dict(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                                   us_per_event_and_lead=round(med * 1e3 / (E * L), 2))
    for variant in ("warm", "cold_l2"):
        res[f"fss_over_events_{variant}"] = round(res["ldc_rollout_fss"][variant]["median_ms"] / res["ldc_rollout_events"][variant]["median_ms"], 3)
    res["torch_over_fss_warm"] = round(torch_ms / res["ldc_rollout_fss"]["warm"]["median_ms"], 1)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fss_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--worker", type=int, nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(*args.worker, args.reps)
        return 0
    me = [sys.executable, os.path.abspath(__file__)]
    results = []
    for shape in SHAPES:
        st, res = _child(me + ["--reps", str(args.reps), "--worker", *map(str, shape)], str(shape))
        if st:
            return st
        results.append(res)
    _write(args.out, dict(tool="tools/fss_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
