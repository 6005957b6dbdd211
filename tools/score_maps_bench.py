"""Times ldc_rollout_score_maps (with a climatology, every channel mapped) with one lead per plane and with the four leads pooled in one
plane against the unchanged ldc_rollout_regional at R = 1 (the globe) on the same forecast, with device events around the C-ABI calls
-> profiles/score_maps_timing.json.

    python tools/score_maps_bench.py [--out profiles/score_maps_timing.json] [--reps 20]

The protocol is that of tools/regional_bench.py: every shape runs in a child process of its own under a time limit; the parent never
opens the device, and stops at the first child that fails or runs out of time.  Each call gets a warmed variant (the calls alternate
A, B, C after 3 warm-ups of each, so drift of the machine hits them alike) and a cold variant (a 1 GiB buffer is written before every
timed call, which leaves nothing of the forecast or the maps in L2 or in the memory-side cache).  The figure reported is the median,
with the minimum and the maximum beside it.  Bytes are what the algorithm must move, computed from the shapes: members, truth and
climatology once, and for the maps one read and one write of the 76 bytes of every (channel, plane, point) a call addresses.
`over_byte_model`: the time of a map call over (the regional call's time x the ratio of their bytes).  The maps of one call, pooled over
the globe with the latitude weights, must agree with the regional call's sums before a time means anything."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 84, 4, 120, 240), (10, 84, 4, 120, 240))  # M, C, L, H, W
STEP_TIMEOUT_S = 300
FLUSH_BYTES = 1 << 30
WARMUPS = 3


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


def worker(M, C, L, H, W, reps):
    import ctypes

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip
    from ladcast_amd.evaluate.evaluate_ens_gpu import row_latitudes

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    cl = 0.3 * torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    wh = np.cos(np.deg2rad(row_latitudes(H)))
    w = torch.tensor(wh / wh.mean(), dtype=torch.float32, device=dev)
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    chan = torch.arange(C, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = H * W
    planes = dict(maps_plane_per_lead=list(range(L)), maps_leads_in_one_plane=[0] * L)
    n_planes = {k: max(v) + 1 for k, v in planes.items()}
    pol = {k: torch.tensor(v, dtype=torch.int32, device=dev) for k, v in planes.items()}
    sums = {k: torch.zeros(C, n_planes[k], 8, P, dtype=torch.float64, device=dev) for k in planes}
    counts = {k: torch.zeros(C, n_planes[k], 3, P, dtype=torch.int32, device=dev) for k in planes}
    map_bytes = {k: int(hip.lib.ldc_score_maps_bytes(C, n_planes[k], H, W)) for k in planes}
    words = torch.ones(P, dtype=torch.int32, device=dev)
    r_sums, r_counts = torch.empty(1, C, L, 10, dtype=torch.float64, device=dev), torch.empty(1, C, L, 3, dtype=torch.int32, device=dev)
    nb_reg = int(hip.lib.ldc_rollout_regional_workspace_bytes(M, 1, C, L, H, W))
    ws_reg = torch.empty(nb_reg // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def maps(k):
        st = hip.lib.ldc_rollout_score_maps(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(cl), cl.stride(1), cl.stride(0),
                                            p(slot), p(chan), C, p(pol[k]), n_planes[k], M, C, L, H, W, p(sums[k]), p(counts[k]), stream)
        assert st == 0, st

    def regional():
        st = hip.lib.ldc_rollout_regional(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(cl), cl.stride(1), cl.stride(0),
                                          p(slot), p(w), p(words), 1, M, C, L, H, W, p(r_sums), p(r_counts), L, 0, p(ws_reg), nb_reg, stream)
        assert st == 0, st

    # results must agree before a time means anything: one call into the zeroed maps, pooled over the globe
    regional()
    for k in planes:
        maps(k)
    torch.cuda.synchronize()
    wp = w.double().repeat_interleave(W)
    s = sums["maps_plane_per_lead"]
    pooled = torch.stack([(wp * s[:, :, k]).sum(-1) for k in range(8)], -1)  # (C, L, 8)
    torch.testing.assert_close(pooled[..., :5], r_sums[0][..., 1:6], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(pooled[..., 5:], r_sums[0][..., 7:], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(sums["maps_leads_in_one_plane"][:, 0], s.sum(1), rtol=1e-12, atol=1e-12)
    assert int(counts["maps_plane_per_lead"][:, :, 0].min()) == 1 and int(counts["maps_leads_in_one_plane"][:, :, 2].min()) == L
    assert int(r_counts[..., 0].min()) == P
    calls = {k: (lambda k=k: maps(k)) for k in planes}
    calls["regional_R1_global"] = regional
    for f in calls.values():
        for _ in range(WARMUPS):
            f()
    torch.cuda.synchronize()
    flush = torch.empty(FLUSH_BYTES // 4, device=dev)
    warm, cold = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            warm[k].append(_events(f))
    for _ in range(reps):
        for k, f in calls.items():
            cold[k].append(_events(f, before=flush.zero_))
    read = (M + 2) * C * L * P * 4 / 1e9  # members, truth, climatology
    gb = {k: read + 2 * map_bytes[k] / 1e9 for k in planes}
    gb["regional_R1_global"] = read + C * L * P * 4 / 1e9  # + the mask words once per plane
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), reps=reps, warmups=WARMUPS, forecast_mbytes=round(M * C * L * P * 4 / 1e6, 1),
               map_bytes=map_bytes, planes=planes, device=torch.cuda.get_device_name(0))
    for k in calls:
        res[k] = {}
        for variant, times in (("warm", warm[k]), ("cold_l2", cold[k])):
            med = statistics.median(times)
            res[k][variant] = dict(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                                   gbytes_per_s=round(gb[k] / (med * 1e-3), 1))
        res[k]["gbytes"] = round(gb[k], 4)
    for variant in ("warm", "cold_l2"):
        base = res["regional_R1_global"][variant]["median_ms"]
        res[f"maps_over_regional_{variant}"] = {k: round(res[k][variant]["median_ms"] / base, 3) for k in planes}
        res[f"over_byte_model_{variant}"] = {k: round(res[k][variant]["median_ms"] / (base * gb[k] / gb["regional_R1_global"]), 3) for k in planes}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_maps_timing.json"))
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
    _write(args.out, dict(tool="tools/score_maps_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
