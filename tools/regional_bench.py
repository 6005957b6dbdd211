"""Times ldc_rollout_regional (with a climatology) at R = 1 (the globe), R = 13 (the named regions), R = 32 and for the European box
alone against the pair ldc_rollout_scores + ldc_rollout_reliability on the same forecast - both unchanged, together they yield the global
versions of the same quantities - with device events around the C-ABI calls -> profiles/regional_timing.json.

    python tools/regional_bench.py [--out profiles/regional_timing.json] [--reps 20]

Every shape runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Each call gets a warmed variant (the calls alternate A, B, C, ... after 3 warm-ups of each, so drift of the
machine hits them alike) and a cold variant (a 1 GiB buffer is written before every timed call, which leaves nothing of the forecast in
L2 or in the memory-side cache).  The figure reported is the median, with the minimum and the maximum beside it.  Bytes are what the
algorithm must move, computed from the shapes (the European box: the tiles that hold one of its points).  The global region's sums must
agree with the baseline's scores before a time means anything."""
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
    from ladcast_amd.evaluate import NAMED_REGIONS, Region, region_mask
    from ladcast_amd.evaluate.evaluate_ens_gpu import row_latitudes

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    cl = 0.3 * torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    wh = np.cos(np.deg2rad(row_latitudes(H)))
    w = torch.tensor(wh / wh.mean(), dtype=torch.float32, device=dev)
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lat, lon = row_latitudes(H), np.arange(W) * (360.0 / W)
    named = list(NAMED_REGIONS.values())
    more = [Region(f"band{k}", -90.0 + 9.0 * k, -81.0 + 9.0 * k, 0.0, 360.0) for k in range(32 - len(named))]  # 19 zonal bands on top
    masks = dict(regional_R1_global=([NAMED_REGIONS["global"]]), regional_R13_named=named, regional_R32=named + more,
                 regional_R1_europe=[NAMED_REGIONS["europe"]])
    words = {k: torch.from_numpy(region_mask(v, lat, lon).view(np.int32).copy()).to(dev) for k, v in masks.items()}
    sums = {k: torch.empty(len(v), C, L, 10, dtype=torch.float64, device=dev) for k, v in masks.items()}
    counts = {k: torch.empty(len(v), C, L, 3, dtype=torch.int32, device=dev) for k, v in masks.items()}
    nb_reg = {k: int(hip.lib.ldc_rollout_regional_workspace_bytes(M, len(v), C, L, H, W)) for k, v in masks.items()}
    ws_reg = torch.empty(max(nb_reg.values()) // 4, device=dev)
    out_sc = torch.empty(5, C, L, device=dev)
    nb_sc = int(hip.lib.ldc_rollout_scores_workspace_bytes(C, L, H, W))
    ws_sc = torch.empty(nb_sc // 4, device=dev)
    out_rel, hist, hist_w, ninv = (torch.empty(3, C, L, device=dev), torch.empty(C, L, M + 1, dtype=torch.int32, device=dev),
                                   torch.empty(C, L, M + 1, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev))
    nb_rel = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    ws_rel = torch.empty(nb_rel // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def regional(k):
        st = hip.lib.ldc_rollout_regional(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(cl), cl.stride(1), cl.stride(0),
                                          p(slot), p(w), p(words[k]), len(masks[k]), M, C, L, H, W, p(sums[k]), p(counts[k]), L, 0, p(ws_reg), nb_reg[k], stream)
        assert st == 0, st

    def scores():
        st = hip.lib.ldc_rollout_scores(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(cl), cl.stride(1), cl.stride(0),
                                        p(slot), p(w), M, C, L, H, W, -1, p(out_sc), L, 0, p(ws_sc), nb_sc, stream)
        assert st == 0, st

    def reliability():
        st = hip.lib.ldc_rollout_reliability(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, -1, p(out_rel),
                                             p(hist), p(hist_w), p(ninv), L, 0, p(ws_rel), nb_rel, stream)
        assert st == 0, st

    def pair():
        scores()
        reliability()

    calls = {k: (lambda k=k: regional(k)) for k in masks}
    calls.update(ldc_rollout_scores=scores, ldc_rollout_reliability=reliability, scores_plus_reliability=pair)
    for f in calls.values():
        for _ in range(WARMUPS):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything
    P = H * W
    s = sums["regional_R1_global"][0]
    torch.testing.assert_close((s[..., 2] / P).float(), out_sc[1], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(((s[..., 4] - s[..., 5] / 2) / P).float(), out_sc[4], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close((s[..., 3] / P).float(), out_rel[1], rtol=1e-4, atol=1e-6)
    torch.testing.assert_close((s[..., 7] / torch.sqrt(s[..., 8] * s[..., 9])).float(), out_sc[0], rtol=1e-3, atol=1e-5)
    assert torch.equal(sums["regional_R13_named"][0].view(torch.int64), s.view(torch.int64)) and torch.equal(sums["regional_R32"][:13].view(torch.int64),
                                                                                                              sums["regional_R13_named"].view(torch.int64))
    assert int(counts["regional_R1_global"][..., 0].min()) == P
    flush = torch.empty(FLUSH_BYTES // 4, device=dev)
    warm, cold = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            warm[k].append(_events(f))
    for _ in range(reps):
        for k, f in calls.items():
            cold[k].append(_events(f, before=flush.zero_))
    eu = (words["regional_R1_europe"].reshape(-1) != 0).cpu().numpy()
    tiles = -(-P // 256)
    eu_tiles = int(np.add.reduceat(eu, np.arange(0, P, 256)).astype(bool).sum())
    planes = C * L
    full = lambda extra: ((M + 1 + extra) * planes * P * 4) / 1e9  # noqa: E731  (members, truth and `extra` more planes per (channel, lead))
    gb = {k: full(1) + planes * P * 4 / 1e9 for k in masks}  # + the climatology; the mask words once per plane
    gb["regional_R1_europe"] = (M + 2) * planes * eu_tiles * 256 * 4 / 1e9 + planes * P * 4 / 1e9
    gb.update(ldc_rollout_scores=full(1), ldc_rollout_reliability=full(0), scores_plus_reliability=full(1) + full(0))
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W), reps=reps, warmups=WARMUPS, forecast_mbytes=round(M * C * L * P * 4 / 1e6, 1),
               regions={k: [r.name for r in v] for k, v in masks.items()}, europe_tiles=[eu_tiles, tiles],
               workspace_bytes=dict(regional=nb_reg, scores=nb_sc, reliability=nb_rel), device=torch.cuda.get_device_name(0))
    for k in calls:
        res[k] = {}
        for variant, times in (("warm", warm[k]), ("cold_l2", cold[k])):
            med = statistics.median(times)
            res[k][variant] = dict(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                                   gbytes_per_s=round(gb[k] / (med * 1e-3), 1))
        res[k]["gbytes"] = round(gb[k], 4)
    for variant in ("warm", "cold_l2"):
        base = res["scores_plus_reliability"][variant]["median_ms"]
        res[f"regional_over_pair_{variant}"] = {k: round(res[k][variant]["median_ms"] / base, 3) for k in masks}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regional_timing.json"))
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
    _write(args.out, dict(tool="tools/regional_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
