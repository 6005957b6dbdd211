"""Times ldc_rollout_events (8 events) against ldc_rollout_reliability on the same forecast (reliability.hip reads the same members and
truth once per plane set and walks half as many bins: the project's yardstick per (plane set, lead time)), with device events around
the C-ABI calls -> profiles/events_timing.json.

    python tools/events_bench.py [--out profiles/events_timing.json] [--reps 20]

Every shape runs in a child process of its own under a time limit; the parent never opens the device, and stops at the first child that
fails or runs out of time.  Three calls are timed: `events_8_channels` (8 events, one per channel: 8 plane sets, as reliability's C = 8),
`events_2_channels` (the same 8 events on 2 channels, 4 thresholds each: a plane set is read 4 times, 3 of them from cache) and
`ldc_rollout_reliability` (C = 8).  Each gets a warmed variant (the calls alternate A, B, C, A, B, C, ... after a warm-up of each, so
drift of the machine hits them alike) and a cold variant (a 1 GiB buffer is written before every timed call, which leaves nothing of
the forecast in L2 or in the memory-side cache).  The figure reported is the median, with the minimum and the maximum beside it.  Bytes
are what the algorithm must move, computed from the shapes.  A torch composition of the same histograms ((x > thr).sum(0), bincount with
weights) runs once after a warm-up, for scale; its counts must equal the kernel's before a time means anything."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((50, 8, 4, 120, 240), (10, 8, 4, 120, 240))  # M, E (= C of the reliability call), L, H, W
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


def torch_composition(x, t, w, events):
    """the same histograms from torch ops on the device; x (M, C, L, H, W), t (C, L, H, W), w (H,) -> (count, weight) (E, L, M + 1, 2)"""
    import torch

    M, C, L, H, W = x.shape
    wp = w.view(H, 1).expand(H, W).reshape(-1)
    cnt = torch.zeros(len(events), L, 2 * (M + 1), dtype=torch.int64, device=x.device)
    wsum = torch.zeros(len(events), L, 2 * (M + 1), dtype=torch.float32, device=x.device)
    for e, (c, d, thr) in enumerate(events):
        n = ((x[:, c] > thr) if d > 0 else (x[:, c] < thr)).sum(0)
        o = ((t[c] > thr) if d > 0 else (t[c] < thr)).long()
        key = (2 * n + o).reshape(L, -1)
        for l in range(L):
            cnt[e, l] = torch.bincount(key[l], minlength=2 * (M + 1))
            wsum[e, l] = torch.bincount(key[l], weights=wp, minlength=2 * (M + 1))
    return cnt.reshape(len(events), L, M + 1, 2), wsum.reshape(len(events), L, M + 1, 2)


def worker(M, E, L, H, W, reps):
    import ctypes

    import torch

    sys.path.insert(0, ROOT)
    from ladcast_amd import hip

    dev = "cuda"
    C = E
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    t = torch.randn(C, L, H, W, device=dev, generator=g)
    x = t.unsqueeze(0) + 0.5 * torch.randn(M, C, L, H, W, device=dev, generator=g)
    w = torch.cos(torch.deg2rad(torch.linspace(-88.5, 90.0, H, device=dev)))
    w = (w / w.mean()).contiguous()
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dirs = [1 if k % 2 == 0 else -1 for k in range(E)]
    ev8 = [(k, dirs[k], THRESHOLDS[k % len(THRESHOLDS)]) for k in range(E)]  # one event per channel
    ev2 = [(k // (E // 2), dirs[k], THRESHOLDS[k % len(THRESHOLDS)]) for k in range(E)]  # the same events on channels 0 and 1
    desc8, desc2 = (hip.events_desc([(c, d, v, 0) for c, d, v in ev]) for ev in (ev8, ev2))
    e_cnt, e_w = torch.empty(E, L, M + 1, 2, dtype=torch.int32, device=dev), torch.empty(E, L, M + 1, 2, device=dev)
    e_inv = torch.empty(E, L, dtype=torch.int32, device=dev)
    nb_ev = int(hip.lib.ldc_rollout_events_workspace_bytes(M, E, L, H, W))
    ws_ev = torch.empty(nb_ev // 4, device=dev)
    out, hist, hist_w, ninv = (torch.empty(3, C, L, device=dev), torch.empty(C, L, M + 1, dtype=torch.int32, device=dev),
                               torch.empty(C, L, M + 1, device=dev), torch.empty(C, L, dtype=torch.int32, device=dev))
    nb_rel = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    ws_rel = torch.empty(nb_rel // 4, device=dev)
    ms, cs, ls = x.stride(0), x.stride(1), x.stride(2)

    def events(desc):
        st = hip.lib.ldc_rollout_events(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), None, 0, 0, None, p(w), M, C, L, H, W,
                                        ctypes.byref(desc), p(e_cnt), p(e_w), p(e_inv), L, 0, p(ws_ev), nb_ev, stream)
        assert st == 0, st

    def reliability():
        st = hip.lib.ldc_rollout_reliability(p(x), ms, ls, cs, None, None, 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w), M, C, L, H, W, -1, p(out),
                                             p(hist), p(hist_w), p(ninv), L, 0, p(ws_rel), nb_rel, stream)
        assert st == 0, st

    calls = dict(events_8_channels=lambda: events(desc8), events_2_channels=lambda: events(desc2), ldc_rollout_reliability=reliability)
    for f in calls.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    # results must agree before a time means anything: the counts are integers and must be equal
    torch_composition(x, t, w, ev2)
    torch.cuda.synchronize()
    torch_ms = {}
    for name, ev, desc in (("events_8_channels", ev8, desc8), ("events_2_channels", ev2, desc2)):
        events(desc)
        r_cnt, r_w = None, None

        def comp():
            nonlocal r_cnt, r_w
            r_cnt, r_w = torch_composition(x, t, w, ev)

        torch_ms[name] = round(_events(comp), 3)  # once, for scale
        assert torch.equal(e_cnt.long(), r_cnt), name
        torch.testing.assert_close(e_w, r_w, rtol=1e-4, atol=1e-4)
        assert int(e_inv.sum()) == 0
    flush = torch.empty(FLUSH_BYTES // 4, device=dev)
    warm, cold = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            warm[k].append(_events(f))
    for _ in range(reps):
        for k, f in calls.items():
            cold[k].append(_events(f, before=flush.zero_))
    points = L * H * W
    read = (M + 1) * E * points * 4  # members and truth of E plane sets, once each
    written_ev, written_rel = (e_cnt.numel() + e_w.numel() + e_inv.numel()) * 4, (out.numel() + hist.numel() + hist_w.numel() + ninv.numel()) * 4
    gb = dict(events_8_channels=(read + written_ev) / 1e9, events_2_channels=((M + 1) * 2 * points * 4 + written_ev) / 1e9,
              ldc_rollout_reliability=(read + written_rel) / 1e9)
    res = dict(shape=dict(M=M, E=E, C=C, L=L, H=H, W=W), reps=reps, thresholds=[list(e) for e in ev8], plane_set_mbytes=round(M * H * W * 4 / 1e6, 2),
               workspace_bytes=dict(events=nb_ev, reliability=nb_rel), device=torch.cuda.get_device_name(0),
               torch_composition_once_ms=torch_ms)
    for k in calls:
        res[k] = {}
        for variant, times in (("warm", warm[k]), ("cold_l2", cold[k])):
            med = statistics.median(times)
            res[k][variant] = dict(median_ms=round(med, 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                                   us_per_plane_set_and_lead=round(med * 1e3 / (E * L), 2), gbytes_per_s=round(gb[k] / (med * 1e-3), 1))
        res[k]["gbytes"] = round(gb[k], 4)
    for variant in ("warm", "cold_l2"):
        rel = res["ldc_rollout_reliability"][variant]["median_ms"]
        res[f"events_over_reliability_{variant}"] = {k: round(res[k][variant]["median_ms"] / rel, 3) for k in ("events_8_channels", "events_2_channels")}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_timing.json"))
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
    _write(args.out, dict(tool="tools/events_bench.py", results=results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
