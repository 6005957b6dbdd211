"""ldc_validation_scores against ldc_rollout_scores (no climatology) of a baseline build of the library (the commit before the entry point
existed), and the unchanged entry points in both builds, on the same input in one process: HIP-event brackets of benchlib/kernel_timer.py,
variants alternated launch by launch, ROUNDS rounds of REPS launches each.

    python tools/validation_scores_bench.py BASELINE_LIB.so [OUT.json]      (shapes: 10 x 84 x 4 x 120 x 240 and 50 x 84 x 2 x 120 x 240)"""
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchlib.kernel_timer import KernelTimer  # noqa: E402
from ladcast_amd import hip  # noqa: E402

ROUNDS, REPS = 9, 20
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
parent = ctypes.CDLL(os.path.abspath(sys.argv[1]))
OUT = sys.argv[2] if len(sys.argv) > 2 else "validation_scores_timing.json"
for lib in (parent, hip.lib):
    for name in ("ldc_rollout_scores", "ldc_ensemble_scores", "ldc_rollout_scores_workspace_bytes", "ldc_ensemble_scores_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = hip.SIGNATURES[name]
assert not hasattr(parent, "ldc_validation_scores")
p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731


def bracket(timer, name, work, fn):
    """a HIP-event pair around one call, recorded where KernelTimer keeps its own brackets (`records`: name -> (start, end, work)), so that
    `KernelTimer.summary()` does the arithmetic"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    timer.records.setdefault(name, []).append((s, e, work))


def run_case(M, C, Lr, H, W, out):
    g = torch.Generator(device="cuda").manual_seed(3)
    fc = torch.randn(M, C, Lr, H, W, device="cuda", generator=g) * 2 + 0.5
    tr = torch.randn(C, Lr, H, W, device="cuda", generator=g)
    w = torch.rand(H, device="cuda", generator=g) + 0.5
    slots = torch.arange(Lr, dtype=torch.int32, device="cuda")
    nbytes = max(int(hip.lib.ldc_validation_scores_workspace_bytes(C, Lr, H, W)), int(hip.lib.ldc_rollout_scores_workspace_bytes(C, Lr, H, W)),
                 int(parent.ldc_rollout_scores_workspace_bytes(C, Lr, H, W)), int(hip.lib.ldc_ensemble_scores_workspace_bytes(C, H, W)))
    ws = torch.empty(nbytes // 4, device="cuda")  # one scratch block, large enough for every entry point of both builds
    o5, o5p, o3, oe, oep = (torch.full((5, C, Lr), float("nan"), device="cuda"), torch.full((5, C, Lr), float("nan"), device="cuda"),
                            torch.full((3, C, Lr), float("nan"), device="cuda"), torch.empty(5, C, device="cuda"), torch.empty(5, C, device="cuda"))
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def rollout(lib, o):
        st = lib.ldc_rollout_scores(p(fc), fc.stride(0), fc.stride(2), fc.stride(1), None, None, 1.0, p(tr), tr.stride(1), tr.stride(0), p(slots), None, 0, 0,
                                    None, p(w), M, C, Lr, H, W, -1, p(o), Lr, 0, p(ws), ws.numel() * 4, stream())
        assert st == 0, st

    def validation():
        st = hip.lib.ldc_validation_scores(p(fc), fc.stride(0), fc.stride(2), fc.stride(1), None, None, 1.0, p(tr), tr.stride(1), tr.stride(0), p(slots),
                                           p(w), M, C, Lr, H, W, p(o3), Lr, 0, p(ws), ws.numel() * 4, stream())
        assert st == 0, st

    f0, t0 = fc[:, :, 0], tr[:, 0]

    def ensemble(lib, o):  # one lead time: the third entry point that shares the body
        st = lib.ldc_ensemble_scores(p(f0), f0.stride(0), f0.stride(1), p(t0), t0.stride(0), None, 0, p(w), M, C, H, W, -1, p(o), None, None, p(ws),
                                     ws.numel() * 4, stream())
        assert st == 0, st

    full, one = 4.0 * M * C * Lr * H * W, 4.0 * M * C * H * W
    variants = [("rollout_scores[parent]", full, lambda: rollout(parent, o5p)), ("rollout_scores[this]", full, lambda: rollout(hip.lib, o5)),
                ("validation_scores[this]", full, validation), ("ensemble_scores[parent]", one, lambda: ensemble(parent, oep)),
                ("ensemble_scores[this]", one, lambda: ensemble(hip.lib, oe))]
    for _ in range(3):  # warm-up: code objects, clocks
        for _, _, fn in variants:
            fn()
    torch.cuda.synchronize()
    # the unchanged entry points compute what the parent computed, and the new one shares their bits
    same = lambda a, b: torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) and torch.equal(torch.isnan(a), torch.isnan(b))  # noqa: E731
    assert same(o5, o5p) and same(oe, oep), "unchanged entry points differ from the parent build"
    assert same(o3[0], o5[1]) and same(o3[2], o5[4]) and bool(torch.isfinite(o3).all())
    timer, rounds = KernelTimer(), {n: [] for n, _, _ in variants}
    for _ in range(ROUNDS):
        timer.clear()
        for r in range(REPS):  # the order rotates: each variant follows each other one equally often (the 256 MB last-level cache keeps
            for n, work, fn in variants[r % len(variants):] + variants[: r % len(variants)]:  # part of what the previous launch read)
                bracket(timer, n, work, fn)
        torch.cuda.synchronize()
        for n, s in timer.summary().items():
            rounds[n].append(s["avg_us"])
    res = {}
    for n, work, _ in variants:
        v = rounds[n]
        med = statistics.median(v)
        res[n] = dict(median_us=round(med, 2), min_us=round(min(v), 2), max_us=round(max(v), 2), spread_pct=round(100 * (max(v) - min(v)) / med, 2),
                      bytes=work, GBps=round(work / (med * 1e-6) / 1e9, 1))
    base = res["rollout_scores[parent]"]
    res["validation_over_parent_rollout"] = round(res["validation_scores[this]"]["median_us"] / base["median_us"], 4)
    res["rollout_this_over_parent"] = round(res["rollout_scores[this]"]["median_us"] / base["median_us"], 4)
    res["ensemble_this_over_parent"] = round(res["ensemble_scores[this]"]["median_us"] / res["ensemble_scores[parent]"]["median_us"], 4)
    out[f"{M}x{C}x{Lr}x{H}x{W}"] = res
    print(json.dumps({f"{M}x{C}x{Lr}x{H}x{W}": res}), flush=True)


out = dict(method=f"HIP events around each C-ABI call (main + finish kernel), variants alternated launch by launch in rotating order, {ROUNDS} rounds x {REPS} launches; "
                  "per-round averages: median, min, max; spread = (max - min) / median", device=torch.cuda.get_device_name(0))
for shape in ((10, 84, 4, 120, 240), (50, 84, 2, 120, 240)):
    run_case(*shape, out)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
json.dump(out, open(OUT, "w"), indent=1)
