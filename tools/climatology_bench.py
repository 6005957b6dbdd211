"""`Climatology.update` (ldc_climatology_accumulate) and `Climatology.finish` (ldc_climatology_smooth) on one channel block of the real
grid - 12 channels x 121 x 240, 366 x 4 slots, 6.1 GB of state - each next to a device-to-device copy that moves the same number of
bytes, timed in the same run with HIP events, the kernel and its copy alternated call by call.  No pass threshold: the claim the numbers
support is that the device side is not the bottleneck next to reading a multi-decade dataset from disk.

    python tools/climatology_bench.py [TIMING.json]          (default profiles/climatology_timing.json)"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ladcast_amd.preprocess import Climatology  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "climatology_timing.json")
C, H, W, B = 12, 121, 240, 32
N_DAYS, N_HOURS = 366, 4
ROUNDS = 7
HBM_SPEC_GBPS = 8000.0


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    return s, e


def summarise(pairs, nbytes):
    us = [s.elapsed_time(e) * 1e3 for s, e in pairs]
    med = statistics.median(us)
    return dict(median_us=round(med, 1), min_us=round(min(us), 1), max_us=round(max(us), 1), spread_pct=round(100 * (max(us) - min(us)) / med, 2),
                bytes=nbytes, GBps=round(nbytes / (med * 1e-6) / 1e9, 1), calls=len(us))


def copy_of(nbytes):
    """a device-to-device copy that moves nbytes in all: nbytes / 2 read, nbytes / 2 written"""
    n = nbytes // 2 // 16 * 4
    src, dst = torch.empty(n, device="cuda", dtype=torch.float32).normal_(), torch.empty(n, device="cuda", dtype=torch.float32)
    return lambda: dst.copy_(src)


def main():
    points = C * H * W
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(B, C, H, W, device="cuda", generator=g) * 3 + 280
    x[:, C - 2][:, : H // 3] = float("nan")  # an SST-like channel: a third of its rows are land
    valid = int((~torch.isnan(x)).sum())
    clim = Climatology(C, H, W, "cuda", n_days=N_DAYS)
    n_slots = N_DAYS * N_HOURS

    # update: 32 consecutive 6-hourly frames = 32 distinct slots; the slots advance from call to call, so nothing is cache-resident.
    # bytes: every value read (4), and for the non-NaN ones sum read + written (16) and count read + written (8)
    upd_bytes = 4 * B * points + 24 * valid
    copy_u = copy_of(upd_bytes)
    calls = [[(k * B + i) % n_slots for i in range(B)] for k in range(2 * ROUNDS * 6 + 6)]
    for k in range(3):
        clim.update(x, calls[k])
        copy_u()
    torch.cuda.synchronize()
    upd, cpu_ = [], []
    k = 3
    for _ in range(ROUNDS * 6):
        upd.append(timed(lambda: clim.update(x, calls[k])))
        cpu_.append(timed(copy_u))
        k += 1
    torch.cuda.synchronize()
    res = dict(update=summarise(upd, upd_bytes), update_copy=summarise(cpu_, upd_bytes))
    res["update"]["share_of_copy_rate"] = round(res["update_copy"]["median_us"] / res["update"]["median_us"], 3)
    print(json.dumps({k_: res[k_] for k_ in ("update", "update_copy")}), flush=True)
    del copy_u

    # finish: sum (8) and count (4) read once, out (4) written once per table entry
    fin_bytes = 16 * n_slots * points
    copy_f = copy_of(fin_bytes)
    out = clim.finish()
    n_empty = clim.n_empty().tolist()
    copy_f()
    torch.cuda.synchronize()
    clim.finish(window_days=1)
    fin, fin1, cpf = [], [], []
    for _ in range(ROUNDS):
        fin.append(timed(lambda: clim.finish()))
        cpf.append(timed(copy_f))
        fin1.append(timed(lambda: clim.finish(window_days=1)))  # the same traffic with one multiply-add per output: staging and stores alone
    torch.cuda.synchronize()
    res["finish"], res["finish_copy"], res["finish_window_1"] = summarise(fin, fin_bytes), summarise(cpf, fin_bytes), summarise(fin1, fin_bytes)
    res["finish"]["share_of_copy_rate"] = round(res["finish_copy"]["median_us"] / res["finish"]["median_us"], 3)
    res["finish_window_1"]["share_of_copy_rate"] = round(res["finish_copy"]["median_us"] / res["finish_window_1"]["median_us"], 3)
    res["finish"]["fp64_fma_per_call"] = 2 * 61 * n_slots * points
    res["finish"]["n_empty"] = n_empty
    res["finish"]["nan_outputs"] = int(torch.isnan(out).sum())
    print(json.dumps({k_: res[k_] for k_ in ("finish", "finish_copy", "finish_window_1")}), flush=True)

    doc = dict(method=f"HIP events around each call, the kernel and a device-to-device copy of the same total bytes (half read, half written) alternated call "
                      f"by call; update: {ROUNDS * 6} calls of {B} frames after 3 warm-ups, the slots advancing by {B} per call (state and frames exceed the "
                      f"caches); finish: {ROUNDS} calls (window 61, sigma 10) after 1 warm-up; median, min, max; spread = (max - min) / median; HBM3E peak "
                      f"{HBM_SPEC_GBPS:.0f} GB/s; share_of_copy_rate = copy time / kernel time",
               device=torch.cuda.get_device_name(0), shape=dict(C=C, H=H, W=W, B=B, n_days=N_DAYS, n_hours=N_HOURS, state_bytes=12 * n_slots * points), **res)
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
