"""Times one ldc_rollout_energy call on a decode batch beside the DC-AE decoder call that produced the batch -> profiles/energy_timing.json.

    python tools/energy_bench.py [--out profiles/energy_timing.json] [--reps 20] [--members 50] [--leads 4]

The batch is what evaluate_ens_gpu scores with `--decode_batch_frames M * L`: M x L latents (84 x 15 x 30) go through the DC_AE_84 decoder
(random-init, seed 1234) in one call, and the energy score reads the decoder's output where it lies - frame-major, its 84
channels, the inverse normalisation fused.  Device events around the calls; the decoder is timed in the bf16x3 mode (the rollout's) and
in exact fp32, the energy call without groups, with three groups, and with the dist2 matrix written, each warm (the calls alternate, so
drift of the machine hits them alike) and cold (a 1 GiB buffer is written before every timed call, which leaves nothing of the batch in
L2 or in the memory-side cache).  Medians, with the minimum, the maximum and every sample beside them.  Pair terms and bytes are what the
kernel's tiling computes and moves, counted from the shapes.  One (channel, lead time) is checked against a float64 computation in torch
before a time means anything.  The work runs in a child process under a time limit; the parent never opens the device."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 420
FLUSH_BYTES = 1 << 30
WARMUPS = 3
C, H, W = 84, 120, 240
GROUPS = ((7, 23, 80), (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12), (80, 81, 82, 83))  # three overlapping groups of channels


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


def _stats(times):
    return dict(median_ms=round(statistics.median(times), 4), min_ms=round(min(times), 4), max_ms=round(max(times), 4),
                samples_ms=[round(t, 4) for t in times])


def worker(M, L, reps):
    import ctypes

    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from benchlib.configs import CONFIG_DCAE_84
    from ladcast_amd import hip
    from ladcast_amd.evaluate.evaluate_ens_gpu import row_latitudes
    from ladcast_amd.models import AutoencoderDC

    dev = "cuda"
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(CONFIG_DCAE_84).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(M * 1000 + L)
    z = torch.randn(L * M, CONFIG_DCAE_84["latent_channels"], H // 8, W // 8, device=dev, generator=g)  # lead-major, then member
    decode = {}
    with torch.no_grad():
        for prec in ("bf16x3", "fp32"):
            model.set_gemm_precision(prec)
            y = model.decode(z).sample
            torch.cuda.synchronize()
            decode[prec] = _stats([_events(lambda: model.decode(z)) for _ in range(3)])
        model.set_gemm_precision("bf16x3")
        y = model.decode(z).sample  # (L * M, C, H, W), still normalised
    Cd = y.shape[1]
    assert y.shape == (L * M, Cd, H, W) and Cd >= C and y.is_contiguous()
    frames = y.reshape(L, M, Cd, H, W)
    ls, ms, cs = frames.stride(0), frames.stride(1), frames.stride(2)
    mean, std = torch.randn(C, device=dev, generator=g) * 10, torch.rand(C, device=dev, generator=g) * 5 + 0.5
    t = (frames[:, :, :C].mean(1) + 0.1 * torch.randn(L, C, H, W, device=dev, generator=g)) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)
    t = t.permute(1, 0, 2, 3).contiguous()  # (C, L, H, W), physical units
    wh = np.cos(np.deg2rad(row_latitudes(H)))
    w = torch.tensor(wh / wh.mean(), dtype=torch.float32, device=dev)
    slot = torch.arange(L, dtype=torch.int32, device=dev)
    words = [0] * C
    for k, chans in enumerate(GROUPS):
        for c in chans:
            words[c] |= 1 << k
    gmask = torch.tensor(words, dtype=torch.int32, device=dev)
    inv_s2 = (1.0 / (std.double() * std.double())).contiguous()
    G, N = len(GROUPS), M + 1
    energy, group = torch.empty(5, C, L, dtype=torch.float64, device=dev), torch.empty(5, G, L, dtype=torch.float64, device=dev)
    ninv, dist2 = torch.empty(C, L, dtype=torch.int32, device=dev), torch.empty(C, L, N, N, dtype=torch.float64, device=dev)
    nbytes = int(hip.lib.ldc_rollout_energy_workspace_bytes(M, C, G, L, H, W))
    ws = torch.empty(nbytes // 4, device=dev)
    p = lambda a: None if a is None else ctypes.c_void_p(a.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(groups, d2):
        st = hip.lib.ldc_rollout_energy(p(frames), ms, ls, cs, p(mean), p(std), 1.0, p(t), t.stride(1), t.stride(0), p(slot), p(w),
                                        p(gmask) if groups else None, p(inv_s2) if groups else None, G if groups else 0, M, C, L, H, W, p(energy),
                                        p(group) if groups else None, p(ninv), p(dist2) if d2 else None, L, 0, p(ws), nbytes, stream)
        assert st == 0, st

    calls = dict(energy=lambda: call(False, False), energy_3_groups=lambda: call(True, False), energy_dist2=lambda: call(False, True))
    for f in calls.values():
        for _ in range(WARMUPS):
            f()
    call(True, True)
    torch.cuda.synchronize()
    # one (channel, lead time) in float64 before a time means anything
    c0, l0 = 7, L - 1
    yy = torch.cat([(frames[l0, :, c0] * std[c0] + mean[c0]).double(), t[c0, l0].double().unsqueeze(0)]).reshape(N, -1)  # fp32 inverse normalisation
    wp = w.double().repeat_interleave(W)
    d = torch.cdist(yy * wp.sqrt(), yy * wp.sqrt()) ** 2
    torch.testing.assert_close(dist2[c0, l0], d, rtol=1e-5, atol=1e-9 * float(d.max()))
    nm = (d / wp.sum()).sqrt()
    skill, spread = nm[:M, M].sum() / M, nm[:M, :M].sum() / (M * M)
    torch.testing.assert_close(energy[2, c0, l0], skill, rtol=1e-5, atol=0)
    torch.testing.assert_close(energy[0, c0, l0], skill - 0.5 * spread, rtol=1e-4, atol=0)
    assert int(ninv.abs().sum()) == 0 and bool(torch.isfinite(group).all())
    flush = torch.empty(FLUSH_BYTES // 4, device=dev)
    warm, cold = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(reps):
        for k, f in calls.items():
            warm[k].append(_events(f))
    for _ in range(reps):
        for k, f in calls.items():
            cold[k].append(_events(f, before=flush.zero_))
    P = H * W
    NB = (N + 3) // 4
    NBP = NB * (NB + 1) // 2
    terms = C * L * P * NBP * 16  # pair terms the upper-triangle blocks compute (each: fp32 subtract, fp32 multiply, convert, fp64 fused multiply-add)
    gbytes = (N * C * L * P * 4 * -(-NBP // 256)) / 1e9  # members and truth, once per block group
    res = dict(shape=dict(M=M, C=C, L=L, H=H, W=W, decoded_channels=Cd), reps=reps, warmups=WARMUPS, device=torch.cuda.get_device_name(0),
               batch_mbytes=round(L * M * Cd * P * 4 / 1e6, 1), workspace_bytes=nbytes, pair_terms=terms, gbytes=round(gbytes, 4),
               decode={k: dict(v, frames=L * M, note="one decoder call for the whole batch, eager launches") for k, v in decode.items()})
    for k in calls:
        res[k] = dict(warm=_stats(warm[k]), cold_l2=_stats(cold[k]))
        res[k]["gterms_per_s_warm"] = round(terms / (res[k]["warm"]["median_ms"] * 1e-3) / 1e9, 1)
    for prec in decode:
        res[f"energy_over_decode_{prec}"] = round(res["energy"]["warm"]["median_ms"] / decode[prec]["median_ms"], 5)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--leads", type=int, default=4)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker(args.members, args.leads, args.reps)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--members", str(args.members), "--leads", str(args.leads), "--worker"]
    st, res = _child(cmd, f"M={args.members} L={args.leads}")
    if st:
        return st
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(tool="tools/energy_bench.py", results=[res]), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
