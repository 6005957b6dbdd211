"""Timing of the cyclone tracker at the reference's size: 50 members x 28 six-hour steps (7 days), plus the ensemble mean.

    python tools/track_timing.py [--members 50] [--steps 28] [--out FILE]

Prints one JSON line:
  * tracker_ms: one ldc_track_storms launch over 51 tracks (members + mean) on decoded-like fields resident in HBM (median of 20);
  * latent_flow_s[mode]: track_latent_ensemble from a latent_YYYYMMDDHH.npy on the full-size DC-AE (random weights) in the fp32 and
    bf16x3 modes: file read, decode of members x (steps + 1) frames, gather, mean and tracker launch (one run after a warm-up run);
  * oracle_cpu_s: the same 51 tracks by tests/track_oracle.py (numpy) on the host, for scale.
Not called by bench.py."""
import argparse
import json
import os
import sys
import tempfile
import time
import warnings
from datetime import datetime

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_fields(E, F, seed=0):
    """(E, F, H, W) MSLP-like fields on the device: 101000 Pa background, one moving low per member, noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.arange(-88.5, 90 + 1e-6, 1.5, device="cuda", dtype=torch.float64)[:, None]
    lon = torch.arange(0, 358.5 + 1e-6, 1.5, device="cuda", dtype=torch.float64)[None, :]
    out = torch.empty(E, F, lat.numel(), lon.numel(), device="cuda", dtype=torch.float32)
    for e in range(E):
        for t in range(F):
            c_la, c_lo = 15.0 + 0.5 * t + 0.05 * e, (140.0 - 1.2 * t - 0.1 * e) % 360
            d2 = ((lat - c_la) ** 2 + ((lon - c_lo + 180) % 360 - 180) ** 2) / 9.0
            out[e, t] = (101000.0 - 2500.0 * torch.exp(-0.5 * d2)).float()
    out += torch.randn(out.shape, generator=g, device="cuda") * 20.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--steps", type=int, default=28)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    from ladcast_amd.evaluate.track import _track_launch, round_to_grid, track_latent_ensemble
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.io import save_latent_npy
    from oracle.dcae import CONFIG_DCAE_84
    from tests import track_oracle as O

    E, S = args.members, args.steps
    F = S + 1
    start = round_to_grid(15.2), round_to_grid(140.3)
    res = {"members": E, "steps": S, "tracks": E + 1, "device": torch.cuda.get_device_name(0)}

    # 1) the tracker launch alone
    f = synthetic_fields(E + 1, F)
    kw = dict(track_stride=F * f.shape[-2] * f.shape[-1], frame_stride=f.shape[-2] * f.shape[-1], mslp_off=0, z_off=None, lsm=None,
              n_tracks=E + 1, n_frames=F, n_steps=S, lat0=[start[0]] * (E + 1), lon0=[start[1]] * (E + 1), inner_box_sizes=[7, 4, 1],
              enforce_msl=True, lat=None, lon=None)
    lats, lons, _ = _track_launch(f, **kw)  # warm-up (module load, grid upload)
    times = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _track_launch(f, **kw)  # includes the tiny uploads and the read-back of the tracks
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    res["tracker_ms_with_host_io"] = round(float(np.median(times)), 3)
    from ladcast_amd import hip
    from ladcast_amd.evaluate.track import _f64, _grid

    glat, glon = _grid(f.device, None, None)
    lat0, lon0 = _f64(kw["lat0"], f.device), _f64(kw["lon0"], f.device)
    ol = torch.empty(E + 1, F, dtype=torch.float64, device="cuda")
    oo, oc = torch.empty_like(ol), torch.empty(E + 1, S, dtype=torch.int32, device="cuda")
    times = []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip.track_storms(f, glat, glon, lat0, lon0, ol, oo, oc, track_stride=kw["track_stride"], frame_stride=kw["frame_stride"], mslp_off=0,
                         z_off=-1, lsm=None, H=120, W=240, n_tracks=E + 1, n_steps=S, inner_box_sizes=[7, 4, 1], enforce_msl=True)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    res["tracker_ms"] = round(float(np.median(times)), 3)
    assert np.array_equal(ol.cpu().numpy(), lats) and np.array_equal(oo.cpu().numpy(), lons)

    # 2) the CPU restatement on the same fields, for scale
    host = f.cpu().numpy()
    t0 = time.perf_counter()
    for e in range(E + 1):
        trk = O.track_first_n_steps(datetime(2018, 10, 1), start[0], start[1], host[e], S)
        assert np.array_equal(np.array([(a, b) for _, a, b in trk]), np.stack([lats[e], lons[e]], 1)), e
    res["oracle_cpu_s"] = round(time.perf_counter() - t0, 2)
    del f, host

    # 3) the --latent_path flow on the full-size DC-AE
    g = torch.Generator().manual_seed(1)
    mean = torch.randn(84, generator=g)
    std = torch.rand(84, generator=g) + 0.5
    mean[81], std[81] = 101325.0, 1200.0
    model = AutoencoderDC.from_config(dict(CONFIG_DCAE_84)).cuda().eval()
    with tempfile.TemporaryDirectory() as d:
        lat_ = torch.randn(1, E, 84, F, 15, 30, generator=g)
        (path,) = save_latent_npy(lat_, [2018100100], d)
        del lat_
        res["latent_flow_s"] = {}
        for mode in ("fp32", "bf16x3"):
            model.set_gemm_precision(mode)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                track_latent_ensemble(path, model, mean, std, 15.2, 140.3, S)  # warm-up: plans, graphs
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ens, mtrk = track_latent_ensemble(path, model, mean, std, 15.2, 140.3, S)
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res["latent_flow_s"][mode] = round(dt, 3)
            res.setdefault("latent_flow_ms_per_frame", {})[mode] = round(dt * 1e3 / (E * F), 3)
            assert len(ens) == E and len(mtrk) == F
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
