"""Tropical-cyclone tracking through a decoded ensemble on the GPU (ladcast/evaluate/track.py:24-25,55-81,151-335 and its
``--latent_path`` mode, :758-909, with the decode of ladcast/pipelines/utils.py:83-246).

The reference decodes every member into an xarray dataset on the host and walks it with a Python loop.  Here the decoded frames
stay on the device: only the two fields the tracker reads are gathered (``ldc_track_gather``, bit-equal to
``decode_latent_ens(...)[:, ch]``), the ensemble mean is taken on the device (``ldc_track_nanmean``, bit-equal to ``np.nanmean``
over the members) and every track - all members plus the mean - runs in one launch (``ldc_track_storms``); only the tracks come
back to the host.  The search reproduces the reference's float arithmetic coordinate for coordinate; tests/golden/make_track_golden.py
pins it against the reference's own functions.

Grid convention (``latent_ens_to_xarr``): fp64 coordinates ``latitude = np.arange(-88.5, 90 + 1e-6, 1.5)`` (120 rows, ascending,
the south-pole row cropped) and ``longitude = np.arange(0, 358.5 + 1e-6, 1.5)`` (240 columns); a field is an fp32 ``(H, W)`` plane,
row = latitude.  Frame ``k`` of a rollout is lead ``6 h * k``; frame 0 is the initial condition.

Plotting, storm-catalogue (IBTrACS / HURDAT) reading and downloading, KML model tracks and the IFS-ENS zarr path are not here.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import warnings
from datetime import datetime, timedelta
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import hip

GRID_RES = 1.5  # ERA5 grid resolution in degrees
NEIGHBOR_DEG = 1.5  # half-width of the local-min search box

VARIABLE_NAMES = [
    "geopotential",
    "specific_humidity",
    "temperature",
    "u_component_of_wind",
    "v_component_of_wind",
    "vertical_velocity",
    "10m_u_component_of_wind",
    "10m_v_component_of_wind",
    "2m_temperature",
    "mean_sea_level_pressure",
    "sea_surface_temperature",
    "total_precipitation_6hr",
]
LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
NUM_ATM_VARS = 6
MSLP_CHANNEL = NUM_ATM_VARS * len(LEVELS) + 3  # surface variable 3: 81
Z700_CHANNEL = LEVELS.index(700)  # geopotential (atmospheric variable 0) at 700 hPa: 9
STEP_HOURS = 6

Track = List[Tuple[datetime, float, float]]


def latitude_grid() -> np.ndarray:
    """the decoded grid's latitudes, as latent_ens_to_xarr builds them (pipelines/utils.py:161)"""
    return np.arange(-88.5, 90.0 + 1e-6, 1.5)


def longitude_grid() -> np.ndarray:
    return np.arange(0.0, 358.5 + 1e-6, 1.5)


def round_to_grid(val, resolution=GRID_RES):
    """track.py:151-153 (np.round: half to even)"""
    return float(np.round(val / resolution) * resolution)


def py_mod_restated(x: float, m: float) -> float:
    """Python's float ``%`` as the tracker kernel computes it (CPython's float_rem): fmod, then the divisor's sign; a zero remainder
    is +0.0 for m > 0.  tests/test_track_cpu.py holds it to ``x % m``."""
    r = math.fmod(x, m)
    if r != 0.0:
        if (m < 0.0) != (r < 0.0):
            r += m
    else:
        r = math.copysign(0.0, m)
    return r


# ---- argument checks and device inputs ------------------------------------------------------------------------------------
def _require_device(*ts):
    for t in ts:
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise RuntimeError("ladcast_amd tracking needs device tensors (no CPU fallback)")


def _check_boxes(inner_box_sizes) -> List[int]:
    boxes = list(inner_box_sizes)
    if not boxes:
        raise ValueError("inner_box_sizes must not be empty")
    if len(boxes) > hip.TRACK_MAX_BOXES:
        raise ValueError(f"at most {hip.TRACK_MAX_BOXES} inner box sizes, got {len(boxes)}")
    out = []
    for b in boxes:
        if float(b) != int(b):
            raise ValueError(f"inner box sizes are whole degrees, got {b}")
        if not 0 <= int(b) <= hip.TRACK_MAX_INNER:
            raise ValueError(f"inner box size {b} outside [0, {hip.TRACK_MAX_INNER}] degrees")
        out.append(int(b))
    return out


_grid_cache: Dict = {}


def _grid(dev, lat, lon):
    lat = latitude_grid() if lat is None else np.asarray(lat, dtype=np.float64)
    lon = longitude_grid() if lon is None else np.asarray(lon, dtype=np.float64)
    for name, c in (("lat", lat), ("lon", lon)):
        if c.ndim != 1 or not 0 < c.size <= hip.TRACK_MAX_GRID or not np.all(np.isfinite(c)) or np.any(np.diff(c) <= 0):
            raise ValueError(f"{name} must be 1-D, finite, strictly ascending, 1..{hip.TRACK_MAX_GRID} entries")
    key = (str(dev), lat.tobytes(), lon.tobytes())
    hit = _grid_cache.get(key)
    if hit is None:
        if len(_grid_cache) >= 16:
            _grid_cache.clear()
        hit = _grid_cache[key] = (torch.from_numpy(lat.copy()).to(dev), torch.from_numpy(lon.copy()).to(dev))
    return hit


def _f64(values, dev):
    return torch.tensor([float(v) for v in values], dtype=torch.float64).to(dev)


# ---- the search and the tracker -------------------------------------------------------------------------------------------
def find_local_minima(fields: torch.Tensor, centers: Sequence[Tuple[float, float]], inner_degs: Sequence[int],
                      field_idx: Optional[Sequence[int]] = None, *, lat=None, lon=None) -> List[Optional[Tuple[float, float, float]]]:
    """A batch of ``find_local_minimum`` calls in one launch (``ldc_track_local_min``).  fields: ``(F, H, W)`` fp32 device planes;
    query q searches ``fields[field_idx[q]]`` (default: q) around ``centers[q]`` with inner size ``inner_degs[q]``.  Each result is
    ``(la, lo, v)`` or None, as the reference returns them.  ``lat`` / ``lon``: any strictly ascending finite grid of up to
    ``hip.TRACK_MAX_GRID`` entries per axis (default: the decoded 120 x 240 grid); a non-finite centre gives None.

    The distance key that picks the closest surviving minimum is ``d * d`` per coordinate difference, each product correctly
    rounded.  It equals the reference's ``d ** 2`` bit for bit whenever the differences square exactly (the default grid; any
    dyadic grid and centre).  Otherwise it can differ by one rounding per term, which can decide only between candidates whose
    keys are within 2 ulp of each other."""
    _require_device(fields)
    if fields.dim() != 3 or fields.dtype != torch.float32:
        raise ValueError("fields must be (F, H, W) float32")
    nq = len(centers)
    if nq == 0:
        return []
    if field_idx is None:
        field_idx = list(range(nq))
    if len(field_idx) != nq or len(inner_degs) != nq:
        raise ValueError("one field index, center and inner size per query")
    if any(not 0 <= int(i) < fields.shape[0] for i in field_idx):
        raise ValueError("field index out of range")
    inner = [_check_boxes([b])[0] for b in inner_degs]
    fields = fields.contiguous()
    dev = fields.device
    glat, glon = _grid(dev, lat, lon)
    H, W = glat.numel(), glon.numel()
    if tuple(fields.shape[1:]) != (H, W):
        raise ValueError(f"fields are {tuple(fields.shape[1:])}, the grid is {(H, W)}")
    lat0 = _f64([c[0] for c in centers], dev)
    lon0 = _f64([c[1] for c in centers], dev)
    fi = torch.tensor([int(i) for i in field_idx], dtype=torch.int32).to(dev)
    inn = torch.tensor(inner, dtype=torch.int32).to(dev)
    found = torch.empty(nq, dtype=torch.int32, device=dev)
    la = torch.empty(nq, dtype=torch.float64, device=dev)
    lo = torch.empty(nq, dtype=torch.float64, device=dev)
    v = torch.empty(nq, dtype=torch.float32, device=dev)
    hip.track_local_min(fields, fi, glat, glon, lat0, lon0, inn, found, la, lo, v, field_stride=H * W, H=H, W=W, n_queries=nq)
    found, la, lo, v = found.cpu().tolist(), la.cpu().tolist(), lo.cpu().tolist(), v.cpu().numpy()
    if any(f not in (0, 1) for f in found):
        raise RuntimeError("ldc_track_local_min refused a query")
    return [(la[q], lo[q], float(v[q])) if found[q] else None for q in range(nq)]


def find_local_minimum(field2d: torch.Tensor, center: Tuple[float, float], inner_deg: int, *, lat=None, lon=None):
    """track.py:173-238 on one ``(H, W)`` fp32 device plane: ``(la, lo, v)`` of the local minimum closest to ``center`` or None"""
    _require_device(field2d)
    return find_local_minima(field2d.unsqueeze(0), [center], [inner_deg], lat=lat, lon=lon)[0]


def _track_launch(fields, *, track_stride, frame_stride, mslp_off, z_off, lsm, n_tracks, n_frames, n_steps, lat0, lon0,
                  inner_box_sizes, enforce_msl, lat, lon):
    """one ldc_track_storms launch over a contiguous fp32 buffer -> (lat, lon) (n_tracks, n_steps + 1) fp64, codes (n_tracks, n_steps)"""
    boxes = _check_boxes(inner_box_sizes)
    if n_steps < 0 or n_steps + 1 > n_frames:
        raise ValueError(f"n_steps={n_steps} needs {n_steps + 1} frames, the fields hold {n_frames}")
    dev = fields.device
    glat, glon = _grid(dev, lat, lon)
    H, W = glat.numel(), glon.numel()
    if tuple(fields.shape[-2:]) != (H, W):
        raise ValueError(f"fields are {tuple(fields.shape[-2:])}, the grid is {(H, W)}")
    last = (n_tracks - 1) * track_stride + n_steps * frame_stride + max(mslp_off, z_off or 0) + H * W
    if not fields.is_contiguous() or last > fields.numel():
        raise ValueError("the track / frame strides reach past the fields")
    if not enforce_msl:
        if lsm is None or z_off is None:
            raise ValueError("enforce_msl=False needs z700 and land_sea_mask")
        _require_device(lsm)
        lsm = lsm.to(torch.float32).contiguous()
        if tuple(lsm.shape) != (H, W):
            raise ValueError(f"land_sea_mask must be {(H, W)}")
    out_lat = torch.empty(n_tracks, n_steps + 1, dtype=torch.float64, device=dev)
    out_lon = torch.empty_like(out_lat)
    out_code = torch.empty(n_tracks, max(n_steps, 1), dtype=torch.int32, device=dev)
    hip.track_storms(fields, glat, glon, _f64(lat0, dev), _f64(lon0, dev), out_lat, out_lon, out_code, track_stride=track_stride,
                     frame_stride=frame_stride, mslp_off=mslp_off, z_off=-1 if z_off is None else z_off, lsm=None if enforce_msl else lsm,
                     H=H, W=W, n_tracks=n_tracks, n_steps=n_steps, inner_box_sizes=boxes, enforce_msl=enforce_msl)
    return out_lat.cpu().numpy(), out_lon.cpu().numpy(), out_code[:, :n_steps].cpu().numpy()


def _to_track(t0, lats, lons, codes, enforce_msl) -> Track:
    """the reference's list of (time, lat, lon), with its warnings for the steps that did not move (track.py:318-327)"""
    track = [(t0, float(lats[0]), float(lons[0]))]
    for step in range(1, len(lats)):
        t_next = t0 + timedelta(hours=STEP_HOURS * step)
        if codes[step - 1] == 0:
            if enforce_msl:
                warnings.warn(f"Enforce msl but no local min found at {t_next}, not moving")
            else:
                warnings.warn(f"Tried geopotential but no local min found at {t_next}, not moving")
        track.append((t_next, float(lats[step]), float(lons[step])))
    return track


def track_first_n_steps(t0, raw_lat0, raw_lon0, mslp: torch.Tensor, *, z700: Optional[torch.Tensor] = None,
                        land_sea_mask: Optional[torch.Tensor] = None, n_steps: int, inner_box_sizes=(7, 4, 1), enforce_msl: bool = True,
                        lat=None, lon=None, return_codes: bool = False):
    """track.py:243-335 on device tensors.  mslp (and z700): ``(T, H, W)`` for one track or ``(E, T, H, W)`` for E tracks, fp32,
    frame k = lead 6 h * k; all tracks run in one launch.  Returns one track ``[(t0, lat0, lon0), (t0 + 6 h, lat, lon), ...]`` or a
    list of them (with ``return_codes``: also the per-step codes of ldc_track_storms, (n_steps,) or (E, n_steps))."""
    _require_device(mslp, z700, land_sea_mask)
    single = mslp.dim() == 3
    if mslp.dim() not in (3, 4) or mslp.dtype != torch.float32:
        raise ValueError("mslp must be (T, H, W) or (E, T, H, W) float32")
    m = mslp.unsqueeze(0) if single else mslp
    if z700 is not None:
        z = z700.unsqueeze(0) if single else z700
        if z.shape != m.shape or z.dtype != torch.float32:
            raise ValueError("z700 must have the shape and dtype of mslp")
        buf = torch.stack([m, z], dim=2).contiguous()  # (E, T, 2, H, W)
        z_off = m.shape[-2] * m.shape[-1]
    else:
        buf = m.unsqueeze(2).contiguous()
        z_off = None
    E, T, nc, H, W = buf.shape
    if not (math.isfinite(raw_lat0) and math.isfinite(raw_lon0)):
        raise ValueError("the start must be finite")
    lat0, lon0 = round_to_grid(raw_lat0), round_to_grid(raw_lon0)
    lats, lons, codes = _track_launch(buf, track_stride=T * nc * H * W, frame_stride=nc * H * W, mslp_off=0, z_off=z_off, lsm=land_sea_mask,
                                      n_tracks=E, n_frames=T, n_steps=n_steps, lat0=[lat0] * E, lon0=[lon0] * E,
                                      inner_box_sizes=inner_box_sizes, enforce_msl=enforce_msl, lat=lat, lon=lon)
    tracks = [_to_track(t0, lats[e], lons[e], codes[e], enforce_msl) for e in range(E)]
    if single:
        return (tracks[0], codes[0]) if return_codes else tracks[0]
    return (tracks, codes) if return_codes else tracks


# ---- the --latent_path flow -----------------------------------------------------------------------------------------------
def _timestamp_to_datetime(ts) -> datetime:
    return datetime.strptime(str(int(ts)), "%Y%m%d%H")


@torch.no_grad()
def track_latent_ensemble(latents_or_path: Union[str, torch.Tensor], encdec_model, mean_tensor, std_tensor, raw_lat0: float,
                          raw_lon0: float, n_steps: int, *, timestamp=None, ens_member_idx: Optional[Sequence[int]] = None,
                          ens_mean: bool = True, decode_batch_frames: Optional[int] = None, inner_box_sizes=(7, 4, 1),
                          enforce_msl: bool = True, land_sea_mask: Optional[torch.Tensor] = None, lat=None, lon=None,
                          return_fields: bool = False):
    """The reference's ``--latent_path`` mode (track.py:758-840): a saved ``latent_YYYYMMDDHH.npy`` (or an ``(ens, C, T, h, w)``
    tensor with ``timestamp``) -> ``({"M{m}": track, ...}, mean_track)``.

    ``n_steps + 1`` frames of each selected member are decoded (``decode_batch_frames`` frames per decoder call; None = all of a
    member's frames at once, as ``latent_ens_to_xarr`` does), de-normalised and gathered on the device into one
    ``(E [+ 1], n_steps + 1, n_ch, H, W)`` buffer (MSLP, then Z700 when ``enforce_msl=False``); the mean over the members fills the
    last slot; one tracker launch runs every member and the mean.  ``mean_track`` is None without ``ens_mean``.  The start time
    is the file's timestamp (the dataset's only ``time``).  ``return_fields``: also return the buffer."""
    from ..pipelines.io import load_latent_npy
    from ..pipelines.utils import _device_vector

    if isinstance(latents_or_path, (str, os.PathLike)):
        latents, ts = load_latent_npy(os.fspath(latents_or_path))
    else:
        if timestamp is None:
            raise ValueError("When passing a tensor, you must give a timestamp")
        latents, ts = latents_or_path, timestamp
    t0 = ts if isinstance(ts, datetime) else _timestamp_to_datetime(ts)
    if latents.dim() != 5:
        raise ValueError(f"latents must be (ens, C, T, h, w), got {tuple(latents.shape)}")
    ens, C, T, h, w = latents.shape
    F = n_steps + 1
    if n_steps < 0 or T < F:
        raise ValueError(f"n_steps={n_steps} needs {F} frames, the latents hold {T}")
    members = list(range(ens)) if ens_member_idx is None else [int(m) for m in ens_member_idx]
    if not members or any(not 0 <= m < ens for m in members):
        raise ValueError(f"ensemble members must lie in [0, {ens})")
    boxes = _check_boxes(inner_box_sizes)
    dev = encdec_model.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("ladcast_amd tracking needs the model on the device (no CPU fallback)")
    if not enforce_msl:
        _require_device(land_sea_mask)
    channels = [MSLP_CHANNEL] if enforce_msl else [MSLP_CHANNEL, Z700_CHANNEL]
    mean_d, std_d = _device_vector(mean_tensor, dev), _device_vector(std_tensor, dev)
    per = F if not decode_batch_frames else max(1, int(decode_batch_frames))
    E = len(members)
    buf = None
    for i, m in enumerate(members):
        for s0 in range(0, F, per):
            nf = min(per, F - s0)
            x = latents[m : m + 1, :, s0 : s0 + nf].to(dev).permute(0, 2, 1, 3, 4).reshape(nf, C, h, w).contiguous()
            y = encdec_model.decode(x).sample  # (nf, C', H, W): frame-major, gathered without the permute
            Cy, H, W = y.shape[1:]
            if max(channels) >= Cy or mean_d.numel() != Cy:
                raise ValueError(f"the decoder gives {Cy} channels; tracking reads channels {channels} and needs {Cy} statistics")
            if buf is None:
                buf = torch.empty(E + int(bool(ens_mean)), F, len(channels), H, W, dtype=torch.float32, device=dev)
            y = y.contiguous()
            hip.track_gather(y, buf[i], channels, mean_d, std_d, sb=0, st=Cy * H * W, sc=H * W, B=1, T=nf, HW=H * W, T_total=F, t_off=s0)
    nc, H, W = buf.shape[2:]
    per_track = F * nc * H * W
    if ens_mean:
        hip.track_nanmean(buf, buf[E], member_stride=per_track, E=E, n=per_track)
    lat0, lon0 = round_to_grid(raw_lat0), round_to_grid(raw_lon0)
    n_tracks = buf.shape[0]
    lats, lons, codes = _track_launch(buf, track_stride=per_track, frame_stride=nc * H * W, mslp_off=0,
                                      z_off=None if enforce_msl else H * W, lsm=land_sea_mask, n_tracks=n_tracks, n_frames=F,
                                      n_steps=n_steps, lat0=[lat0] * n_tracks, lon0=[lon0] * n_tracks, inner_box_sizes=boxes,
                                      enforce_msl=enforce_msl, lat=lat, lon=lon)
    ens_tracks = {f"M{m}": _to_track(t0, lats[i], lons[i], codes[i], enforce_msl) for i, m in enumerate(members)}
    mean_track = _to_track(t0, lats[E], lons[E], codes[E], enforce_msl) if ens_mean else None
    if return_fields:
        return ens_tracks, mean_track, buf
    return ens_tracks, mean_track


# ---- CSV files (track.py:55-81, 891-909) ----------------------------------------------------------------------------------
def save_tracks_csv(ens_tracks: Dict[str, Track], mean_track: Optional[Track], members_csv: str, mean_csv: Optional[str]):
    """``ladcast_members.csv`` / ``ladcast_mean.csv`` with the reference's columns: members ``time, lat, lon, member, step``,
    mean ``time, lat, lon, step, member`` (member = "mean")"""
    import pandas as pd

    rows = []
    for member, track in ens_tracks.items():
        df = pd.DataFrame(track, columns=["time", "lat", "lon"])
        df["member"] = member
        df["step"] = df.index
        rows.append(df)
    pd.concat(rows, ignore_index=True).to_csv(members_csv, index=False)
    if mean_csv is not None and mean_track is not None:
        mean_df = pd.DataFrame(mean_track, columns=["time", "lat", "lon"])
        mean_df["step"] = mean_df.index
        mean_df["member"] = "mean"
        mean_df.to_csv(mean_csv, index=False)


def load_ensemble_members(csv_path="ensemble_members.csv"):
    """{member: [(time, lat, lon), ...]} in step order (track.py:55-71)"""
    import pandas as pd

    df = pd.read_csv(csv_path, parse_dates=["time"])
    ens_tracks = {}
    for member, grp in df.groupby("member"):
        grp = grp.sort_values("step")
        ens_tracks[member] = list(zip(grp["time"], grp["lat"], grp["lon"]))
    return ens_tracks


def load_ensemble_mean(csv_path="ensemble_mean.csv"):
    """[(time, lat, lon), ...] in step order (track.py:74-81)"""
    import pandas as pd

    df = pd.read_csv(csv_path, parse_dates=["time"])
    df = df.sort_values("step")
    return list(zip(df["time"], df["lat"], df["lon"]))


# ---- command line ---------------------------------------------------------------------------------------------------------
def mean_std_from_json(normalization_param_dict: Dict, variable_names=VARIABLE_NAMES):
    """per-channel (mean, std) fp32 tensors from the normalisation JSON (dataloader/utils.py:272-301, precompute_mean_std)"""
    means, stds = [], []
    for var in variable_names:
        if var not in normalization_param_dict:
            raise ValueError(f"No normalization parameters found for variable {var}.")
        p = normalization_param_dict[var]
        if isinstance(p["mean"], dict):
            for level in p["mean"].keys():
                means.append(p["mean"][level])
                stds.append(p["std"][level])
        else:
            means.append(p["mean"])
            stds.append(p["std"])
    return torch.tensor(means, dtype=torch.float32), torch.tensor(stds, dtype=torch.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Track a tropical cyclone through a saved latent ensemble (track.py --latent_path mode)")
    ap.add_argument("--latent_path", required=True, help="latent_YYYYMMDDHH.npy written by a rollout")
    ap.add_argument("--normalization_json", required=True, help="per-variable mean / std JSON of the decoded fields")
    ap.add_argument("--encdec_model", required=True, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--lat", type=float, required=True, help="start latitude (rounded to the 1.5 degree grid)")
    ap.add_argument("--lon", type=float, required=True, help="start longitude in degrees east (rounded to the grid)")
    ap.add_argument("--startdate", type=str, default=None, help="YYYYMMDDHH; must equal the file's timestamp when given")
    ap.add_argument("--n_steps", type=int, required=True, help="number of 6-h steps")
    ap.add_argument("--inner_box_sizes", type=str, default="7,4,1", help="comma-separated inner box sizes in degrees")
    ap.add_argument("--ens_member", type=str, default=None, help='comma-separated members (e.g. "0,2,5"); default all')
    ap.add_argument("--no_mean", action="store_true", help="skip the ensemble-mean track")
    ap.add_argument("--decode_batch_frames", type=int, default=None, help="frames per decoder call (default: a member's frames at once)")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    ap.add_argument("--members_csv", type=str, default="ladcast_members.csv")
    ap.add_argument("--mean_csv", type=str, default="ladcast_mean.csv")
    args = ap.parse_args(argv)

    from ..models import AutoencoderDC

    with open(args.normalization_json) as f:
        mean_t, std_t = mean_std_from_json(json.load(f))
    if os.path.isdir(args.encdec_model) and any(n.endswith((".safetensors", ".bin")) for n in os.listdir(args.encdec_model)):
        model = AutoencoderDC.from_pretrained(args.encdec_model)
    else:
        cfg_path = os.path.join(args.encdec_model, "config.json") if os.path.isdir(args.encdec_model) else args.encdec_model
        with open(cfg_path) as f:
            model = AutoencoderDC.from_config(json.load(f))
        warnings.warn(f"{args.encdec_model}: no weights found, the DC-AE keeps its initial weights")
    model = model.to("cuda").eval()
    model.set_gemm_precision(args.gemm_precision)
    if args.startdate is not None:
        file_ts = os.path.basename(args.latent_path).split("_")[-1].split(".")[0]
        if args.startdate != file_ts:
            raise SystemExit(f"--startdate {args.startdate} differs from the file's timestamp {file_ts}")
    members = [int(m) for m in args.ens_member.split(",")] if args.ens_member else None
    boxes = [int(b) for b in args.inner_box_sizes.split(",")]
    ens_tracks, mean_track = track_latent_ensemble(args.latent_path, model, mean_t, std_t, args.lat, args.lon, args.n_steps,
                                                   ens_member_idx=members, ens_mean=not args.no_mean,
                                                   decode_batch_frames=args.decode_batch_frames, inner_box_sizes=boxes)
    save_tracks_csv(ens_tracks, mean_track, args.members_csv, None if args.no_mean else args.mean_csv)
    for name, trk in list(ens_tracks.items()) + ([("mean", mean_track)] if mean_track else []):
        print(f"{name}: " + " -> ".join(f"({la:.1f}, {lo:.1f})" for _, la, lo in trk))


if __name__ == "__main__":
    main()
