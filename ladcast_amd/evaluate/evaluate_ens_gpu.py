"""Scores of a saved ensemble rollout on the device (reference: ladcast/evaluate/evaluate_ens_gpu.py): the `latent_YYYYMMDDHH.npy`
files a rollout wrote -> `ens_acc`, `ens_mse`, `crps_spread`, `crps_skill`, `crps` arrays of shape (init time, C, lead time).

Per initial time the latents are decoded lead-major, a few lead times per decoder call, and every decoder output is scored where it
lies by one `ldc_rollout_scores` launch: the inverse normalisation is fused into the scorer's loads, truth and climatology are tables
of planes indexed by a slot per lead time, and the five (C, lead time) arrays fill one device buffer that comes to the host in a single
copy.  Decoded fields never exist beyond one decode batch (the reference keeps the whole (ens, C, T, H, W) array: 19.4 GB at
50 x 84 x 40 x 120 x 240).

    python -m ladcast_amd.evaluate.evaluate_ens_gpu --result_path rollout/ --data_path era5_2018.npy --climatology_path clim.npy \\
        --normalization_json ERA5_normal.json --encdec_model DCAE/ --start_date 2018-01-01 --end_date 2018-12-31T18 --output scores/ --crop_init

xarray / zarr are not available: `--data_path` is a .npy of raw frames (N, C, H_in, W), `--step_size_hour` apart, the first at
`--start_date`; `--climatology_path` a .npy (366, 4, C, H_in, W) (day of year, hour 0 / 6 / 12 / 18).  `H_in == H + 1` crops row 0,
the south pole.  `--reliability`, `--spectrum`, `--event` / `--event_anomaly` / `--fss_scales`, `--region` / `--region_box` and `--energy` /
`--energy_group` add metrics that are not in the reference; what each computes and writes is stated by its class in `rollout_metrics`.
`--derive NAME speed|diff|shear|vorticity|divergence CHANNEL ...` appends a derived field (`derived`: wind speed, a difference, vertical
shear, relative vorticity or divergence of a wind on the grid) to the channels: every array gains a row, and `derived.json` names the fields.
Single rank only: splitting the initial times over ranks (`accelerate.split_between_processes`), more than 64
members and the reference's commented-out `single_mse` are out of scope.
"""
from __future__ import annotations

import argparse
import json
import os
import warnings
from datetime import datetime, timedelta
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from .track import LEVELS, NUM_ATM_VARS, VARIABLE_NAMES, mean_std_from_json
from .rollout_metrics import (ENERGY_GROUP_NAMES, ENERGY_KEYS, ENERGY_NAMES, EVENTS_KEYS, FSS_KEYS, METRICS, REGIONAL_KEYS, RELIABILITY_KEYS,  # noqa: F401
                              SPECTRUM_KEYS, Batch, _channel_names, _crop_rows, parse_energy_groups, parse_events, parse_fss_scales, parse_regions, row_latitudes,
                              spectrum_band_weights)  # the keys and parsers are this module's names too
from .utils import SCORE_NAMES, get_normalized_lat_weights_based_on_cos, rollout_scores

SST_CHANNEL_IDX = 82
CLIMATOLOGY_HOURS = (0, 6, 12, 18)


def _to_datetime(t) -> datetime:
    if isinstance(t, datetime):
        return t
    if isinstance(t, np.datetime64):
        return t.astype("datetime64[s]").tolist()
    if isinstance(t, (int, np.integer)):
        return datetime.strptime(str(int(t)), "%Y%m%d%H")
    return datetime.fromisoformat(str(t))


def climatology_slots(start_time, lead_time: int, interval: int = 6, exclude_start: bool = True,
                      hours: Sequence[int] = CLIMATOLOGY_HOURS) -> List[int]:
    """The index computation of climatology_to_timeseries (evaluate/utils.py:173-186) for a (dayofyear = 1..366, hour) climatology
    flattened to (366 * len(hours)) planes: the times `start_time`, `+ interval` h, ... up to `start_time + lead_time` h (the start
    left out with `exclude_start`) -> slot `(dayofyear - 1) * len(hours) + hours.index(hour)` per time.  Host only (datetime)."""
    start = _to_datetime(start_time)
    hours = [int(h) for h in hours]
    n = int(lead_time) // int(interval)  # pd.date_range(start, end, freq): every whole interval up to and including the end
    slots = []
    for k in range(1 if exclude_start else 0, n + 1):
        t = start + timedelta(hours=k * int(interval))
        if t.hour not in hours or t.minute or t.second:
            raise ValueError(f"{t.isoformat()} is not at one of the climatology's hours {hours}")
        slots.append((t.timetuple().tm_yday - 1) * len(hours) + hours.index(t.hour))
    return slots


def truth_frame_slots(init_time, start_date, step_size_hour: int, total_num_steps: int) -> List[int]:
    """frames `step_size_hour` apart, the first at `start_date`: lead time t (0-based) of the forecast started at `init_time` is frame
    `(init_time - start_date) / step + 1 + t` (evaluate_ens_gpu.py:312-319: the frames from init + step to init + total lead time)"""
    delta = _to_datetime(init_time) - _to_datetime(start_date)
    hours, rem = divmod(delta.total_seconds(), 3600)
    first, off = divmod(int(hours), int(step_size_hour))
    if rem or off:
        raise ValueError(f"initial time {init_time} is not a whole number of {step_size_hour} h steps after {start_date}")
    return [first + 1 + t for t in range(total_num_steps)]


def _stage_planes(table, slots: Sequence[int], dev, what: str):
    """a host table (N, C, H, W) (array, memmap or tensor): only the planes `slots` names go to the device, the slots are renumbered"""
    slots = [int(s) for s in slots]
    if any(not 0 <= s < table.shape[0] for s in slots):
        raise ValueError(f"{what}: slots {slots} reach outside the table's {table.shape[0]} entries")
    used = sorted(set(slots))
    if isinstance(table, torch.Tensor):
        host = table[used].to(torch.float32)
    else:
        host = torch.from_numpy(np.stack([np.asarray(table[s], dtype=np.float32) for s in used]))
    return host.to(dev), [used.index(s) for s in slots]


@torch.no_grad()
def score_latent_rollout(latents_or_path: Union[str, torch.Tensor], encdec_model, mean_tensor, std_tensor, truth, truth_slots: Sequence[int],
                         clim, clim_slots: Optional[Sequence[int]], lat_weight: torch.Tensor, *, sst_channel: int = SST_CHANNEL_IDX,
                         total_num_steps: Optional[int] = None, crop_init: bool = False, force_ens_size: Optional[int] = None,
                         decode_batch_frames: Optional[int] = None, reliability: bool = False, spectrum: bool = False,
                         spectrum_row_weight: Optional[torch.Tensor] = None, events: Optional[Sequence] = None,
                         regions: Optional[Sequence] = None, region_mask=None, fss_radii: Optional[Sequence[int]] = None, energy: bool = False,
                         energy_groups: Optional[Sequence] = None, energy_scales=None, derived: Optional[Sequence] = None,
                         score_maps: Optional["ScoreMaps"] = None) -> Dict[str, torch.Tensor]:  # noqa: F821  (score_maps.ScoreMaps)
    """One initial time of evaluate_ens_gpu.py:268-425: a saved `latent_YYYYMMDDHH.npy` (or its (ens, C, T, h, w) tensor) -> the five
    (C, total_num_steps) fp32 CPU tensors `ens_acc`, `ens_mse`, `crps_spread`, `crps_skill`, `crps`.

    The T lead times are decoded lead-major, `max(1, decode_batch_frames // ens)` of them per decoder call (default: one, i.e. `ens`
    frames), and each decoder output is scored in place with the inverse normalisation (`mean_tensor` / `std_tensor`, one value per
    decoded channel) fused into the scorer: the peak memory for decoded fields is one decode batch.  truth / clim are (N, C, H, W)
    tables in physical units of which lead t reads entry `truth_slots[t]` / `clim_slots[t]` (clim None: no ACC).  On the device they
    are indexed where they are; host arrays or memmaps have only the planes this initial time needs staged to the device.  Columns
    T .. total_num_steps - 1 stay NaN, as the reference's `torch.full(nan)` leaves them; T > total_num_steps is a ValueError (the
    reference fails with an index error).  `crop_init` drops slot 0 (the IC latent), `force_ens_size` keeps the first members.

    `reliability`, `spectrum` / `spectrum_row_weight`, `events` / `fss_radii`, `regions` / `region_mask`, `energy` / `energy_groups` /
    `energy_scales` switch on the optional metrics of `rollout_metrics.METRICS` (`Reliability`, `Spectrum`, `Events`, `Regional`,
    `Energy`: each class states its options and the keys the result gains).  Every decode batch goes through each of them, in that
    order, while it is on the device; nothing more is decoded or kept.  Every other output is the bits of a call without it.
    `score_maps`: a `score_maps.ScoreMaps` accumulator (`Maps`, the last of them); every decode batch is added to it on the device and
    the result gains no key: the caller downloads the accumulator once, after the last initial time.

    `derived`: a sequence of `derived.Derived(name, kind, channels)`; the D fields become channels C' .. C' + D - 1 of every result
    and of every option that names a channel (`events`, `energy_groups`, `energy_scales`).  Each decode batch is copied into the head
    of a (lead, ens, C' + D, H, W) buffer whose tail `derive_forecast` fills; truth and climatology become per-batch tables extended
    the same way, the climatology of a `speed` / `shear` field NaN (so its `ens_acc` is NaN; `vorticity` / `divergence` are linear in the
    wind and have a true climatology, on the rows `row_latitudes(H)`).  A field that reads `sst_channel` and an
    anomaly event on a `speed` / `shear` field are ValueErrors.  Without `derived` not one launch or copy is added."""
    from ..pipelines.io import load_latent_npy
    from ..pipelines.utils import _device_vector

    if isinstance(latents_or_path, (str, os.PathLike)):
        latents, _ = load_latent_npy(os.fspath(latents_or_path), crop_init=crop_init, force_ens_size=force_ens_size)
    else:
        latents = latents_or_path
        if latents.dim() != 5:
            raise ValueError(f"latents must be (ens, C, T, h, w), got {tuple(latents.shape)}")
        if crop_init:
            latents = latents[:, :, 1:]
        if force_ens_size is not None:
            latents = latents[:force_ens_size]
    ens, C, T, h, w = latents.shape
    total = T if total_num_steps is None else int(total_num_steps)
    if T > total:
        raise ValueError(f"the latents hold {T} lead times, total_num_steps is {total}")
    if ens < 1 or T < 1:
        raise ValueError(f"nothing to score in latents of shape {tuple(latents.shape)}")
    if len(truth_slots) < T or (clim is not None and len(clim_slots) < T):
        raise ValueError(f"{T} lead times need {T} truth and climatology slots")
    fields = None
    if derived is not None:
        from .derived import ExtendedBatch, _field_list, check_scoring_fields, extended_scales

        fields = _field_list(derived, int(torch.as_tensor(mean_tensor).numel()))
        check_scoring_fields(fields, int(torch.as_tensor(mean_tensor).numel()), sst_channel, events)
    options = dict(reliability=reliability, spectrum=spectrum, spectrum_row_weight=spectrum_row_weight, events=events, fss_radii=fss_radii,
                   regions=regions, region_mask=region_mask, energy=energy, energy_groups=energy_groups, energy_scales=energy_scales,
                   score_maps=score_maps, clim=clim, std_tensor=std_tensor if fields is None else extended_scales(fields, std_tensor))
    metrics = [m for m in (cls.for_rollout(options) for cls in METRICS) if m is not None]  # their options: checked before anything is decoded
    dev = encdec_model.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("ladcast_amd scoring needs the model on the device (no CPU fallback)")
    t_slots, c_slots = list(truth_slots[:T]), None if clim is None else list(clim_slots[:T])
    if not (isinstance(truth, torch.Tensor) and truth.is_cuda):
        truth, t_slots = _stage_planes(truth, t_slots, dev, "truth")
    if clim is not None and not (isinstance(clim, torch.Tensor) and clim.is_cuda):
        clim, c_slots = _stage_planes(clim, c_slots, dev, "clim")
    mean_d, std_d = _device_vector(mean_tensor, dev), _device_vector(std_tensor, dev)
    ext = None if fields is None else ExtendedBatch(fields, mean_d, std_d)
    lat_weight = lat_weight.to(dev, torch.float32)
    latents = latents.to(dev, torch.float32)
    for m in metrics:
        m.start(lat_weight)
    scores = None
    per = max(1, int(decode_batch_frames) // ens) if decode_batch_frames else 1  # lead times per decoder call: a lead time's members stay together
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        x = latents[:, :, s0 : s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ens, C, h, w).contiguous()  # lead-major, then member
        y = encdec_model.decode(x).sample  # (nl * ens, C', H, W), still normalised
        if ext is None:
            b = Batch(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, sst_channel, total,
                      dict(lead_dim=0, mean=mean_d, std=std_d, truth_slot=t_slots[s0 : s0 + nl], l_off=s0),
                      dict(clim=clim, clim_slots=None if clim is None else c_slots[s0 : s0 + nl]))
        else:  # the batch, its truth and its climatology with the derived fields as tail channels; the tables' slots are 0 .. nl - 1
            if y.shape[1] != ext.C:
                raise ValueError(f"the decoder gives {y.shape[1]} channels, mean_tensor / std_tensor hold {ext.C}")
            ext.buffer(per, ens, y.shape[2], y.shape[3], dev)[:nl, :, : ext.C].copy_(y.reshape(nl, ens, *y.shape[1:]))
            b = Batch(ext.derive(nl), ext.table("truth", truth, t_slots[s0 : s0 + nl], per), lat_weight, sst_channel, total,
                      dict(lead_dim=0, mean=ext.mean, std=ext.std, truth_slot=list(range(nl)), l_off=s0),
                      dict(clim=None if clim is None else ext.table("clim", clim, c_slots[s0 : s0 + nl], per),
                           clim_slots=None if clim is None else list(range(nl))))
        if scores is None:
            scores = torch.full((5, b.y.shape[2], total), float("nan"), device=dev, dtype=torch.float32)
        rollout_scores(b.y, b.truth, b.clim_kw["clim"], lat_weight, sst_channel, lead_dim=0, mean=b.kw["mean"], std=b.kw["std"],
                       truth_slots=b.kw["truth_slot"], clim_slots=b.clim_kw["clim_slots"], out=scores, lead_offset=s0)
        for m in metrics:
            m.run(b)
    host = scores.cpu()  # the one copy (and the one wait) of this initial time
    res = {k: host[i] for i, k in enumerate(SCORE_NAMES)}
    for m in metrics:
        res.update(m.result())
    return res


def lat_weights_for(H: int) -> torch.Tensor:
    """the reference's `get_normalized_lat_weights_based_on_cos(np.linspace(-88.5, 90, 120))` for the 120-row grid; any other H: the same
    formula over the H rows kept of an equiangular pole-to-pole grid of H + 1 (`equiangular_lat_weights`)"""
    if H == 120:
        return get_normalized_lat_weights_based_on_cos(torch.from_numpy(np.linspace(-88.5, 90, 120))).to(torch.float32)
    from .evaluate_encdec_model import equiangular_lat_weights

    return equiangular_lat_weights(H + 1, True)


def _load_encdec(path: str):
    """a DC-AE checkpoint directory (config.json + weights), or a config.json alone (initial weights, with a warning)"""
    from ..models import AutoencoderDC

    if os.path.isdir(path) and any(n.endswith((".safetensors", ".bin")) for n in os.listdir(path)):
        return AutoencoderDC.from_pretrained(path)
    cfg_path = os.path.join(path, "config.json") if os.path.isdir(path) else path
    with open(cfg_path) as f:
        model = AutoencoderDC.from_config(json.load(f))
    warnings.warn(f"{path}: no weights found, the DC-AE keeps its initial weights")
    return model


def main(argv=None, score: Optional[Callable] = None):
    """`score(path, time_str, truth_slots, clim_slots) -> {name: (C, total_num_steps)}` replaces the autoencoder, the data and the device
    (tests of the file handling).  Returns the gathered arrays, `timestamp` among them.

    The flags of the optional metrics, the keys the scorer then returns too and the files they add are stated by the classes of
    `rollout_metrics.METRICS`.  Without such a flag the launches and the files are those of a run before the flag existed.

    `timestamp.npy` is float32, as the reference stores it: YYYYMMDDHH does not fit fp32's 24 bits, e.g. 2018123118 reads back as
    2018123136.  The per-time file names carry the exact time."""
    ap = argparse.ArgumentParser(description="Score saved ensemble rollouts (evaluate_ens_gpu.py on .npy data)")
    ap.add_argument("--normalization_json", type=str, default="ERA5_normal.json", help="per-variable mean / std JSON of the decoded fields")
    ap.add_argument("--encdec_model", type=str, default=None, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--data_path", type=str, default=None, help=".npy of raw truth frames (N, C, H_in, W), step_size_hour apart from start_date")
    ap.add_argument("--result_path", type=str, default=None, help="directory of the rollout's latent_YYYYMMDDHH.npy files")
    ap.add_argument("--climatology_path", type=str, default=None, help=".npy climatology (366, 4, C, H_in, W): day of year x hour 0/6/12/18")
    ap.add_argument("--start_date", type=str, default="2018-01-01", help="time of the first frame of --data_path")
    ap.add_argument("--end_date", type=str, default="2018-12-31", help="initial times after end_date - total_lead_time_hour are dropped")
    ap.add_argument("--output", type=str, default=None, help="directory for the .npy results")
    ap.add_argument("--step_size_hour", type=int, default=6)
    ap.add_argument("--latent_spatial_scale", type=int, default=8, help="decoded rows / latent rows")
    ap.add_argument("--total_lead_time_hour", type=int, default=240)
    ap.add_argument("--load_ds_in_memory", action="store_true", help="upload truth and climatology to the device once")
    ap.add_argument("--crop_init", action="store_true", help="drop slot 0 of the latents (the initial condition)")
    ap.add_argument("--force_ens_size", type=int, default=None, help="score the first members only")
    ap.add_argument("--decode_batch_frames", type=int, default=None, help="frames per decoder call (default: one lead time's members)")
    ap.add_argument("--sst_channel_idx", type=int, default=SST_CHANNEL_IDX, help="the channel averaged with nanmean (NaN over land)")
    ap.add_argument("--variable_names", nargs="+", default=VARIABLE_NAMES, help="variables of the normalisation JSON, in channel order")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    for cls in METRICS:
        cls.add_arguments(ap)
    ap.add_argument("--derive", nargs="+", action="append", default=[], metavar="NAME_KIND_CHANNELS",
                    help="NAME speed|diff|shear|vorticity|divergence CHANNEL [CHANNEL ...]: also score this derived field (speed: sqrt(a^2 + b^2) of channels a b; "
                         "diff: a - b; shear: sqrt((a - c)^2 + (b - d)^2) of a b c d; vorticity, divergence: of the wind u v on the grid) as one more channel, which --event, --energy_group and the regional results then name; "
                         "may be given several times")
    ap.add_argument("--levels", type=int, nargs="+", default=LEVELS, help="pressure levels of the atmospheric variables, in channel order (--event channel names)")
    ap.add_argument("--num_atm_vars", type=int, default=NUM_ATM_VARS, help="leading variables that have one channel per level (--event channel names)")
    args = ap.parse_args(argv)

    if args.total_lead_time_hour % args.step_size_hour != 0:
        raise ValueError("total_lead_time_hour must be divisible by step_size_hour.")
    total_num_steps = args.total_lead_time_hour // args.step_size_hour
    if args.result_path is None or args.output is None:
        raise SystemExit("--result_path and --output are required")

    from ..pipelines.io import list_latent_files

    files = list_latent_files(args.result_path, end_date=args.end_date, total_lead_time_hour=args.total_lead_time_hour)
    if not files:
        raise SystemExit(f"{args.result_path}: no latent_*.npy at or before end_date - total_lead_time_hour")

    metrics = [m for m in (cls.from_args(args, total_num_steps, files) for cls in METRICS) if m is not None]
    fields = None
    if args.derive:
        from .derived import check_scoring_fields, derived_metadata, extended_scales, parse_derived

        decoded = _channel_names(args)[: -len(args.derive)]
        fields = parse_derived(args.derive, decoded)
        check_scoring_fields(fields, len(decoded), args.sst_channel_idx, [ev for m in metrics for ev in getattr(m, "events", ())])
        derived_meta = derived_metadata(fields, decoded)

    if score is None:
        if args.encdec_model is None or args.data_path is None or args.climatology_path is None:
            raise SystemExit("--encdec_model, --data_path and --climatology_path are required")
        with open(args.normalization_json) as f:
            mean_t, std_t = mean_std_from_json(json.load(f), args.variable_names)
            model = _load_encdec(args.encdec_model).to("cuda").eval()
        model.set_gemm_precision(args.gemm_precision)
        shape = np.load(files[0][1], mmap_mode="r").shape
        H = shape[-2] * args.latent_spatial_scale
        truth = np.load(args.data_path, mmap_mode="r")
        clim = np.load(args.climatology_path, mmap_mode="r")
        if truth.ndim != 4 or clim.ndim != 5 or clim.shape[:2] != (366, len(CLIMATOLOGY_HOURS)):
            raise ValueError(f"--data_path must be (N, C, H_in, W) and --climatology_path (366, 4, C, H_in, W); got {truth.shape} and {clim.shape}")
        truth = _crop_rows(truth, H, "--data_path")
        clim = _crop_rows(clim.reshape(-1, *clim.shape[2:]), H, "--climatology_path")
        if args.load_ds_in_memory:  # both tables resident on the device; otherwise planes are staged per initial time
            truth = torch.from_numpy(np.ascontiguousarray(truth, dtype=np.float32)).to("cuda")
            clim = torch.from_numpy(np.ascontiguousarray(clim, dtype=np.float32)).to("cuda")
        lat_w = lat_weights_for(H)
        kw = {}
        std_ext = std_t
        if fields is not None:
            kw["derived"] = fields
            derived_meta = derived_metadata(fields, decoded, std_t)
            std_ext = extended_scales(fields, std_t)
        for m in metrics:
            kw.update(m.rollout_kwargs(H, int(truth.shape[-1]), lat_w, std_ext))

        def score(path, time_str, t_slots, c_slots):
            return score_latent_rollout(path, model, mean_t, std_t, truth, t_slots, clim, c_slots, lat_w, sst_channel=args.sst_channel_idx,
                                        total_num_steps=total_num_steps, crop_init=args.crop_init, force_ens_size=args.force_ens_size,
                                        decode_batch_frames=args.decode_batch_frames, **kw)

    os.makedirs(args.output, exist_ok=True)
    gathered = {k: [] for k in SCORE_NAMES}
    for i, (time_str, path) in enumerate(files):
        print(f"processing time_str: {time_str}, remaining: {len(files) - i - 1}")
        init = _to_datetime(int(time_str))
        res = score(path, time_str, truth_frame_slots(init, args.start_date, args.step_size_hour, total_num_steps),
                    climatology_slots(init, args.total_lead_time_hour, args.step_size_hour, exclude_start=True))
        for k in SCORE_NAMES:
            a = np.asarray(res[k], dtype=np.float32)
            if a.ndim != 2 or a.shape[1] != total_num_steps:
                raise ValueError(f"{time_str}: {k} is {a.shape}, expected (C, {total_num_steps})")
            np.save(os.path.join(args.output, f"{time_str}_{k}.npy"), a)
            gathered[k].append(a)
        for m in metrics:
            m.gather(res, time_str)
    out = {k: np.stack(v) for k, v in gathered.items()}
    for m in metrics:
        m.finish(out, args.output)
    if fields is not None:
        with open(os.path.join(args.output, "derived.json"), "w") as f:
            json.dump(dict(decoded_channels=len(decoded), derived=derived_meta), f, indent=1)
    out["timestamp"] = np.array([int(t) for t, _ in files]).astype(np.float32)  # as the reference: a float32 tensor of YYYYMMDDHH
    for k, a in out.items():
        np.save(os.path.join(args.output, f"{k}.npy"), a)
    print(f"saved {len(files)} initial times x {out['crps'].shape[1]} channels x {total_num_steps} lead times to {args.output}")
    return out


if __name__ == "__main__":
    main()
