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
the south pole.  `--reliability` adds the spread-skill ratio and the rank histogram (`ldc_rollout_reliability`, not in the reference):
`ens_var.npy`, `ssr.npy`, `n_invalid.npy` (init time, C, lead time) and `rank_hist.npy`, `rank_hist_weighted.npy` (C, lead time, ens + 1).  `--spectrum` adds the zonal power spectra of the members, the ensemble
mean and the truth (`ldc_rollout_spectrum`, not in the reference): `spec_members.npy`, `spec_mean.npy`, `spec_truth.npy` (init time, C,
lead time, W / 2 + 1) and `spec_n_invalid.npy` (init time, C, lead time); `--spectrum_lat_band LO HI` keeps the rows between two latitudes.
`--event CHANNEL gt|lt VALUE` (any number of times; `--event_anomaly` the same on the value minus the climatology) verifies threshold
events (`ldc_rollout_events`, not in the reference): the histogram of "members showing the event" against "the truth showed it", pooled
over the initial times (`event_hist.npy`, `event_hist_weighted.npy` (E, lead time, ens + 1, 2)), `event_n_invalid.npy` (init time, E, lead
time), `events.json`, and from the pooled histogram `event_brier.npy`, `event_bss.npy`, `event_reliability.npy`, `event_resolution.npy`,
`event_uncertainty.npy`, `event_roc_area.npy` (E, lead time).
`--fss_scales R [R ...]` (with events) verifies the same events in neighbourhoods of (2 R + 1) x (2 R + 1) GRID POINTS (`ldc_rollout_fss`,
not in the reference; periodic in longitude, clipped at the poles, not corrected for the convergence of the meridians): the sums of the
fractions skill score pooled over the initial times (`event_fss_sums.npy` (E, scale, lead time, 6)), `event_fss.npy`,
`event_fss_target.npy`, `event_fss_obs_fraction.npy`, `event_fss_freq_bias.npy` (E, scale, lead time), `event_fss_useful_scale.npy` (E, lead
time: the smallest radius whose FSS reaches 0.5 + obs_fraction / 2, or -1), and `fss_radii` / `fss_width_deg` in `events.json`.
`--region NAME` (any number of times, from `NAMED_REGIONS`), `--region_box NAME LAT0 LAT1 LON0 LON1`, `--region_surface NAME land|sea`
(with `--land_sea_mask_path`) break the scores down by region (`ldc_rollout_regional`, not in the reference): every region in one pass
per decode batch, the additive sums pooled over the initial times (`regional_sums.npy` (R, C, lead time, 10), `regional_counts.npy`),
`regional_bias.npy`, `regional_rmse.npy`, `regional_crps.npy`, ... (R, C, lead time) derived from the pooled sums, and `regions.json`;
`--region_per_init` keeps the sums of every initial time too.
`--energy` adds the energy score (`ldc_rollout_energy`, not in the reference): the multivariate generalisation of the CRPS over whole
fields, per channel (`energy_score.npy`, `energy_score_fair.npy`, `energy_skill.npy`, `energy_spread.npy` (init time, C, lead time)
float64, `energy_n_invalid.npy` int32) and, with `--energy_group NAME CHANNEL [CHANNEL ...]` (any number of times; implies `--energy`),
per group of channels, each divided by its normalisation std (`energy_group_score.npy`, ... (init time, G, lead time)); `energy.json`
names the groups, their channels and the scales.  The score is not additive over initial times: pool it by its mean over them.
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
from .energy import ENERGY_GROUP_NAMES, ENERGY_NAMES, EnergyGroup, _group_list, empty_energy, inverse_scale2, rollout_energy
from .regional import (COUNT_NAMES, SUM_NAMES, REGIONAL_KEYS, REGIONAL_SCORE_NAMES, NAMED_REGIONS, Region, empty_regional, mask_words, region_mask as make_region_mask,
                       region_metadata, regional_scores, rollout_regional)
from .utils import (MAX_FSS_SCALES, SCORE_NAMES, SPECTRUM_NAMES, Event, _radius_list, empty_events, empty_fss, empty_reliability, empty_spectrum, event_scores,
                    fss_scores, get_normalized_lat_weights_based_on_cos, rollout_events, rollout_fss, rollout_reliability, rollout_scores,
                    rollout_spectrum)

SST_CHANNEL_IDX = 82
CLIMATOLOGY_HOURS = (0, 6, 12, 18)
RELIABILITY_KEYS = ("ens_var", "ssr", "rank_hist", "rank_hist_weighted", "n_invalid")  # what `--reliability` adds
SPECTRUM_KEYS = SPECTRUM_NAMES + ("spec_n_invalid",)  # what `--spectrum` adds
EVENTS_KEYS = ("event_hist", "event_hist_weighted", "event_n_invalid")  # what `--event` / `--event_anomaly` add to one initial time
FSS_KEYS = ("event_fss_sums", "event_fss_n_invalid")  # what `--fss_scales` adds to one initial time
FSS_FILE_SCORES = dict(event_fss="fss", event_fss_target="fss_target", event_fss_obs_fraction="obs_fraction",
                       event_fss_freq_bias="freq_bias")  # <file>.npy: the score of `fss_scores`, from the pooled sums
ENERGY_KEYS = ENERGY_NAMES + ("energy_n_invalid",)  # what `--energy` adds to one initial time; with groups also `ENERGY_GROUP_NAMES`
ENERGY_FILE_KEYS = ENERGY_NAMES[:4] + ("energy_n_invalid",)  # <key>.npy; the weights stay with the scorer's result
ENERGY_GROUP_FILE_KEYS = ENERGY_GROUP_NAMES[:4]
EVENT_FILE_SCORES = ("brier", "bss", "reliability", "resolution", "uncertainty", "roc_area")  # event_<name>.npy, from the pooled histogram


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
                         energy_groups: Optional[Sequence] = None, energy_scales=None) -> Dict[str, torch.Tensor]:
    """One initial time of evaluate_ens_gpu.py:268-425: a saved `latent_YYYYMMDDHH.npy` (or its (ens, C, T, h, w) tensor) -> the five
    (C, total_num_steps) fp32 CPU tensors `ens_acc`, `ens_mse`, `crps_spread`, `crps_skill`, `crps`.

    The T lead times are decoded lead-major, `max(1, decode_batch_frames // ens)` of them per decoder call (default: one, i.e. `ens`
    frames), and each decoder output is scored in place with the inverse normalisation (`mean_tensor` / `std_tensor`, one value per
    decoded channel) fused into the scorer: the peak memory for decoded fields is one decode batch.  truth / clim are (N, C, H, W)
    tables in physical units of which lead t reads entry `truth_slots[t]` / `clim_slots[t]` (clim None: no ACC).  On the device they
    are indexed where they are; host arrays or memmaps have only the planes this initial time needs staged to the device.  Columns
    T .. total_num_steps - 1 stay NaN, as the reference's `torch.full(nan)` leaves them; T > total_num_steps is a ValueError (the
    reference fails with an index error).  `crop_init` drops slot 0 (the IC latent), `force_ens_size` keeps the first members.

    `reliability`: every decode batch also goes through `ldc_rollout_reliability` while it is on the device (nothing more is decoded or
    kept) and the result gains `RELIABILITY_KEYS`: `ens_var`, `ssr` (C, total_num_steps) fp32, `rank_hist` (C, total_num_steps, ens + 1)
    int32, `rank_hist_weighted` the same in fp32, `n_invalid` (C, total_num_steps) int32; the five scores are the bits of a call without it.

    `spectrum`: every decode batch also goes through `ldc_rollout_spectrum` while it is on the device and the result gains
    `SPECTRUM_KEYS`: `spec_members`, `spec_mean`, `spec_truth` (C, total_num_steps, W / 2 + 1) fp32 and `spec_n_invalid` (C, total_num_steps)
    int32.  `spectrum_row_weight` (H,), non-negative, weights the rows (0: the row is left out and never read); default: `lat_weight`.  The
    five scores and the reliability outputs are the bits of a call without it.

    `events`: a sequence of `Event(channel, "gt" | "lt", threshold, anomaly)`; every decode batch also goes through `ldc_rollout_events`
    while it is on the device and the result gains `EVENTS_KEYS`: `event_hist` (E, total_num_steps, ens + 1, 2) int32, `event_hist_weighted`
    the same in fp32 and `event_n_invalid` (E, total_num_steps) int32 (`rollout_events`).  An anomaly event with `clim` None is a
    ValueError.  The five scores, the reliability outputs and the spectrum outputs are the bits of a call without it.

    `fss_radii`: with `events`, a sequence of neighbourhood radii in grid points; every decode batch also goes through `ldc_rollout_fss`
    while it is on the device and the result gains `FSS_KEYS`: `event_fss_sums` (E, S, total_num_steps, 6) float64 and
    `event_fss_n_invalid` (E, total_num_steps) int32 (`rollout_fss`; columns past the last lead time are zeros).  Without `events` it is a
    ValueError.  Every other output is the bits of a call without it.

    `regions`: a sequence of `Region` (or an int: their number), with `region_mask` the (H, W) uint32 mask of which bit r marks region
    r (`regional.region_mask`; default: built from `regions` on `row_latitudes(H)` and the longitudes 0, 360 / W, ...); every decode
    batch also goes through one `ldc_rollout_regional` launch while it is on the device and the result gains `REGIONAL_KEYS`:
    `regional_sums` (R, C, total_num_steps, 10) float64 and `regional_counts` (R, C, total_num_steps, 3) int32 (`rollout_regional`;
    columns past the last lead time are zeros).  Every other output is the bits of a call without it.

    `energy`: every decode batch also goes through `ldc_rollout_energy` while it is on the device and the result gains `ENERGY_KEYS`:
    `energy_score`, `energy_score_fair`, `energy_skill`, `energy_spread`, `energy_weight` (C, total_num_steps) float64 and
    `energy_n_invalid` (C, total_num_steps) int32 (`rollout_energy`; columns past the last lead time are NaN).  `energy_groups`: a
    sequence of `EnergyGroup(name, channels)` (implies `energy`); the result then gains `ENERGY_GROUP_NAMES` too, (G, total_num_steps)
    float64.  `energy_scales` (C',), positive and finite, divides each channel of a group; default: `std_tensor`.  Up to 256 members;
    the limits of the other scores stand.  Every other output is the bits of a call without it."""
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
    events = [Event(*ev) for ev in events] if events else None
    if events and clim is None and any(ev.anomaly for ev in events):
        raise ValueError("an anomaly event needs the climatology (clim)")
    if fss_radii is not None and not events:
        raise ValueError("fss_radii needs events: the neighbourhood scores verify threshold events")
    fss_radii = None if fss_radii is None else list(fss_radii)
    n_regions = 0
    if regions is not None or region_mask is not None:
        if regions is None:
            raise ValueError("region_mask needs regions (the Region list, or their number)")
        n_regions = int(regions) if isinstance(regions, (int, np.integer)) else len(regions)
        if not 1 <= n_regions <= 32:
            raise ValueError(f"{n_regions} regions: ldc_rollout_regional takes 1 .. 32 per call")
        if region_mask is None and isinstance(regions, (int, np.integer)):
            raise ValueError("a number of regions needs the region_mask")
    energy = bool(energy) or bool(energy_groups)
    if energy_scales is not None and not energy_groups:
        raise ValueError("energy_scales needs energy_groups: the scales divide the channels of a group")
    en_groups = None  # resolved against the decoded channel count at the first batch
    if energy_groups:  # malformed groups and scales raise before anything is decoded; the channel range is checked at the first batch
        _group_list(energy_groups, 1 << 31)
        if energy_scales is not None:
            inverse_scale2(energy_scales, torch.as_tensor(energy_scales).numel())
    dev = encdec_model.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("ladcast_amd scoring needs the model on the device (no CPU fallback)")
    t_slots, c_slots = list(truth_slots[:T]), None if clim is None else list(clim_slots[:T])
    if not (isinstance(truth, torch.Tensor) and truth.is_cuda):
        truth, t_slots = _stage_planes(truth, t_slots, dev, "truth")
    if clim is not None and not (isinstance(clim, torch.Tensor) and clim.is_cuda):
        clim, c_slots = _stage_planes(clim, c_slots, dev, "clim")
    mean_d, std_d = _device_vector(mean_tensor, dev), _device_vector(std_tensor, dev)
    lat_weight = lat_weight.to(dev, torch.float32)
    latents = latents.to(dev, torch.float32)
    if spectrum:
        spec_w = lat_weight if spectrum_row_weight is None else spectrum_row_weight
        if not spec_w.is_cuda and not bool((spec_w >= 0).all()):
            raise ValueError("spectrum_row_weight must be non-negative (0 leaves a row out) and not NaN")
        spec_w = spec_w.to(dev, torch.float32)
    per = max(1, int(decode_batch_frames) // ens) if decode_batch_frames else 1  # lead times per decoder call: a lead time's members stay together
    scores = rel = spec = evs = fss = reg = reg_words = en = None
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        x = latents[:, :, s0 : s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ens, C, h, w).contiguous()  # lead-major, then member
        y = encdec_model.decode(x).sample  # (nl * ens, C', H, W), still normalised
        if scores is None:
            scores = torch.full((5, y.shape[1], total), float("nan"), device=dev, dtype=torch.float32)
        rollout_scores(y.reshape(nl, ens, *y.shape[1:]), truth, clim, lat_weight, sst_channel, lead_dim=0, mean=mean_d, std=std_d,
                       truth_slots=t_slots[s0 : s0 + nl], clim_slots=None if clim is None else c_slots[s0 : s0 + nl], out=scores, lead_offset=s0)
        if reliability:
            if rel is None:
                rel = empty_reliability(ens, y.shape[1], total, dev)
            rollout_reliability(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, sst_channel, lead_dim=0, mean=mean_d, std=std_d,
                                truth_slot=t_slots[s0 : s0 + nl], out=rel, l_off=s0)
        if spectrum:
            if spec is None:
                spec = empty_spectrum(y.shape[1], total, y.shape[3], dev)
            rollout_spectrum(y.reshape(nl, ens, *y.shape[1:]), truth, spec_w, lead_dim=0, mean=mean_d, std=std_d,
                             truth_slot=t_slots[s0 : s0 + nl], out=spec, l_off=s0)
        if events:
            if evs is None:
                evs = empty_events(ens, len(events), total, dev)
            rollout_events(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, events, clim=clim,
                           clim_slots=None if clim is None else c_slots[s0 : s0 + nl], lead_dim=0, mean=mean_d, std=std_d,
                           truth_slot=t_slots[s0 : s0 + nl], out=evs, l_off=s0)
        if fss_radii is not None:
            if fss is None:
                fss = empty_fss(len(events), len(_radius_list(fss_radii, y.shape[3])), total, dev)
            rollout_fss(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, events, fss_radii, clim=clim,
                        clim_slots=None if clim is None else c_slots[s0 : s0 + nl], lead_dim=0, mean=mean_d, std=std_d,
                        truth_slot=t_slots[s0 : s0 + nl], out=fss, l_off=s0)
        if n_regions:
            if reg is None:
                Hd, Wd = y.shape[2], y.shape[3]
                if region_mask is None:
                    region_mask = make_region_mask(regions, row_latitudes(Hd), np.arange(Wd) * (360.0 / Wd))
                reg_words = region_mask if isinstance(region_mask, torch.Tensor) and region_mask.is_cuda else mask_words(region_mask, Hd, Wd).to(dev)
                reg = empty_regional(n_regions, y.shape[1], total, dev)
            rollout_regional(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, reg_words, n_regions, clim=clim,
                             clim_slots=None if clim is None else c_slots[s0 : s0 + nl], lead_dim=0, mean=mean_d, std=std_d,
                             truth_slot=t_slots[s0 : s0 + nl], out=reg, l_off=s0)
        if energy:
            if en is None:
                Cd = y.shape[1]
                en_groups = _group_list(energy_groups, Cd)
                if en_groups and energy_scales is None:
                    energy_scales = std_tensor
                en = empty_energy(ens, Cd, len(en_groups), total, dev)
            rollout_energy(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, groups=en_groups, scales=energy_scales if en_groups else None,
                           lead_dim=0, mean=mean_d, std=std_d, truth_slot=t_slots[s0 : s0 + nl], out=en, l_off=s0)
    host = scores.cpu()  # the one copy (and the one wait) of this initial time
    res = {k: host[i] for i, k in enumerate(SCORE_NAMES)}
    if reliability:
        res.update({k: rel[k].cpu() for k in RELIABILITY_KEYS})
    if spectrum:
        res.update({k: spec[k].cpu() for k in SPECTRUM_NAMES}, spec_n_invalid=spec["n_invalid"].cpu())
    if events:
        res.update({k: evs[k].cpu() for k in EVENTS_KEYS})
    if fss is not None:
        res.update({k: fss[k].cpu() for k in FSS_KEYS})
    if n_regions:
        res.update({k: reg[k].cpu() for k in REGIONAL_KEYS})
    if energy:
        res.update({k: en[k].cpu() for k in ENERGY_KEYS + (ENERGY_GROUP_NAMES if en_groups else ())})
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


def _crop_rows(table: np.ndarray, H: int, what: str) -> np.ndarray:
    """(..., H_in, W) -> the H rows the decoder produces: H_in == H + 1 drops row 0, the south pole (a view: a memmap stays on disk)"""
    H_in = table.shape[-2]
    if H_in == H + 1:
        return table[..., 1:, :]
    if H_in != H:
        raise ValueError(f"{what} has {H_in} rows; the decoded fields have {H} (or {H + 1} with the south pole)")
    return table


def _gather_reliability(rel: dict, res, time_str: str, total_num_steps: int) -> None:
    """one initial time's `RELIABILITY_KEYS` into the run's: `ens_var`, `ssr` (fp32) and `n_invalid` (int32) are kept per initial time,
    the rank histograms are summed over the initial times on the host - the counts in int64, the weighted ones in float64"""
    missing = [k for k in RELIABILITY_KEYS if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --reliability needs {missing} from the scorer")
    a = {k: np.asarray(res[k]) for k in RELIABILITY_KEYS}
    C = a["ens_var"].shape[0]
    hist_shape = a["rank_hist"].shape
    if any(a[k].shape != (C, total_num_steps) for k in ("ens_var", "ssr", "n_invalid")) or len(hist_shape) != 3 \
            or hist_shape[:2] != (C, total_num_steps) or a["rank_hist_weighted"].shape != hist_shape:
        raise ValueError(f"{time_str}: reliability arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {total_num_steps}) "
                         f"and (C, {total_num_steps}, members + 1)")
    if rel["rank_hist"] is None:
        rel["rank_hist"], rel["rank_hist_weighted"] = np.zeros(hist_shape, dtype=np.int64), np.zeros(hist_shape, dtype=np.float64)
    elif rel["rank_hist"].shape != hist_shape:
        raise ValueError(f"{time_str}: a rank histogram of {hist_shape[2] - 1} members after one of {rel['rank_hist'].shape[2] - 1}")
    rel["ens_var"].append(a["ens_var"].astype(np.float32))
    rel["ssr"].append(a["ssr"].astype(np.float32))
    rel["n_invalid"].append(a["n_invalid"].astype(np.int32))
    rel["rank_hist"] += a["rank_hist"].astype(np.int64)
    rel["rank_hist_weighted"] += a["rank_hist_weighted"].astype(np.float64)


def _gather_spectrum(spec: dict, res, time_str: str, total_num_steps: int) -> None:
    """one initial time's `SPECTRUM_KEYS` into the run's: kept per initial time, the spectra in fp32, `spec_n_invalid` in int32"""
    missing = [k for k in SPECTRUM_KEYS if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --spectrum needs {missing} from the scorer")
    a = {k: np.asarray(res[k]) for k in SPECTRUM_KEYS}
    shape = a[SPECTRUM_NAMES[0]].shape
    if len(shape) != 3 or shape[1] != total_num_steps or any(a[k].shape != shape for k in SPECTRUM_NAMES) or a["spec_n_invalid"].shape != shape[:2]:
        raise ValueError(f"{time_str}: spectrum arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {total_num_steps}, K) "
                         f"and (C, {total_num_steps})")
    for k in SPECTRUM_NAMES:
        spec[k].append(a[k].astype(np.float32))
    spec["spec_n_invalid"].append(a["spec_n_invalid"].astype(np.int32))


def _gather_events(evs: dict, res, time_str: str, total_num_steps: int, E: int) -> None:
    """one initial time's `EVENTS_KEYS` into the run's: `event_n_invalid` (int32) is kept per initial time, the histograms are summed over
    the initial times on the host - the counts in int64, the weighted ones in float64"""
    missing = [k for k in EVENTS_KEYS if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --event needs {missing} from the scorer")
    a = {k: np.asarray(res[k]) for k in EVENTS_KEYS}
    shape = a["event_hist"].shape
    if len(shape) != 4 or shape[:2] != (E, total_num_steps) or shape[3] != 2 or a["event_hist_weighted"].shape != shape \
            or a["event_n_invalid"].shape != (E, total_num_steps):
        raise ValueError(f"{time_str}: event arrays of shapes { {k: v.shape for k, v in a.items()} }, expected ({E}, {total_num_steps}, "
                         f"members + 1, 2) and ({E}, {total_num_steps})")
    if evs["event_hist"] is None:
        evs["event_hist"], evs["event_hist_weighted"] = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.float64)
    elif evs["event_hist"].shape != shape:
        raise ValueError(f"{time_str}: an event histogram of {shape[2] - 1} members after one of {evs['event_hist'].shape[2] - 1}")
    evs["event_n_invalid"].append(a["event_n_invalid"].astype(np.int32))
    evs["event_hist"] += a["event_hist"].astype(np.int64)
    evs["event_hist_weighted"] += a["event_hist_weighted"].astype(np.float64)


def _gather_fss(fss: dict, res, time_str: str, total_num_steps: int, E: int, S: int) -> None:
    """one initial time's `FSS_KEYS` into the run's: the sums are added over the initial times on the host in float64,
    `event_fss_n_invalid` (int32) is kept per initial time"""
    missing = [k for k in FSS_KEYS if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --fss_scales needs {missing} from the scorer")
    s, n = np.asarray(res["event_fss_sums"], dtype=np.float64), np.asarray(res["event_fss_n_invalid"])
    if s.shape != (E, S, total_num_steps, 6) or n.shape != (E, total_num_steps):
        raise ValueError(f"{time_str}: fss arrays of shapes {s.shape} and {n.shape}, expected ({E}, {S}, {total_num_steps}, 6) and "
                         f"({E}, {total_num_steps})")
    fss["event_fss_sums"] = s.copy() if fss["event_fss_sums"] is None else fss["event_fss_sums"] + s
    fss["event_fss_n_invalid"].append(n.astype(np.int32))


def parse_fss_scales(values) -> List[int]:
    """`--fss_scales R [R ...]` -> the radii in grid points as given: 1 .. 16 whole numbers >= 0, no two equal (that they fit the
    grid, 2 R + 1 <= W, is checked where W is known: `rollout_fss`)"""
    try:
        radii = [int(str(v)) for v in values]
    except ValueError:
        raise ValueError(f"--fss_scales {' '.join(map(str, values))}: the radii are whole numbers of grid points") from None
    if not 1 <= len(radii) <= MAX_FSS_SCALES:
        raise ValueError(f"--fss_scales: {len(radii)} radii, 1 .. {MAX_FSS_SCALES} are served")
    if any(r < 0 for r in radii):
        raise ValueError(f"--fss_scales {radii}: a radius must not be negative")
    if len(set(radii)) != len(radii):
        raise ValueError(f"--fss_scales {radii}: the radii must differ")
    return radii


def _gather_regional(regs: dict, res, time_str: str, total_num_steps: int, R: int, per_init: bool) -> None:
    """one initial time's `REGIONAL_KEYS` into the run's: summed over the initial times on the host, the sums in float64 and the counts in
    int64; `per_init` also keeps each initial time's sums"""
    missing = [k for k in REGIONAL_KEYS if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --region needs {missing} from the scorer")
    s, n = np.asarray(res["regional_sums"], dtype=np.float64), np.asarray(res["regional_counts"]).astype(np.int64)
    if s.ndim != 4 or s.shape[0] != R or s.shape[2:] != (total_num_steps, 10) or n.shape != s.shape[:3] + (3,):
        raise ValueError(f"{time_str}: regional arrays of shapes {s.shape} and {n.shape}, expected ({R}, C, {total_num_steps}, 10) and "
                         f"({R}, C, {total_num_steps}, 3)")
    if regs["regional_sums"] is None:
        regs["regional_sums"], regs["regional_counts"] = np.zeros(s.shape, dtype=np.float64), np.zeros(n.shape, dtype=np.int64)
    elif regs["regional_sums"].shape != s.shape:
        raise ValueError(f"{time_str}: regional sums of shape {s.shape} after {regs['regional_sums'].shape}")
    regs["regional_sums"] += s
    regs["regional_counts"] += n
    if per_init:
        regs["per_init"].append(s)


def _gather_energy(en: dict, res, time_str: str, total_num_steps: int, G: int) -> None:
    """one initial time's `ENERGY_FILE_KEYS` (and with groups `ENERGY_GROUP_FILE_KEYS`) into the run's: kept per initial time, float64
    (`energy_n_invalid`: int32) - the score is not additive over initial times"""
    keys = ENERGY_FILE_KEYS + (ENERGY_GROUP_FILE_KEYS if G else ())
    missing = [k for k in keys if k not in res]
    if missing:
        raise ValueError(f"{time_str}: --energy needs {missing} from the scorer")
    a = {k: np.asarray(res[k]) for k in keys}
    C = a["energy_score"].shape[0]
    if any(a[k].shape != (C, total_num_steps) for k in ENERGY_FILE_KEYS) or any(a[k].shape != (G, total_num_steps) for k in keys[len(ENERGY_FILE_KEYS):]):
        raise ValueError(f"{time_str}: energy arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {total_num_steps}) and "
                         f"({G}, {total_num_steps})")
    for k in keys:
        en.setdefault(k, []).append(a[k].astype(np.int32 if k == "energy_n_invalid" else np.float64))


def parse_energy_groups(entries: Sequence[Sequence[str]], names: Sequence[str]) -> List[EnergyGroup]:
    """`--energy_group NAME CHANNEL [CHANNEL ...]` entries -> the `EnergyGroup` list; CHANNEL is a name of `names` or an index, resolved
    as `--event` resolves it"""
    from .products import resolve_channels

    groups = []
    for entry in entries:
        if len(entry) < 2:
            raise ValueError(f"--energy_group {' '.join(entry)}: a name and at least one channel are needed")
        groups.append(EnergyGroup(entry[0], tuple(resolve_channels(list(entry[1:]), names))))
    return _group_list(groups, len(names))


def parse_regions(region: Sequence[str], region_box: Sequence[Sequence[str]], region_surface: Sequence[Sequence[str]]) -> List[Region]:
    """`--region NAME`, `--region_box NAME LAT0 LAT1 LON0 LON1` and `--region_surface NAME land|sea` entries -> the `Region` list, named
    regions first; a surface applies to the region of that name"""
    regions: List[Region] = []
    for name in region:
        if name not in NAMED_REGIONS:
            raise ValueError(f"--region {name}: not one of {sorted(NAMED_REGIONS)}")
        regions.append(NAMED_REGIONS[name])
    for name, *box in region_box:
        try:
            lat0, lat1, lon0, lon1 = (float(v) for v in box)
        except ValueError:
            raise ValueError(f"--region_box {name} {' '.join(box)}: four numbers are needed") from None
        if not all(np.isfinite([lat0, lat1, lon0, lon1])) or lat0 > lat1:
            raise ValueError(f"--region_box {name} {' '.join(box)}: finite bounds with LAT0 <= LAT1 are needed")
        regions.append(Region(name, lat0, lat1, lon0, lon1))
    names = [r.name for r in regions]
    if len(set(names)) != len(names):
        raise ValueError(f"region names must differ, got {names}")
    for name, surface in region_surface:
        if surface not in ("land", "sea"):
            raise ValueError(f"--region_surface {name} {surface}: the surface is land or sea")
        if name not in names:
            raise ValueError(f"--region_surface {name}: no such region among {names}")
        regions[names.index(name)] = regions[names.index(name)]._replace(surface=surface)
    if len(regions) > 32:
        raise ValueError(f"{len(regions)} regions: at most 32 per run")
    return regions


def parse_events(event: Sequence[Sequence[str]], event_anomaly: Sequence[Sequence[str]], names: Sequence[str]):
    """`--event` / `--event_anomaly CHANNEL gt|lt VALUE` entries -> (the `Event` list, plain events first; the entries as they go into
    events.json, with the resolved channel names)"""
    from .products import DIRECTIONS, resolve_channels

    events, meta = [], []
    for entries, anomaly in ((event, False), (event_anomaly, True)):
        for chan, direction, value in entries:
            flag = "--event_anomaly" if anomaly else "--event"
            c = resolve_channels([chan], names)[0]
            if direction not in DIRECTIONS:
                raise ValueError(f"{flag} {chan} {direction}: the direction is gt or lt")
            thr = float(value)
            if thr != thr:
                raise ValueError(f"{flag} {chan} {direction} {value}: the threshold must not be NaN")
            events.append(Event(c, direction, thr, anomaly))
            meta.append(dict(channel=names[c], channel_index=c, direction=direction, threshold=thr, anomaly=anomaly))
    return events, meta


def spectrum_band_weights(lat_weight: torch.Tensor, lat_deg, band) -> torch.Tensor:
    """`lat_weight` (H,) with the rows whose latitude `lat_deg` (H,) lies outside [band[0], band[1]] degrees set to 0; band None: unchanged"""
    if band is None:
        return lat_weight
    lo, hi = float(band[0]), float(band[1])
    if not lo <= hi:
        raise ValueError(f"--spectrum_lat_band {lo} {hi}: LO must not exceed HI")
    lat = torch.as_tensor(np.asarray(lat_deg, dtype=np.float64))
    inside = (lat >= lo) & (lat <= hi)
    if not bool(inside.any()):
        raise ValueError(f"--spectrum_lat_band {lo} {hi}: no latitude row inside (rows from {float(lat.min())} to {float(lat.max())})")
    return torch.where(inside, lat_weight, torch.zeros_like(lat_weight))


def row_latitudes(H: int) -> np.ndarray:
    """the latitudes in degrees of the H rows `lat_weights_for` weighs: the 120-row grid's, else the H rows kept of an equiangular
    pole-to-pole grid of H + 1 (row 0, the south pole, dropped)"""
    return np.linspace(-88.5, 90, 120) if H == 120 else np.linspace(-90.0, 90.0, H + 1)[1:]


def main(argv=None, score: Optional[Callable] = None):
    """`score(path, time_str, truth_slots, clim_slots) -> {name: (C, total_num_steps)}` replaces the autoencoder, the data and the device
    (tests of the file handling).  Returns the gathered arrays, `timestamp` among them.

    `--reliability` (the scorer then returns `RELIABILITY_KEYS` too) adds `ens_var.npy`, `ssr.npy` (init time, C, lead time) fp32,
    `n_invalid.npy` the same in int32, and the rank histograms summed over the initial times: `rank_hist.npy` (C, lead time, members + 1)
    int64 and `rank_hist_weighted.npy` float64.  Without it the launches and the files are those of a run before the flag existed.

    `--spectrum` (the scorer then returns `SPECTRUM_KEYS` too) adds `spec_members.npy`, `spec_mean.npy`, `spec_truth.npy` (init time, C,
    lead time, W / 2 + 1) fp32 and `spec_n_invalid.npy` (init time, C, lead time) int32; `--spectrum_lat_band LO HI` (degrees) gives the
    rows outside the band weight 0, the rows inside keep the cos weight.

    `--event CHANNEL gt|lt VALUE` and `--event_anomaly CHANNEL gt|lt VALUE` (each any number of times; CHANNEL a name of
    `products.column_names` or an index; the scorer then returns `EVENTS_KEYS` too, plain events first) add `event_hist.npy` (E, lead time,
    members + 1, 2) int64 and `event_hist_weighted.npy` float64, summed over the initial times, `event_n_invalid.npy` (init time, E, lead
    time) int32, `events.json` (the events as given, with resolved channel names) and `event_brier.npy`, `event_bss.npy`,
    `event_reliability.npy`, `event_resolution.npy`, `event_uncertainty.npy`, `event_roc_area.npy` (E, lead time) float64: `event_scores`
    of the pooled weighted histogram.  Without the flags the launches and the files are those of a run before they existed.

    `--fss_scales R [R ...]` (needs an event flag; the scorer then returns `FSS_KEYS` too) adds `event_fss_sums.npy` (E, scale, lead time, 6)
    float64, summed over the initial times, `event_fss_n_invalid.npy` (init time, E, lead time) int32, `event_fss.npy`,
    `event_fss_target.npy`, `event_fss_obs_fraction.npy`, `event_fss_freq_bias.npy` (E, scale, lead time) and `event_fss_useful_scale.npy`
    (E, lead time) int64: `fss_scores` of the pooled sums; `events.json` gains `fss_radii` (grid points) and `fss_width_deg` (the
    window's width (2 R + 1) 360 / W in degrees of longitude and latitude; in kilometres it shrinks towards the poles).

    `--region NAME` (from `NAMED_REGIONS`), `--region_box NAME LAT0 LAT1 LON0 LON1` (each any number of times; named regions first) and
    `--region_surface NAME land|sea` with `--land_sea_mask_path` (.npy (H_in, W), land where >= 0.5; rows cropped as the truth's) make
    the scorer return `REGIONAL_KEYS` too.  The sums are pooled over the initial times on the host (float64, counts in int64):
    `regional_sums.npy` (R, C, lead time, 10), `regional_counts.npy` (R, C, lead time, 3), `regional_<score>.npy` (R, C, lead time) for
    `REGIONAL_SCORE_NAMES` from the pooled sums (`regional_scores`) and `regions.json` (names, boxes, surface, point count and weight of
    each region).  `--region_per_init` also writes `regional_sums_per_init.npy` (init time, R, C, lead time, 10): off by default, at a
    year of initial times, 84 channels and 13 regions it runs to gigabytes.  Without the flags the launches and files are unchanged.

    `--energy` (the scorer then returns `ENERGY_KEYS` too) adds `energy_score.npy`, `energy_score_fair.npy`, `energy_skill.npy`,
    `energy_spread.npy` (init time, C, lead time) float64 and `energy_n_invalid.npy` int32; `--energy_group NAME CHANNEL [CHANNEL ...]`
    (any number of times, CHANNEL resolved as `--event` resolves it; implies `--energy`; the scorer then returns `ENERGY_GROUP_NAMES`
    too) adds `energy_group_score.npy`, `energy_group_score_fair.npy`, `energy_group_skill.npy`, `energy_group_spread.npy` (init time, G,
    lead time) float64, every channel of a group divided by its normalisation std; `energy.json` holds the group names, channels and
    scales.  The energy score is not additive over initial times: the pooled value is the mean over the first axis, taken by the
    reader.  Without the flags the launches and files are unchanged.

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
    ap.add_argument("--reliability", action="store_true", help="also write ens_var, ssr, rank_hist, rank_hist_weighted and n_invalid")
    ap.add_argument("--spectrum", action="store_true", help="also write spec_members, spec_mean, spec_truth and spec_n_invalid")
    ap.add_argument("--spectrum_lat_band", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                    help="latitudes in degrees between which rows enter the spectra (default: all rows)")
    ap.add_argument("--event", nargs=3, action="append", default=[], metavar=("CHANNEL", "gt|lt", "VALUE"),
                    help="verify the event 'CHANNEL above (gt) / below (lt) VALUE' (physical units); may be given several times")
    ap.add_argument("--event_anomaly", nargs=3, action="append", default=[], metavar=("CHANNEL", "gt|lt", "VALUE"),
                    help="the same on CHANNEL minus its climatology")
    ap.add_argument("--fss_scales", nargs="+", default=None, metavar="R",
                    help="also verify the events in neighbourhoods of (2 R + 1) x (2 R + 1) grid points (fractions skill score); needs --event / --event_anomaly")
    ap.add_argument("--region", action="append", default=[], metavar="NAME", help="break the scores down by this named region; may be given several times")
    ap.add_argument("--region_box", nargs=5, action="append", default=[], metavar=("NAME", "LAT0", "LAT1", "LON0", "LON1"),
                    help="a region of your own: latitudes LAT0 .. LAT1 (inclusive), longitudes LON0 .. LON1 east (LON0 > LON1: across 0 degrees)")
    ap.add_argument("--region_surface", nargs=2, action="append", default=[], metavar=("NAME", "land|sea"),
                    help="restrict the region NAME to land or sea points (needs --land_sea_mask_path)")
    ap.add_argument("--land_sea_mask_path", type=str, default=None, help=".npy (H_in, W): land where >= 0.5")
    ap.add_argument("--region_per_init", action="store_true", help="also write regional_sums_per_init.npy (init time, R, C, lead time, 10)")
    ap.add_argument("--energy", action="store_true", help="also write the energy score per channel: energy_score, energy_score_fair, energy_skill, energy_spread, energy_n_invalid")
    ap.add_argument("--energy_group", nargs="+", action="append", default=[], metavar="NAME_THEN_CHANNELS",
                    help="NAME CHANNEL [CHANNEL ...]: also score these channels together, each divided by its normalisation std; may be given several times; implies --energy")
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

    events, events_meta = [], []
    if args.event or args.event_anomaly:
        from .validate_AR import column_names

        events, events_meta = parse_events(args.event, args.event_anomaly, column_names(args.variable_names, args.levels, args.num_atm_vars))

    fss_radii = None
    if args.fss_scales is not None:
        if not events:
            raise ValueError("--fss_scales needs --event or --event_anomaly")
        fss_radii = parse_fss_scales(args.fss_scales)
    grid_w = None  # points per row, where the data tell it

    energy_groups, energy_names = [], None
    if args.energy_group:
        from .validate_AR import column_names

        energy_names = column_names(args.variable_names, args.levels, args.num_atm_vars)
        energy_groups = parse_energy_groups(args.energy_group, energy_names)
    want_energy = args.energy or bool(energy_groups)
    energy_scales = None

    regions = parse_regions(args.region, args.region_box, args.region_surface)
    if any(r.surface for r in regions) and args.land_sea_mask_path is None:
        raise ValueError("--region_surface needs --land_sea_mask_path")
    if not regions and (args.region_per_init or args.land_sea_mask_path or args.region_surface):
        raise ValueError("--region_per_init, --region_surface and --land_sea_mask_path need --region or --region_box")
    regions_meta = None

    def build_region_mask(H: int, W: int, lat_w):
        lsm = None
        if args.land_sea_mask_path is not None:
            lsm = np.load(args.land_sea_mask_path)
            if lsm.ndim != 2:
                raise ValueError(f"--land_sea_mask_path must be (H_in, W), got {lsm.shape}")
            lsm = _crop_rows(lsm, H, "--land_sea_mask_path")
        mask = make_region_mask(regions, row_latitudes(H), np.arange(W) * (360.0 / W), lsm)
        return mask, region_metadata(regions, mask, lat_w)

    if score is None:
        if args.encdec_model is None or args.data_path is None or args.climatology_path is None:
            raise SystemExit("--encdec_model, --data_path and --climatology_path are required")
        with open(args.normalization_json) as f:
            mean_t, std_t = mean_std_from_json(json.load(f), args.variable_names)
        if energy_groups:
            energy_scales = [float(v) for v in torch.as_tensor(std_t).reshape(-1).tolist()]
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
        grid_w = int(truth.shape[-1])
        lat_w = lat_weights_for(H)
        spec_w = spectrum_band_weights(lat_w, row_latitudes(H), args.spectrum_lat_band) if args.spectrum else None
        reg_mask = None
        if regions:
            reg_mask, regions_meta = build_region_mask(H, truth.shape[-1], lat_w.numpy())

        def score(path, time_str, t_slots, c_slots):
            return score_latent_rollout(path, model, mean_t, std_t, truth, t_slots, clim, c_slots, lat_w, sst_channel=args.sst_channel_idx,
                                        total_num_steps=total_num_steps, crop_init=args.crop_init, force_ens_size=args.force_ens_size,
                                        decode_batch_frames=args.decode_batch_frames, reliability=args.reliability, spectrum=args.spectrum,
                                        spectrum_row_weight=spec_w, events=events or None, regions=regions or None, region_mask=reg_mask,
                                        fss_radii=fss_radii, energy=want_energy, energy_groups=energy_groups or None)

    os.makedirs(args.output, exist_ok=True)
    gathered = {k: [] for k in SCORE_NAMES}
    rel = dict(ens_var=[], ssr=[], n_invalid=[], rank_hist=None, rank_hist_weighted=None)
    spec = {k: [] for k in SPECTRUM_KEYS}
    evs = dict(event_n_invalid=[], event_hist=None, event_hist_weighted=None)
    fss = dict(event_fss_sums=None, event_fss_n_invalid=[])
    regs = dict(regional_sums=None, regional_counts=None, per_init=[])
    engy: dict = {}
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
        if args.reliability:
            _gather_reliability(rel, res, time_str, total_num_steps)
        if args.spectrum:
            _gather_spectrum(spec, res, time_str, total_num_steps)
        if events:
            _gather_events(evs, res, time_str, total_num_steps, len(events))
        if fss_radii is not None:
            _gather_fss(fss, res, time_str, total_num_steps, len(events), len(fss_radii))
        if regions:
            _gather_regional(regs, res, time_str, total_num_steps, len(regions), args.region_per_init)
        if want_energy:
            _gather_energy(engy, res, time_str, total_num_steps, len(energy_groups))
    out = {k: np.stack(v) for k, v in gathered.items()}
    if args.reliability:
        out.update({k: np.stack(rel[k]) for k in ("ens_var", "ssr", "n_invalid")}, rank_hist=rel["rank_hist"], rank_hist_weighted=rel["rank_hist_weighted"])
    if args.spectrum:
        out.update({k: np.stack(v) for k, v in spec.items()})
    if events:
        out.update(event_n_invalid=np.stack(evs["event_n_invalid"]), event_hist=evs["event_hist"], event_hist_weighted=evs["event_hist_weighted"])
        sc = event_scores(evs["event_hist_weighted"])
        out.update({f"event_{k}": np.asarray(sc[k], dtype=np.float64) for k in EVENT_FILE_SCORES})
        meta = dict(events=events_meta)
        if fss_radii is not None:
            out.update(event_fss_sums=fss["event_fss_sums"], event_fss_n_invalid=np.stack(fss["event_fss_n_invalid"]))
            sc = fss_scores(fss["event_fss_sums"], fss_radii)
            out.update({name: np.asarray(sc[k], dtype=np.float64) for name, k in FSS_FILE_SCORES.items()},
                       event_fss_useful_scale=np.asarray(sc["useful_scale"], dtype=np.int64))
            meta.update(fss_radii=fss_radii, fss_width_deg=None if grid_w is None else [(2 * r + 1) * 360.0 / grid_w for r in fss_radii])
        with open(os.path.join(args.output, "events.json"), "w") as f:
            json.dump(meta, f, indent=1)
    if regions:
        out.update(regional_sums=regs["regional_sums"], regional_counts=regs["regional_counts"])
        ens = int(np.load(files[0][1], mmap_mode="r").shape[0])  # the members the sums were taken over: the ssr's (M + 1) / M
        ens = ens if args.force_ens_size is None else min(ens, args.force_ens_size)
        sc = regional_scores(regs["regional_sums"], regs["regional_counts"], ens)
        out.update({f"regional_{k}": np.asarray(sc[k]) for k in REGIONAL_SCORE_NAMES})
        if args.region_per_init:
            out["regional_sums_per_init"] = np.stack(regs["per_init"])
        if regions_meta is None:  # an injected scorer: the mask of the pooled arrays' grid is not known here
            regions_meta = [dict(name=r.name, boxes=[[r.lat_min, r.lat_max, r.lon_min, r.lon_max]] + [list(b) for b in r.boxes], surface=r.surface,
                                 n_points=None, weight=None) for r in regions]
        with open(os.path.join(args.output, "regions.json"), "w") as f:
            json.dump(dict(regions=regions_meta, members=ens, sums=list(SUM_NAMES), counts=list(COUNT_NAMES)), f, indent=1)
    if want_energy:
        out.update({k: np.stack(v) for k, v in engy.items()})
        with open(os.path.join(args.output, "energy.json"), "w") as f:
            json.dump(dict(groups=[dict(name=g.name, channels=list(g.channels),
                                        channel_names=None if energy_names is None else [energy_names[c] for c in g.channels],
                                        scales=None if energy_scales is None else [energy_scales[c] for c in g.channels]) for g in energy_groups]),
                      f, indent=1)
    out["timestamp"] = np.array([int(t) for t, _ in files]).astype(np.float32)  # as the reference: a float32 tensor of YYYYMMDDHH
    for k, a in out.items():
        np.save(os.path.join(args.output, f"{k}.npy"), a)
    print(f"saved {len(files)} initial times x {out['crps'].shape[1]} channels x {total_num_steps} lead times to {args.output}")
    return out


if __name__ == "__main__":
    main()
