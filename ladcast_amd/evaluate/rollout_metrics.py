"""The optional metrics of the rollout-scoring driver (`evaluate_ens_gpu`), one object each; `METRICS` fixes their order: that of the
launches inside a decode batch and of the keys of a result.  Device half, used by `score_latent_rollout`: `for_rollout(options)` checks
the options before anything is decoded, `start` runs once the device tensors exist, `run(batch)` allocates the result at the first batch,
when the decoded C', H, W are known, and launches, `result()` copies it to the host.  Host half, used by `main`, which an injected scorer
can drive without a device: `add_arguments`, `from_args`, `rollout_kwargs` (the keywords for `score_latent_rollout`), `gather(res, time_str)`
(missing keys, shapes, then pooled or appended), `finish(out, output)` (arrays and JSON file).  A class states what its option adds to one
initial time's result (T = total_num_steps) and what its flags write."""
from __future__ import annotations

import json
import os
from collections import namedtuple
from typing import List, Sequence

import numpy as np
import torch

from .energy import ENERGY_GROUP_NAMES, ENERGY_NAMES, EnergyGroup, _group_list, empty_energy, inverse_scale2, rollout_energy
from .regional import (COUNT_NAMES, SUM_NAMES, REGIONAL_KEYS, REGIONAL_SCORE_NAMES, NAMED_REGIONS, Region, empty_regional, mask_words, region_mask as make_region_mask,
                       region_metadata, regional_scores, rollout_regional)
from .score_maps import MAP_COUNT_NAMES, SCORE_MAP_NAMES, TERM_NAMES, ScoreMaps, parse_map_planes, rollout_score_maps, score_maps
from .utils import (MAX_FSS_SCALES, SPECTRUM_NAMES, Event, _radius_list, empty_events, empty_fss, empty_reliability, empty_spectrum, event_scores, fss_scores,
                    rollout_events, rollout_fss, rollout_reliability, rollout_spectrum)

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


# One decode batch as every metric sees it, built once per batch: y (nl, ens, C', H, W), the decoder's output, still normalised; total, the
# columns of every result; kw: lead_dim, mean, std and this batch's truth_slot and l_off as the wrappers take them; clim_kw: clim and clim_slots.
Batch = namedtuple("Batch", "y truth lat_weight sst_channel total kw clim_kw")


def row_latitudes(H: int) -> np.ndarray:
    """the latitudes in degrees of the H rows `lat_weights_for` weighs: the 120-row grid's, else the H rows kept of an equiangular
    pole-to-pole grid of H + 1 (row 0, the south pole, dropped)"""
    return np.linspace(-88.5, 90, 120) if H == 120 else np.linspace(-90.0, 90.0, H + 1)[1:]


def _crop_rows(table: np.ndarray, H: int, what: str) -> np.ndarray:
    """(..., H_in, W) -> the H rows the decoder produces: H_in == H + 1 drops row 0, the south pole (a view: a memmap stays on disk)"""
    H_in = table.shape[-2]
    if H_in == H + 1:
        return table[..., 1:, :]
    if H_in != H:
        raise ValueError(f"{what} has {H_in} rows; the decoded fields have {H} (or {H + 1} with the south pole)")
    return table


def _channel_names(args) -> List[str]:  # the names `--event` and `--energy_group` resolve a CHANNEL against
    from .validate_AR import column_names

    names = column_names(args.variable_names, args.levels, args.num_atm_vars)
    if getattr(args, "derive", None):  # the derived fields are channels C', C' + 1, ... of everything
        from .derived import parse_derived

        names = names + [d.name for d in parse_derived(args.derive, names)]
    return names


class Metric:
    """what the metrics share; `flag`: the command-line flag as the messages name it, `keys`: what one initial time's result gains"""

    flag, keys = "", ()
    out = None  # device half: the result dict, allocated at the first batch

    def start(self, lat_weight: torch.Tensor) -> None:  # once per initial time, when `lat_weight` is on the device, before the first decode
        pass

    def result(self) -> dict:
        return {k: self.out[k].cpu() for k in self.keys}

    @classmethod
    def from_args(cls, args, total: int, files):  # None: not asked for; else ready to gather `total` lead times per initial time
        m = cls.parse(args, files)
        if m is not None:
            m.total, m.acc = total, {}
        return m

    def arrays(self, res, time_str: str, keys, flag=None) -> dict:
        missing = [k for k in keys if k not in res]
        if missing:
            raise ValueError(f"{time_str}: {flag or self.flag} needs {missing} from the scorer")
        return {k: np.asarray(res[k]) for k in keys}

    def keep(self, a: dict, dtypes: dict) -> None:  # kept per initial time
        for k, dt in dtypes.items():
            self.acc.setdefault(k, []).append(a[k].astype(dt))

    def add(self, a: dict, dtypes: dict) -> None:  # summed over the initial times on the host
        for k, dt in dtypes.items():
            self.acc[k] = self.acc.get(k, 0) + a[k].astype(dt)

    def finish(self, out: dict, output: str) -> None:
        out.update({k: np.stack(v) if isinstance(v, list) else v for k, v in self.acc.items()})


class Reliability(Metric):
    """`reliability` / `--reliability`: spread-skill ratio and rank histogram (`rollout_reliability`).  Result: `ens_var`, `ssr` (C, T) fp32,
    `rank_hist` (C, T, ens + 1) int32, `rank_hist_weighted` the same in fp32, `n_invalid` (C, T) int32.  Files: `ens_var.npy`, `ssr.npy`,
    `n_invalid.npy` (init time, C, lead time), and summed over the initial times `rank_hist.npy` int64, `rank_hist_weighted.npy` float64."""

    flag, keys = "--reliability", RELIABILITY_KEYS

    @classmethod
    def for_rollout(cls, o):
        return cls() if o["reliability"] else None

    def run(self, b):
        if self.out is None:
            self.out = empty_reliability(b.y.shape[1], b.y.shape[2], b.total, b.y.device)
        rollout_reliability(b.y, b.truth, b.lat_weight, b.sst_channel, out=self.out, **b.kw)

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--reliability", action="store_true", help="also write ens_var, ssr, rank_hist, rank_hist_weighted and n_invalid")

    @classmethod
    def parse(cls, args, files):
        return cls() if args.reliability else None

    def rollout_kwargs(self, H, W, lat_w, std_t):
        return dict(reliability=True)

    def gather(self, res, time_str):
        T, a = self.total, self.arrays(res, time_str, RELIABILITY_KEYS)
        C = a["ens_var"].shape[0]
        hist_shape = a["rank_hist"].shape
        if any(a[k].shape != (C, T) for k in ("ens_var", "ssr", "n_invalid")) or len(hist_shape) != 3 \
                or hist_shape[:2] != (C, T) or a["rank_hist_weighted"].shape != hist_shape:
            raise ValueError(f"{time_str}: reliability arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {T}) and (C, {T}, members + 1)")
        if "rank_hist" in self.acc and self.acc["rank_hist"].shape != hist_shape:
            raise ValueError(f"{time_str}: a rank histogram of {hist_shape[2] - 1} members after one of {self.acc['rank_hist'].shape[2] - 1}")
        self.keep(a, dict(ens_var=np.float32, ssr=np.float32, n_invalid=np.int32))
        self.add(a, dict(rank_hist=np.int64, rank_hist_weighted=np.float64))


class Spectrum(Metric):
    """`spectrum` / `--spectrum`: zonal power spectra (`rollout_spectrum`).  Result: `spec_members`, `spec_mean`, `spec_truth`
    (C, T, W / 2 + 1) fp32, `spec_n_invalid` (C, T) int32.  `spectrum_row_weight` (H,), non-negative, weights the rows (0: the row is left
    out and never read); default: `lat_weight`.  `--spectrum_lat_band LO HI` (degrees) gives the rows outside the band weight 0, the rows
    inside keep the cos weight.  Files: `<key>.npy` (init time, C, lead time[, W / 2 + 1])."""

    flag, keys = "--spectrum", SPECTRUM_KEYS

    def __init__(self, row_weight=None, band=None):
        self.row_weight, self.band = row_weight, band

    @classmethod
    def for_rollout(cls, o):
        return cls(o["spectrum_row_weight"]) if o["spectrum"] else None

    def start(self, lat_weight):
        w = lat_weight if self.row_weight is None else self.row_weight
        if not w.is_cuda and not bool((w >= 0).all()):
            raise ValueError("spectrum_row_weight must be non-negative (0 leaves a row out) and not NaN")
        self.w = w.to(lat_weight.device, torch.float32)

    def run(self, b):
        if self.out is None:
            self.out = empty_spectrum(b.y.shape[2], b.total, b.y.shape[4], b.y.device)
        rollout_spectrum(b.y, b.truth, self.w, out=self.out, **b.kw)

    def result(self):
        return dict({k: self.out[k].cpu() for k in SPECTRUM_NAMES}, spec_n_invalid=self.out["n_invalid"].cpu())

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--spectrum", action="store_true", help="also write spec_members, spec_mean, spec_truth and spec_n_invalid")
        ap.add_argument("--spectrum_lat_band", type=float, nargs=2, default=None, metavar=("LO", "HI"),
                        help="latitudes in degrees between which rows enter the spectra (default: all rows)")

    @classmethod
    def parse(cls, args, files):
        return cls(band=args.spectrum_lat_band) if args.spectrum else None

    def rollout_kwargs(self, H, W, lat_w, std_t):
        return dict(spectrum=True, spectrum_row_weight=spectrum_band_weights(lat_w, row_latitudes(H), self.band))

    def gather(self, res, time_str):
        T, a = self.total, self.arrays(res, time_str, SPECTRUM_KEYS)
        shape = a[SPECTRUM_NAMES[0]].shape
        if len(shape) != 3 or shape[1] != T or any(a[k].shape != shape for k in SPECTRUM_NAMES) or a["spec_n_invalid"].shape != shape[:2]:
            raise ValueError(f"{time_str}: spectrum arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {T}, K) and (C, {T})")
        self.keep(a, dict({k: np.float32 for k in SPECTRUM_NAMES}, spec_n_invalid=np.int32))


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


class Events(Metric):
    """`events` / `--event`, `--event_anomaly`: threshold events (`rollout_events`), and with `fss_radii` / `--fss_scales` their neighbourhood
    verification (`rollout_fss`), which follows in the same batch: it verifies the same `Event` list, its shapes carry their number and
    `events.json` is one file, so the two are one object.  `events`: a sequence of `Event(channel, "gt" | "lt", threshold, anomaly)`; an
    anomaly event with `clim` None is a ValueError.  Result: `event_hist` (E, T, ens + 1, 2) int32, `event_hist_weighted` the same in
    fp32, `event_n_invalid` (E, T) int32.  `fss_radii`: radii in grid points, a ValueError without `events`.  Result: `event_fss_sums`
    (E, S, T, 6) float64, `event_fss_n_invalid` (E, T) int32 (columns past the last lead time are zeros).
    `--event CHANNEL gt|lt VALUE`, `--event_anomaly CHANNEL gt|lt VALUE` (each any number of times; CHANNEL a name of
    `products.column_names` or an index; plain events first).  Files: `event_hist.npy` int64, `event_hist_weighted.npy` float64, summed
    over the initial times, `event_n_invalid.npy` (init time, E, lead time), `events.json` (the events as given, with resolved channel
    names), `event_<score>.npy` (E, lead time) float64 for `EVENT_FILE_SCORES`: `event_scores` of the pooled weighted histogram.
    `--fss_scales R [R ...]` (needs an event flag): `event_fss_sums.npy` summed over the initial times, `event_fss_n_invalid.npy` (init
    time, E, lead time), the files of `FSS_FILE_SCORES` (E, scale, lead time), `event_fss_useful_scale.npy` (E, lead time) int64:
    `fss_scores` of the pooled sums; `events.json` gains `fss_radii` and `fss_width_deg` (the window's width
    (2 R + 1) 360 / W in degrees; in kilometres it shrinks towards the poles)."""

    flag, keys = "--event", EVENTS_KEYS
    fss = grid_w = None  # device half: the result dict of `rollout_fss`; host half: points per row, where the data tell it

    def __init__(self, events, radii=None, has_clim: bool = True, meta=None):
        self.events, self.meta = [Event(*ev) for ev in events], meta
        if not has_clim and any(ev.anomaly for ev in self.events):
            raise ValueError("an anomaly event needs the climatology (clim)")
        self.radii = None if radii is None else list(radii)

    @classmethod
    def for_rollout(cls, o):
        if o["fss_radii"] is not None and not o["events"]:
            raise ValueError("fss_radii needs events: the neighbourhood scores verify threshold events")
        return cls(o["events"], o["fss_radii"], o["clim"] is not None) if o["events"] else None

    def run(self, b):
        if self.out is None:
            self.out = empty_events(b.y.shape[1], len(self.events), b.total, b.y.device)
        rollout_events(b.y, b.truth, b.lat_weight, self.events, out=self.out, **b.clim_kw, **b.kw)
        if self.radii is not None:
            if self.fss is None:
                self.fss = empty_fss(len(self.events), len(_radius_list(self.radii, b.y.shape[4])), b.total, b.y.device)
            rollout_fss(b.y, b.truth, b.lat_weight, self.events, self.radii, out=self.fss, **b.clim_kw, **b.kw)

    def result(self):
        return dict(super().result(), **({} if self.fss is None else {k: self.fss[k].cpu() for k in FSS_KEYS}))

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--event", nargs=3, action="append", default=[], metavar=("CHANNEL", "gt|lt", "VALUE"),
                        help="verify the event 'CHANNEL above (gt) / below (lt) VALUE' (physical units); may be given several times")
        ap.add_argument("--event_anomaly", nargs=3, action="append", default=[], metavar=("CHANNEL", "gt|lt", "VALUE"),
                        help="the same on CHANNEL minus its climatology")
        ap.add_argument("--fss_scales", nargs="+", default=None, metavar="R",
                        help="also verify the events in neighbourhoods of (2 R + 1) x (2 R + 1) grid points (fractions skill score); needs --event / --event_anomaly")

    @classmethod
    def parse(cls, args, files):
        events, meta = parse_events(args.event, args.event_anomaly, _channel_names(args)) if args.event or args.event_anomaly else ([], [])
        if args.fss_scales is not None and not events:
            raise ValueError("--fss_scales needs --event or --event_anomaly")
        return cls(events, None if args.fss_scales is None else parse_fss_scales(args.fss_scales), meta=meta) if events else None

    def rollout_kwargs(self, H, W, lat_w, std_t):
        self.grid_w = W
        return dict(events=self.events, fss_radii=self.radii)

    def gather(self, res, time_str):
        T, E = self.total, len(self.events)
        a = self.arrays(res, time_str, EVENTS_KEYS)
        shape = a["event_hist"].shape
        if len(shape) != 4 or shape[:2] != (E, T) or shape[3] != 2 or a["event_hist_weighted"].shape != shape \
                or a["event_n_invalid"].shape != (E, T):
            raise ValueError(f"{time_str}: event arrays of shapes { {k: v.shape for k, v in a.items()} }, expected ({E}, {T}, members + 1, 2) and ({E}, {T})")
        if "event_hist" in self.acc and self.acc["event_hist"].shape != shape:
            raise ValueError(f"{time_str}: an event histogram of {shape[2] - 1} members after one of {self.acc['event_hist'].shape[2] - 1}")
        self.keep(a, dict(event_n_invalid=np.int32))
        self.add(a, dict(event_hist=np.int64, event_hist_weighted=np.float64))
        if self.radii is not None:
            a, S = self.arrays(res, time_str, FSS_KEYS, "--fss_scales"), len(self.radii)
            s, n = a["event_fss_sums"], a["event_fss_n_invalid"]
            if s.shape != (E, S, T, 6) or n.shape != (E, T):
                raise ValueError(f"{time_str}: fss arrays of shapes {s.shape} and {n.shape}, expected ({E}, {S}, {T}, 6) and ({E}, {T})")
            self.add(a, dict(event_fss_sums=np.float64))
            self.keep(a, dict(event_fss_n_invalid=np.int32))

    def finish(self, out, output):
        super().finish(out, output)
        sc = event_scores(self.acc["event_hist_weighted"])
        out.update({f"event_{k}": np.asarray(sc[k], dtype=np.float64) for k in EVENT_FILE_SCORES})
        meta = dict(events=self.meta)
        if self.radii is not None:
            sc = fss_scores(self.acc["event_fss_sums"], self.radii)
            out.update({name: np.asarray(sc[k], dtype=np.float64) for name, k in FSS_FILE_SCORES.items()},
                       event_fss_useful_scale=np.asarray(sc["useful_scale"], dtype=np.int64))
            meta.update(fss_radii=self.radii, fss_width_deg=None if self.grid_w is None else [(2 * r + 1) * 360.0 / self.grid_w for r in self.radii])
        with open(os.path.join(output, "events.json"), "w") as f:
            json.dump(meta, f, indent=1)


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


class Regional(Metric):
    """`regions` / `--region`, `--region_box`: the scores by region, every region in one `rollout_regional` launch per batch.  `regions`: a
    sequence of `Region` (or an int: their number) with `region_mask`, the (H, W) uint32 mask of which bit r marks region r (default:
    built from `regions` on `row_latitudes(H)` and the longitudes 0, 360 / W, ...).  Result: `regional_sums` (R, C, T, 10) float64,
    `regional_counts` (R, C, T, 3) int32 (columns past the last lead time are zeros).
    `--region NAME` (from `NAMED_REGIONS`), `--region_box NAME LAT0 LAT1 LON0 LON1` (each any number of times; named regions first),
    `--region_surface NAME land|sea` with `--land_sea_mask_path` (.npy (H_in, W), land where >= 0.5; rows cropped as the truth's).
    Files: `regional_sums.npy`, `regional_counts.npy` pooled over the initial times on the host (float64, int64), `regional_<score>.npy`
    (R, C, lead time) for `REGIONAL_SCORE_NAMES` (`regional_scores` of the pooled sums), `regions.json` (`region_metadata`);
    `--region_per_init` also `regional_sums_per_init.npy` (init time, R, C, lead time, 10): a year of 84 channels x 13 regions is gigabytes."""

    flag, keys = "--region", REGIONAL_KEYS
    meta = None  # regions.json's entries, where the mask is built here

    def __init__(self, regions, mask=None):
        self.regions, self.mask = regions, mask
        if regions is None:
            raise ValueError("region_mask needs regions (the Region list, or their number)")
        number = isinstance(regions, (int, np.integer))
        self.n = int(regions) if number else len(regions)
        if not 1 <= self.n <= 32:
            raise ValueError(f"{self.n} regions: ldc_rollout_regional takes 1 .. 32 per call")
        if mask is None and number:
            raise ValueError("a number of regions needs the region_mask")

    @classmethod
    def for_rollout(cls, o):
        return cls(o["regions"], o["region_mask"]) if o["regions"] is not None or o["region_mask"] is not None else None

    def run(self, b):
        if self.out is None:
            H, W = b.y.shape[3:]
            mask = self.mask if self.mask is not None else make_region_mask(self.regions, row_latitudes(H), np.arange(W) * (360.0 / W))
            self.words = mask if isinstance(mask, torch.Tensor) and mask.is_cuda else mask_words(mask, H, W).to(b.y.device)
            self.out = empty_regional(self.n, b.y.shape[2], b.total, b.y.device)
        rollout_regional(b.y, b.truth, b.lat_weight, self.words, self.n, out=self.out, **b.clim_kw, **b.kw)

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--region", action="append", default=[], metavar="NAME", help="break the scores down by this named region; may be given several times")
        ap.add_argument("--region_box", nargs=5, action="append", default=[], metavar=("NAME", "LAT0", "LAT1", "LON0", "LON1"),
                        help="a region of your own: latitudes LAT0 .. LAT1 (inclusive), longitudes LON0 .. LON1 east (LON0 > LON1: across 0 degrees)")
        ap.add_argument("--region_surface", nargs=2, action="append", default=[], metavar=("NAME", "land|sea"),
                        help="restrict the region NAME to land or sea points (needs --land_sea_mask_path)")
        ap.add_argument("--land_sea_mask_path", type=str, default=None, help=".npy (H_in, W): land where >= 0.5")
        ap.add_argument("--region_per_init", action="store_true", help="also write regional_sums_per_init.npy (init time, R, C, lead time, 10)")

    @classmethod
    def parse(cls, args, files):
        regions = parse_regions(args.region, args.region_box, args.region_surface)
        if any(r.surface for r in regions) and args.land_sea_mask_path is None:
            raise ValueError("--region_surface needs --land_sea_mask_path")
        if not regions:
            if args.region_per_init or args.land_sea_mask_path or args.region_surface:
                raise ValueError("--region_per_init, --region_surface and --land_sea_mask_path need --region or --region_box")
            return None
        m = cls(regions)
        m.lsm_path, m.per_init = args.land_sea_mask_path, [] if args.region_per_init else None
        m.members = int(np.load(files[0][1], mmap_mode="r").shape[0])  # the members the sums are taken over: the ssr's (M + 1) / M
        m.members = m.members if args.force_ens_size is None else min(m.members, args.force_ens_size)
        return m

    def rollout_kwargs(self, H, W, lat_w, std_t):
        lsm = None
        if self.lsm_path is not None:
            lsm = np.load(self.lsm_path)
            if lsm.ndim != 2:
                raise ValueError(f"--land_sea_mask_path must be (H_in, W), got {lsm.shape}")
            lsm = _crop_rows(lsm, H, "--land_sea_mask_path")
        mask = make_region_mask(self.regions, row_latitudes(H), np.arange(W) * (360.0 / W), lsm)
        self.meta = region_metadata(self.regions, mask, lat_w.numpy())
        return dict(regions=self.regions, region_mask=mask)

    def gather(self, res, time_str):
        T, R = self.total, self.n
        a = self.arrays(res, time_str, REGIONAL_KEYS)
        s, n = a["regional_sums"], a["regional_counts"]
        if s.ndim != 4 or s.shape[0] != R or s.shape[2:] != (T, 10) or n.shape != s.shape[:3] + (3,):
            raise ValueError(f"{time_str}: regional arrays of shapes {s.shape} and {n.shape}, expected ({R}, C, {T}, 10) and ({R}, C, {T}, 3)")
        if "regional_sums" in self.acc and self.acc["regional_sums"].shape != s.shape:
            raise ValueError(f"{time_str}: regional sums of shape {s.shape} after {self.acc['regional_sums'].shape}")
        self.add(a, dict(regional_sums=np.float64, regional_counts=np.int64))
        if self.per_init is not None:
            self.per_init.append(s.astype(np.float64))

    def finish(self, out, output):
        super().finish(out, output)
        sc = regional_scores(self.acc["regional_sums"], self.acc["regional_counts"], self.members)
        out.update({f"regional_{k}": np.asarray(sc[k]) for k in REGIONAL_SCORE_NAMES})
        if self.per_init is not None:
            out["regional_sums_per_init"] = np.stack(self.per_init)
        meta = self.meta
        if meta is None:  # an injected scorer: the mask of the pooled arrays' grid is not known here
            meta = [dict(name=r.name, boxes=[[r.lat_min, r.lat_max, r.lon_min, r.lon_max]] + [list(b) for b in r.boxes], surface=r.surface,
                         n_points=None, weight=None) for r in self.regions]
        with open(os.path.join(output, "regions.json"), "w") as f:
            json.dump(dict(regions=meta, members=self.members, sums=list(SUM_NAMES), counts=list(COUNT_NAMES)), f, indent=1)


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


class Energy(Metric):
    """`energy` / `--energy`: the energy score (`rollout_energy`; up to 256 members).  Result: `energy_score`, `energy_score_fair`,
    `energy_skill`, `energy_spread`, `energy_weight` (C, T) float64, `energy_n_invalid` (C, T) int32 (columns past the last lead time are
    NaN).  `energy_groups` / `--energy_group NAME CHANNEL [CHANNEL ...]` (any number of times, CHANNEL resolved as `--event` resolves it;
    implies `energy`): a sequence of `EnergyGroup(name, channels)`; the result gains `ENERGY_GROUP_NAMES`, (G, T) float64.  `energy_scales`
    (C',), positive and finite, divides each channel of a group; default: `std_tensor`.  Files: `energy_score.npy`, `energy_score_fair.npy`,
    `energy_skill.npy`, `energy_spread.npy` (init time, C, lead time) float64, `energy_n_invalid.npy` int32, `energy_group_score.npy`, ...
    (init time, G, lead time), `energy.json` (group names, channels, scales).  Not additive over initial times: pool by the mean over them."""

    flag = "--energy"
    names = scales_meta = None  # the channel names and scales of energy.json, where the command line knows them

    def __init__(self, groups, scales=None, default_scales=None):
        self.groups, self.scales, self.default_scales = groups, scales, default_scales
        if scales is not None and not groups:
            raise ValueError("energy_scales needs energy_groups: the scales divide the channels of a group")
        if groups:  # malformed groups and scales raise before anything is decoded; the channel range is checked at the first batch
            _group_list(groups, 1 << 31)
            if scales is not None:
                inverse_scale2(scales, torch.as_tensor(scales).numel())

    @classmethod
    def for_rollout(cls, o):
        m = cls(o["energy_groups"], o["energy_scales"], o["std_tensor"])
        return m if o["energy"] or o["energy_groups"] else None

    def run(self, b):
        if self.out is None:
            self.groups = _group_list(self.groups, b.y.shape[2])  # resolved against the decoded channel count
            if self.groups and self.scales is None:
                self.scales = self.default_scales
            self.keys = ENERGY_KEYS + (ENERGY_GROUP_NAMES if self.groups else ())
            self.out = empty_energy(b.y.shape[1], b.y.shape[2], len(self.groups), b.total, b.y.device)
        rollout_energy(b.y, b.truth, b.lat_weight, groups=self.groups, scales=self.scales if self.groups else None, out=self.out, **b.kw)

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--energy", action="store_true", help="also write the energy score per channel: energy_score, energy_score_fair, energy_skill, energy_spread, energy_n_invalid")
        ap.add_argument("--energy_group", nargs="+", action="append", default=[], metavar="NAME_THEN_CHANNELS",
                        help="NAME CHANNEL [CHANNEL ...]: also score these channels together, each divided by its normalisation std; may be given several times; implies --energy")

    @classmethod
    def parse(cls, args, files):
        if not (args.energy or args.energy_group):
            return None
        names = _channel_names(args) if args.energy_group else None
        m = cls(parse_energy_groups(args.energy_group, names) if args.energy_group else [])
        m.names = names
        return m

    def rollout_kwargs(self, H, W, lat_w, std_t):
        if self.groups:
            self.scales_meta = [float(v) for v in torch.as_tensor(std_t).reshape(-1).tolist()]
        return dict(energy=True, energy_groups=self.groups or None)

    def gather(self, res, time_str):
        T, G = self.total, len(self.groups)
        a = self.arrays(res, time_str, ENERGY_FILE_KEYS + (ENERGY_GROUP_FILE_KEYS if G else ()))
        C = a["energy_score"].shape[0]
        if any(a[k].shape != (C, T) for k in ENERGY_FILE_KEYS) or any(a[k].shape != (G, T) for k in list(a)[len(ENERGY_FILE_KEYS):]):
            raise ValueError(f"{time_str}: energy arrays of shapes { {k: v.shape for k, v in a.items()} }, expected (C, {T}) and ({G}, {T})")
        self.keep(a, {k: np.int32 if k == "energy_n_invalid" else np.float64 for k in a})

    def finish(self, out, output):
        super().finish(out, output)
        with open(os.path.join(output, "energy.json"), "w") as f:
            json.dump(dict(groups=[dict(name=g.name, channels=list(g.channels),
                                        channel_names=None if self.names is None else [self.names[c] for c in g.channels],
                                        scales=None if self.scales_meta is None else [self.scales_meta[c] for c in g.channels]) for g in self.groups]),
                      f, indent=1)


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


class Maps(Metric):
    """`score_maps` / `--map`: per-point score maps accumulated on the device over the initial times (`rollout_score_maps`).  `score_maps`:
    a `ScoreMaps` accumulator, which the caller keeps over any number of `score_latent_rollout` calls and downloads once; every decode
    batch is added to it after the other metrics have run, and `n_init` counts the calls.  The result of an initial time gains NO key.
    `--map CHANNEL [CHANNEL ...]` (names as `--event` resolves them, or indices; `all`: every channel), `--map_lead_hours H ...` (one
    plane per listed lead hour; default: every lead time) or `--map_lead_bins A-B ...` (one plane per inclusive range of lead hours,
    pooled), `--map_max_gib` (default 16; a guard, not a measurement: the run prints the bytes of the accumulators and refuses above it
    before anything is decoded).  Files, written once from one download: `score_map_sums.npy` (Cm, P, 8, H, W) float64,
    `score_map_counts.npy` (Cm, P, 3, H, W) int32, `score_map_<score>.npy` (Cm, P, H, W) for `SCORE_MAP_NAMES` (`score_maps`),
    `score_maps.json` (channel names, planes with their lead hours, members, n_init, term names)."""

    flag = "--map"
    names = planes = None  # score_maps.json's channel names and planes, where the command line knows them

    def __init__(self, acc):
        if not isinstance(acc, ScoreMaps):
            raise ValueError("score_maps must be a ScoreMaps accumulator")
        self.maps = acc

    @classmethod
    def for_rollout(cls, o):
        acc = o.get("score_maps")  # option dicts built before this metric existed do not hold the key
        return cls(acc) if acc is not None else None

    def run(self, b):
        rollout_score_maps(b.y, b.truth, self.maps, **b.clim_kw, **b.kw)

    def result(self):
        self.maps.n_init += 1
        return {}

    @staticmethod
    def add_arguments(ap):
        ap.add_argument("--map", nargs="+", default=None, metavar="CHANNEL", help="accumulate per-point score maps of these channels (names or indices; all: every channel)")
        ap.add_argument("--map_lead_hours", nargs="+", default=None, metavar="H", help="one map plane per listed lead hour (default: every lead time)")
        ap.add_argument("--map_lead_bins", nargs="+", default=None, metavar="A-B", help="one map plane per inclusive range of lead hours, pooled; excludes --map_lead_hours")
        ap.add_argument("--map_max_gib", type=float, default=16.0, help="refuse map accumulators larger than this many GiB of device memory")

    @classmethod
    def parse(cls, args, files):
        if args.map is None:
            if args.map_lead_hours is not None or args.map_lead_bins is not None:
                raise ValueError("--map_lead_hours and --map_lead_bins need --map")
            return None
        from .products import resolve_channels

        names = _channel_names(args)
        chans = list(range(len(names))) if list(args.map) == ["all"] else resolve_channels(args.map, names)
        if len(set(chans)) != len(chans):
            raise ValueError(f"--map {' '.join(args.map)}: a channel is named twice")
        total = args.total_lead_time_hour // args.step_size_hour
        plane_of_lead, planes = parse_map_planes(total, args.step_size_hour, args.map_lead_hours, args.map_lead_bins)
        if not args.map_max_gib > 0:
            raise ValueError("--map_max_gib must be positive")
        m = cls(ScoreMaps(chans, plane_of_lead, len(planes)))
        m.names, m.planes, m.max_gib = [names[c] for c in chans], planes, float(args.map_max_gib)
        return m

    def rollout_kwargs(self, H, W, lat_w, std_t):
        nbytes = self.maps.nbytes(H, W)
        print(f"score maps: {len(self.maps.channels)} channels x {self.maps.n_planes} planes x {H} x {W} points: {nbytes} bytes on the device")
        if nbytes <= 0 or nbytes > self.max_gib * 2 ** 30:
            raise ValueError(f"--map: the accumulators take {nbytes} bytes ({nbytes / 2 ** 30:.2f} GiB; 0: sizes the kernel refuses), --map_max_gib is {self.max_gib}")
        return dict(score_maps=self.maps)

    def gather(self, res, time_str):
        pass

    def finish(self, out, output):
        if self.maps.sums is None:
            raise ValueError("--map: nothing was accumulated (the maps live on the device: an injected scorer must add to the ScoreMaps itself)")
        sums, counts = self.maps.download()
        sc = score_maps(sums, counts, self.maps.members)
        out.update(score_map_sums=sums, score_map_counts=counts, **{f"score_map_{k}": np.asarray(sc[k]) for k in SCORE_MAP_NAMES})
        with open(os.path.join(output, "score_maps.json"), "w") as f:
            json.dump(dict(channels=self.names, channel_indices=self.maps.channels, planes=self.planes, plane_of_lead=self.maps.plane_of_lead,
                           members=self.maps.members, n_init=self.maps.n_init, terms=list(TERM_NAMES), counts=list(MAP_COUNT_NAMES)), f, indent=1)


METRICS = (Reliability, Spectrum, Events, Regional, Energy, Maps)  # launch and key order; `Events` holds the fss, which follows the events
