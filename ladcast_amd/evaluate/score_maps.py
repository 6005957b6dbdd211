"""Per-point score maps accumulated on the device over initial times (`ldc_rollout_score_maps`, csrc/score_maps.hip, DESIGN.md section
8.11; not in the reference): where the ensemble is biased, where it is under-dispersive, where the anomaly correlation is lost.

    acc = ScoreMaps(channels=[0, 7], plane_of_lead=[0, 0, 1, 1, -1, 2], n_planes=3)    # leads 0-1 and 2-3 pooled, lead 4 skipped
    for forecast, truth, clim in initial_times:                                        # or score_latent_rollout(..., score_maps=acc)
        rollout_score_maps(forecast, truth, acc, clim=clim)
    sums, counts = acc.download()                                                      # (Cm, P, 8, H, W) float64, (Cm, P, 3, H, W) int32
    maps = score_maps(sums, counts, acc.members)                                       # bias, rmse, ssr, crps, ens_acc, ... (Cm, P, H, W)

A map is as large as the field, so it is never copied to the host per initial time: the two buffers live on the device, every call adds
to them in place, one thread per (channel, plane, point) and no atomics, and `download` reads them back once.  The maps are unweighted;
weights enter when maps are pooled on the host: `regional_from_maps` gives the sums of any region after the fact."""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from .regional import N_COUNTS, N_SUMS
from .utils import _launch_args, _prologue, _upload_slots

N_TERMS, N_MAP_COUNTS, MAX_MAP_MEMBERS = hip.SCORE_MAPS_TERMS, hip.SCORE_MAPS_COUNTS, hip.SCORE_MAPS_MAX_MEMBERS
MAX_MAP_CHANNELS = MAX_MAP_PLANES = 65535
# the 8 sums of one (channel, plane, point): over its valid samples, then over its ACC-valid samples
TERM_NAMES = ("e", "se", "var", "skill", "spread", "fa_ta", "fa_fa", "ta_ta")
MAP_COUNT_NAMES = ("n_valid", "n_invalid", "n_acc_valid")
SCORE_MAP_NAMES = ("bias", "ens_mse", "rmse", "ens_var", "ssr", "crps_skill", "crps_spread", "crps", "ens_acc", "n_valid")


def _int_list(values, what: str):
    vals = list(values.tolist() if isinstance(values, (torch.Tensor, np.ndarray)) else values)
    if any(isinstance(v, bool) or int(v) != v for v in vals):
        raise ValueError(f"{what} must be whole numbers, got {vals}")
    return [int(v) for v in vals]


class ScoreMaps:
    """The accumulator of the score maps: `channels` (indices into the forecast's channels, any order), `plane_of_lead` (for every lead
    time of a rollout the plane 0 .. `n_planes` - 1 it adds to, or -1: skipped; several lead times may share a plane) and the two zeroed
    device buffers, allocated at the first batch, when grid, ensemble size and device are known.  `members`: the ensemble size of the
    batches so far (one accumulator serves one); `n_init`: the initial times `score_latent_rollout` has added."""

    def __init__(self, channels: Sequence[int], plane_of_lead: Sequence[int], n_planes: int):
        self.channels, self.plane_of_lead, self.n_planes = _int_list(channels, "channels"), _int_list(plane_of_lead, "plane_of_lead"), int(n_planes)
        if not 1 <= len(self.channels) <= MAX_MAP_CHANNELS or any(c < 0 for c in self.channels):
            raise ValueError(f"channels must be 1 .. {MAX_MAP_CHANNELS} non-negative indices, got {self.channels}")
        if not 1 <= self.n_planes <= MAX_MAP_PLANES:
            raise ValueError(f"{self.n_planes} planes: ldc_rollout_score_maps takes 1 .. {MAX_MAP_PLANES}")
        if not self.plane_of_lead or any(not -1 <= p < self.n_planes for p in self.plane_of_lead):
            raise ValueError(f"plane_of_lead must name a plane 0 .. {self.n_planes - 1} or -1 for every lead time, got {self.plane_of_lead}")
        self.sums = self.counts = self.members = self.grid = None
        self.n_init = 0
        self._chan_d, self._plane_d = None, {}

    def nbytes(self, H: int, W: int) -> int:
        """bytes of the two device buffers together on an (H, W) grid (`ldc_score_maps_bytes`; 0 for sizes the kernel refuses)"""
        return hip.score_maps_bytes(len(self.channels), self.n_planes, int(H), int(W))

    def _prepare(self, r, l_off: int):
        """checks of one batch against the accumulator, no device touched: -> the slice of `plane_of_lead` of this batch"""
        if l_off < 0 or l_off + r.L > len(self.plane_of_lead):
            raise ValueError(f"lead times {l_off} .. {l_off + r.L - 1} reach outside the {len(self.plane_of_lead)} entries of plane_of_lead")
        if max(self.channels) >= r.C:
            raise ValueError(f"channels {self.channels} reach outside the forecast's {r.C} channels")
        if r.H * r.W > 1 << 24:
            raise ValueError(f"{r.H} x {r.W} points: ldc_rollout_score_maps serves at most 2^24")
        if self.sums is not None and (self.grid != (r.H, r.W) or self.members != r.M or self.sums.device != r.f.device):
            raise ValueError(f"this accumulator holds {self.members} members on a {self.grid} grid on {self.sums.device}; "
                             f"got {r.M} on {(r.H, r.W)} on {r.f.device}")
        return self.plane_of_lead[l_off : l_off + r.L]

    def _buffers(self, r):
        if self.sums is None:
            Cm, P, dev = len(self.channels), self.n_planes, r.f.device
            self.sums = torch.zeros(Cm, P, N_TERMS, r.H, r.W, device=dev, dtype=torch.float64)
            self.counts = torch.zeros(Cm, P, N_MAP_COUNTS, r.H, r.W, device=dev, dtype=torch.int32)
            self.grid, self.members = (r.H, r.W), r.M
            self._chan_d = _upload_slots(self.channels, dev)
        return self.sums, self.counts

    def _planes(self, l_off: int, planes, dev) -> torch.Tensor:
        key = (l_off, len(planes))
        if key not in self._plane_d:  # one upload per batch position, not per initial time
            self._plane_d[key] = _upload_slots(planes, dev)
        return self._plane_d[key]

    def download(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (sums (Cm, P, 8, H, W) float64, counts (Cm, P, 3, H, W) int32), the one copy to the host"""
        if self.sums is None:
            raise RuntimeError("nothing was accumulated: no batch has gone through rollout_score_maps")
        return self.sums.cpu().numpy(), self.counts.cpu().numpy()


@torch.no_grad()
def rollout_score_maps(forecast: torch.Tensor, truth: torch.Tensor, maps: ScoreMaps, *, clim: Optional[torch.Tensor] = None, clim_slots=None,
                       lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0,
                       truth_slot=None, l_off: int = 0) -> ScoreMaps:
    """Adds the L lead times of a decode batch to `maps` in one launch (`ldc_rollout_score_maps`): lead l goes to plane
    `maps.plane_of_lead[l_off + l]` (-1: skipped).  Per point of a mapped channel, all fp32 and the bits `rollout_regional` forms: e,
    se, var, skill, spread, fa * ta, fa * fa, ta * ta; a valid point (no NaN among members and truth) adds the first five to the fp64
    sums and is counted, an ACC-valid point (the climatology is not NaN either) also the last three; an invalid point is counted only.
    The lead times of a call that share a plane are added in ascending order; the bits of a plane depend on the sequence of
    contributions alone, not on how the lead times are batched into calls.  Without `clim` the ACC terms are not touched.  1 <= M <= 64.

    forecast, `lead_dim`, `mean` / `std` / `target_std`, truth / `truth_slot`, `clim` / `clim_slots`: as `rollout_regional`.  Returns `maps`."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), clim=(clim, clim_slots),
                  members=("ldc_rollout_score_maps", MAX_MAP_MEMBERS))
    planes = maps._prepare(r, int(l_off))
    hip._dev(forecast, truth, clim, mean, std)
    sums, counts = maps._buffers(r)
    args, kw = _launch_args(r, r.L, 0)
    del kw["L_total"], kw["l_off"]
    hip.rollout_score_maps(*args[:-1], maps._chan_d, maps._planes(int(l_off), planes, r.f.device), sums, counts, Cm=len(maps.channels),
                           P=maps.n_planes, **kw)
    return maps


def _split(sums, counts):
    s, n = np.asarray(sums, dtype=np.float64), np.asarray(counts)
    if s.ndim < 3 or n.ndim != s.ndim or s.shape[-3] != N_TERMS or n.shape[-3] != N_MAP_COUNTS or s.shape[:-3] != n.shape[:-3] \
            or s.shape[-2:] != n.shape[-2:]:
        raise ValueError(f"sums must be (..., {N_TERMS}, H, W) and counts (..., {N_MAP_COUNTS}, H, W) over the same grid, got {s.shape} and {n.shape}")
    return s, n


def score_maps(sums, counts, M: int) -> Dict[str, np.ndarray]:
    """The score of every (channel, plane, point) from the accumulated sums, on the host in float64 (numpy; no device): `regional_scores`
    with the valid count N in place of sum w.  sums (..., 8, H, W) = S0 .. S7 (`TERM_NAMES`), counts (..., 3, H, W):
        bias = S0 / N               ens_mse = S1 / N            rmse = sqrt(ens_mse)        ens_var = S2 / N
        ssr = sqrt((M + 1) / M) * sqrt(ens_var / ens_mse)       (NaN at M == 1)
        crps_skill = S3 / N         crps_spread = S4 / N        crps = crps_skill - crps_spread / 2
        ens_acc = S5 / sqrt(S6 * S7)   over the ACC-valid samples: the temporal anomaly correlation of the point (NaN without one)
        n_valid = N
    each of shape (..., H, W); NaN where a point has no valid sample."""
    s, n = _split(sums, counts)
    M = int(M)
    if M < 1:
        raise ValueError("at least one member")
    n_valid, n_acc = n[..., 0, :, :].astype(np.int64), n[..., 2, :, :].astype(np.int64)
    t = lambda k: s[..., k, :, :]  # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        s0 = np.where(n_valid > 0, n_valid.astype(np.float64), np.nan)
        bias, mse, var, skill, spread = (t(k) / s0 for k in range(5))
        ssr = np.sqrt((M + 1.0) / M) * np.sqrt(var / mse) if M > 1 else np.full(mse.shape, np.nan)
        acc = np.where(n_acc > 0, t(5) / np.sqrt(t(6) * t(7)), np.nan)
    return dict(bias=bias, ens_mse=mse, rmse=np.sqrt(mse), ens_var=var, ssr=ssr, crps_skill=skill, crps_spread=spread, crps=skill - spread / 2,
                ens_acc=acc, n_valid=n_valid)


def regional_from_maps(sums, counts, lat_weight, region_mask, R: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pools maps over regions: -> (sums (R, ..., 10) float64, counts (R, ..., 3) int64) in the format of `rollout_regional` (`regional.SUM_NAMES`,
    `COUNT_NAMES`), so that `regional_scores` gives the scores of any region after the fact, without another pass over the rollouts.
    sums (..., 8, H, W), counts (..., 3, H, W); `lat_weight` (H,), taken as the fp32 values the kernels read; `region_mask` (H, W) words of
    which bit r < R marks region r.  With w the weight of a point's row, over the points of region r:
        S0 = sum w n_valid, S1 .. S5 = sum w (terms 0 .. 4), S6 = sum w n_acc_valid, S7 .. S9 = sum w (terms 5 .. 7); counts summed."""
    s, n = _split(sums, counts)
    H, W = s.shape[-2:]
    R = int(R)
    if not 1 <= R <= 32:
        raise ValueError(f"{R} regions: a mask word holds 1 .. 32")
    m = np.asarray(region_mask.cpu() if isinstance(region_mask, torch.Tensor) else region_mask)
    if m.shape != (H, W) or m.dtype.kind not in "iu":
        raise ValueError(f"region_mask must hold integer words (H, W) = {(H, W)}, got {m.dtype} {m.shape}")
    w = np.asarray(lat_weight.cpu() if isinstance(lat_weight, torch.Tensor) else lat_weight, dtype=np.float32).reshape(-1)
    if w.size != H:
        raise ValueError("lat_weight must have one value per latitude row")
    words = m.astype(np.int64).reshape(-1)
    wp = np.repeat(w.astype(np.float64), W)
    lead = s.shape[:-3]
    sf, nf = s.reshape(-1, N_TERMS, H * W), n.reshape(-1, N_MAP_COUNTS, H * W).astype(np.int64)
    out_s, out_n = np.zeros((R, sf.shape[0], N_SUMS)), np.zeros((R, sf.shape[0], N_COUNTS), dtype=np.int64)
    for r in range(R):  # a point outside the region is not added at all: an inf or NaN there has no effect
        sel = ((words >> r) & 1) == 1
        terms = np.concatenate([nf[:, 0:1, sel], sf[:, 0:5, sel], nf[:, 2:3, sel], sf[:, 5:8, sel]], axis=1)  # (B, 10, points of r)
        with np.errstate(invalid="ignore", over="ignore"):
            out_s[r] = (terms * wp[sel]).sum(-1)
        out_n[r] = nf[:, :, sel].sum(-1)
    return out_s.reshape(R, *lead, N_SUMS), out_n.reshape(R, *lead, N_COUNTS)


def parse_map_planes(total_num_steps: int, step_size_hour: int, lead_hours=None, lead_bins=None):
    """`--map_lead_hours H ...` / `--map_lead_bins A-B ...` -> (plane_of_lead, one entry per lead time 0 .. total_num_steps - 1 whose
    lead hour is (l + 1) * step_size_hour; the planes as they go into score_maps.json: [{"lead_hours": [...]}]).  Neither flag: one plane
    per lead time.  Hours: one plane per listed lead hour, each a lead time of the rollout, no two equal.  Bins: one plane per inclusive
    range of lead hours, pooled; A <= B, at least one lead time inside, no lead time in two bins."""
    T, step = int(total_num_steps), int(step_size_hour)
    hours = [(l + 1) * step for l in range(T)]
    if lead_hours is not None and lead_bins is not None:
        raise ValueError("--map_lead_hours and --map_lead_bins exclude each other")
    plane_of_lead, planes = [-1] * T, []
    if lead_bins is not None:
        for tok in lead_bins:
            a, sep, b = str(tok).partition("-")
            if not (sep and a.isdigit() and b.isdigit()) or int(a) > int(b):
                raise ValueError(f"--map_lead_bins {tok}: a bin is A-B in lead hours with A <= B")
            inside = [l for l in range(T) if int(a) <= hours[l] <= int(b)]
            if not inside:
                raise ValueError(f"--map_lead_bins {tok}: no lead time inside (lead hours {hours[0]} .. {hours[-1]} every {step})")
            if any(plane_of_lead[l] != -1 for l in inside):
                raise ValueError(f"--map_lead_bins {tok}: overlaps an earlier bin")
            for l in inside:
                plane_of_lead[l] = len(planes)
            planes.append(dict(lead_hours=[hours[l] for l in inside], bin=[int(a), int(b)]))
    else:
        try:
            wanted = hours if lead_hours is None else [int(str(h)) for h in lead_hours]
        except ValueError:
            raise ValueError(f"--map_lead_hours {' '.join(map(str, lead_hours))}: whole lead hours are needed") from None
        if not wanted or len(set(wanted)) != len(wanted):
            raise ValueError(f"--map_lead_hours {wanted}: at least one lead hour, no two equal")
        for h in wanted:
            if h not in hours:
                raise ValueError(f"--map_lead_hours {h}: not a lead time of the rollout (lead hours {hours[0]} .. {hours[-1]} every {step})")
            plane_of_lead[hours.index(h)] = len(planes)
            planes.append(dict(lead_hours=[h]))
    return plane_of_lead, planes
