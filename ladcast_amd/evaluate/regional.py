"""Regional ensemble scores (`ldc_rollout_regional`, csrc/regional.hip; not in the reference): the regions of a
scorecard as bit masks over the grid, one launch per decode batch that returns the additive sufficient statistics of every region at
once, and the scores derived from them on the host in float64.

    regions = [NAMED_REGIONS["tropics"], NAMED_REGIONS["europe"], Region("alps", 43, 49, 5, 17, surface="land")]
    mask = region_mask(regions, row_latitudes(H), longitude_grid(), land_sea_mask)        # uint32 (H, W), bit r = region r
    out = rollout_regional(forecast, truth, lat_weight, mask, len(regions), clim=clim)    # regional_sums (R, C, L, 10) fp64, regional_counts
    scores = regional_scores(out["regional_sums"].cpu().numpy(), out["regional_counts"].cpu().numpy(), M)

The sums ADD over initial times: summing `regional_sums` (and `regional_counts`) of many initial times before `regional_scores` gives
the scores pooled over all their points - no average of averages.  That is the point of the design."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence

import numpy as np
import torch

from .. import hip
from .utils import _Buf, _empty, _launch_args, _out_buffers, _prologue

MAX_REGIONS, MAX_REGIONAL_MEMBERS = hip.REGIONS_MAX, hip.REGIONAL_MAX_MEMBERS
N_SUMS, N_COUNTS = hip.REGIONAL_SUMS, hip.REGIONAL_COUNTS
# the 10 sums of one (region, channel, lead time): over the valid points, then over the ACC-valid points
SUM_NAMES = ("w", "w_e", "w_se", "w_var", "w_skill", "w_spread", "acc_w", "acc_fa_ta", "acc_fa_fa", "acc_ta_ta")
COUNT_NAMES = ("n_valid", "n_invalid", "n_acc_valid")
REGIONAL_KEYS = ("regional_sums", "regional_counts")
REGIONAL_SCORE_NAMES = ("bias", "ens_mse", "rmse", "ens_var", "ssr", "crps_skill", "crps_spread", "crps", "ens_acc", "weight", "n_valid")
SURFACES = (None, "land", "sea")


class Region(NamedTuple):
    """a latitude / longitude box in degrees north and east, both latitude bounds inclusive; the longitudes live on [0, 360) (negative
    inputs are taken modulo 360) and `lon_min > lon_max` is a box across the 0 degree meridian; `surface`: None, "land" or "sea".  A
    tuple of boxes in `boxes` (same surface) makes the region their union."""

    name: str
    lat_min: float
    lat_max: float
    lon_min: float
    lon_max: float
    surface: Optional[str] = None
    boxes: tuple = ()  # further (lat_min, lat_max, lon_min, lon_max) boxes united with the first


_ALL_LON = (0.0, 360.0)  # lon_max = 360: every longitude of [0, 360)
NAMED_REGIONS: Dict[str, Region] = {r.name: r for r in (
    Region("global", -90.0, 90.0, *_ALL_LON),
    Region("tropics", -20.0, 20.0, *_ALL_LON),
    Region("extratropics", 20.0, 90.0, *_ALL_LON, boxes=((-90.0, -20.0, *_ALL_LON),)),  # |lat| >= 20: the union of the next two
    Region("nh_extratropics", 20.0, 90.0, *_ALL_LON),
    Region("sh_extratropics", -90.0, -20.0, *_ALL_LON),
    Region("arctic", 60.0, 90.0, *_ALL_LON),
    Region("antarctic", -90.0, -60.0, *_ALL_LON),
    Region("europe", 35.0, 75.0, 347.5, 42.5),
    Region("north_america", 25.0, 60.0, 240.0, 285.0),
    Region("north_atlantic", 25.0, 65.0, 290.0, 350.0),
    Region("north_pacific", 25.0, 60.0, 145.0, 230.0),
    Region("east_asia", 25.0, 60.0, 102.5, 150.0),
    Region("ausnz", -45.0, -12.5, 120.0, 175.0),
)}


def _box(lat: np.ndarray, lon: np.ndarray, lat_min, lat_max, lon_min, lon_max) -> np.ndarray:
    lat_min, lat_max, lon_min, lon_max = float(lat_min), float(lat_max), float(lon_min), float(lon_max)
    if not lat_min <= lat_max:
        raise ValueError(f"a region's lat_min ({lat_min}) must not exceed its lat_max ({lat_max})")
    rows = (lat >= lat_min) & (lat <= lat_max)
    if lon_max - lon_min >= 360.0:
        cols = np.ones(lon.shape, dtype=bool)
    else:
        lo, hi = lon_min % 360.0, lon_max % 360.0
        cols = (lon >= lo) & (lon <= hi) if lo <= hi else (lon >= lo) | (lon <= hi)  # lo > hi: the box crosses the 0 degree meridian
    return rows[:, None] & cols[None, :]


def region_mask(regions: Sequence[Region], lat_deg, lon_deg, land_sea_mask=None) -> np.ndarray:
    """-> uint32 (H, W): bit r of entry (i, j) is set when the point (lat_deg[i], lon_deg[j]) lies in regions[r].  Latitude bounds are
    inclusive, and so are the longitude bounds; lon_deg is taken modulo 360.  `surface="land"` keeps the points with
    `land_sea_mask >= 0.5`, "sea" the others; a region with a surface needs the (H, W) mask.  At most 32 regions."""
    regions = [r if isinstance(r, Region) else Region(*r) for r in regions]
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError(f"{len(regions)} regions: a mask word holds 1 .. {MAX_REGIONS}")
    lat = np.asarray(lat_deg, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon_deg, dtype=np.float64).reshape(-1) % 360.0
    land = None
    if land_sea_mask is not None:
        lsm = np.asarray(land_sea_mask)
        if lsm.shape != (lat.size, lon.size):
            raise ValueError(f"land_sea_mask must be (H, W) = {(lat.size, lon.size)}, got {lsm.shape}")
        land = lsm >= 0.5
    mask = np.zeros((lat.size, lon.size), dtype=np.uint32)
    for r, reg in enumerate(regions):
        if reg.surface not in SURFACES:
            raise ValueError(f"region {reg.name!r}: surface is 'land', 'sea' or None, got {reg.surface!r}")
        if reg.surface is not None and land is None:
            raise ValueError(f"region {reg.name!r} is restricted to {reg.surface}: it needs the land_sea_mask")
        inside = _box(lat, lon, reg.lat_min, reg.lat_max, reg.lon_min, reg.lon_max)
        for b in reg.boxes:
            inside |= _box(lat, lon, *b)
        if reg.surface is not None:
            inside &= land if reg.surface == "land" else ~land
        mask |= inside.astype(np.uint32) << np.uint32(r)
    return mask


def region_metadata(regions: Sequence[Region], mask: np.ndarray, lat_weight) -> list:
    """what regions.json holds per region: its name, box(es), surface, point count and the sum of `lat_weight` over its points"""
    w = np.broadcast_to(np.asarray(lat_weight, dtype=np.float64).reshape(-1, 1), mask.shape)
    meta = []
    for r, reg in enumerate(regions):
        inside = (mask >> np.uint32(r)) & np.uint32(1) == 1
        boxes = [[reg.lat_min, reg.lat_max, reg.lon_min, reg.lon_max]] + [list(b) for b in reg.boxes]
        meta.append(dict(name=reg.name, boxes=boxes, surface=reg.surface, n_points=int(inside.sum()), weight=float(w[inside].sum())))
    return meta


def regional_scores(sums, counts, M: int) -> Dict[str, np.ndarray]:
    """The scores of every (region, channel, lead time) from the sufficient statistics, on the host in float64 (numpy; no device).

    sums (..., 10) = S0 .. S9 and counts (..., 3) of `rollout_regional`, for one initial time or SUMMED over any number of them: the
    result is then the score pooled over all their points.  With S0 = sum w over the valid points:
        bias = S1 / S0              ens_mse = S2 / S0           rmse = sqrt(ens_mse)        ens_var = S3 / S0
        ssr = sqrt((M + 1) / M) * sqrt(ens_var / ens_mse)       (NaN at M == 1)
        crps_skill = S4 / S0        crps_spread = S5 / S0       crps = crps_skill - crps_spread / 2
        ens_acc = S7 / sqrt(S8 * S9)                            (over the ACC-valid points; NaN without a climatology)
        weight = S0                 n_valid = counts[..., 0]
    An empty region, or one without a valid point, gives NaN.  The scale of the weights cancels in every score but `weight`."""
    s = np.asarray(sums, dtype=np.float64)
    n = np.asarray(counts)
    if s.shape[-1] != N_SUMS or n.shape[-1] != N_COUNTS or s.shape[:-1] != n.shape[:-1]:
        raise ValueError(f"sums must be (..., {N_SUMS}) and counts (..., {N_COUNTS}) with the same leading dimensions, got {s.shape} and {n.shape}")
    M = int(M)
    if M < 1:
        raise ValueError("at least one member")
    n_valid, n_acc = n[..., 0].astype(np.int64), n[..., 2].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        s0 = np.where(n_valid > 0, s[..., 0], np.nan)
        bias, mse, var, skill, spread = (s[..., k] / s0 for k in (1, 2, 3, 4, 5))
        ssr = np.sqrt((M + 1.0) / M) * np.sqrt(var / mse) if M > 1 else np.full(mse.shape, np.nan)
        acc = np.where(n_acc > 0, s[..., 7] / np.sqrt(s[..., 8] * s[..., 9]), np.nan)
    return dict(bias=bias, ens_mse=mse, rmse=np.sqrt(mse), ens_var=var, ssr=ssr, crps_skill=skill, crps_spread=spread, crps=skill - spread / 2,
                ens_acc=acc, weight=np.where(n_valid > 0, s[..., 0], 0.0), n_valid=n_valid)


class RegionalDict(dict):
    """{regional_sums: (R, C, L_total, 10) fp64; regional_counts: (R, C, L_total, 3) int32} over the two device buffers
    `ldc_rollout_regional` fills (`SUM_NAMES`, `COUNT_NAMES`)"""

    _spec = (_Buf(lambda Lt, R, C: (R, C, Lt, N_SUMS), torch.float64, 0, 2), _Buf(lambda Lt, R, C: (R, C, Lt, N_COUNTS), torch.int32, 0, 2))

    def __init__(self, sums, counts):
        super().__init__(regional_sums=sums, regional_counts=counts)
        self._buffers = (sums, counts)


def empty_regional(R: int, C: int, L_total: int, device) -> RegionalDict:
    """the result of `rollout_regional` before any column is written: all sums and counts zero"""
    return RegionalDict(*_empty(RegionalDict._spec, L_total, device, R=R, C=C))


def mask_words(mask, H: int, W: int) -> torch.Tensor:
    """a region mask (numpy uint32 / int32 / int64 array or tensor, (H, W)) -> a contiguous int32 host tensor of the same bits"""
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.shape != (H, W):
        raise ValueError(f"region_mask must be (H, W) = {(H, W)}, got {m.shape}")
    if m.dtype.kind not in "iu":
        raise ValueError(f"region_mask must hold integer words, got {m.dtype}")
    if m.dtype.itemsize > 4:
        if ((m < -(1 << 31)) | (m >= (1 << 32))).any():
            raise ValueError("region_mask words must fit 32 bits")
        m = (m.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    return torch.from_numpy(np.ascontiguousarray(m.astype(np.uint32, copy=False)).view(np.int32).copy())


@torch.no_grad()
def rollout_regional(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, region_mask, n_regions: int, *,
                     clim: Optional[torch.Tensor] = None, clim_slots=None, lead_dim: int = 2, mean: Optional[torch.Tensor] = None,
                     std: Optional[torch.Tensor] = None, target_std: float = 1.0, truth_slot=None, out: Optional[Dict[str, torch.Tensor]] = None,
                     l_off: int = 0) -> Dict[str, torch.Tensor]:
    """The sufficient statistics of the regional scores for every lead time in one launch (`ldc_rollout_regional`; not in the reference).
    `region_mask`: (H, W) words of which bit r < `n_regions` <= 32 says that the point belongs to region r (`region_mask()`); a device
    int32 tensor is used where it lies.  Per point of at least one region, all fp32: mean, e = mean - t, se = e^2, var (two-pass, ddof 1;
    0 at one member), skill = mean_i |t - x_i|, spread (sorted members; 0 at one member), fa = mean - a, ta = t - a.  A point is valid
    when no member and not the truth is NaN, ACC-valid when the climatology is not NaN either; in every channel the invalid points are
    left out and counted (no mean / nanmean distinction).  `regional_sums[r, c, l]` = sum over the valid points of region r of
    w, w e, w se, w var, w skill, w spread, then over its ACC-valid points of w, w fa ta, w fa^2, w ta^2 (zeros without `clim`), in
    fp64; `regional_counts[r, c, l]` = valid, invalid, ACC-valid points.  1 <= M <= 64.  `regional_scores` derives the scores.

    forecast, `lead_dim`, `mean` / `std` / `target_std`, truth / `truth_slot`, `clim` / `clim_slots`, `out` / `l_off`: as
    `rollout_events`.  Returns a `RegionalDict` of device tensors with L_total = l_off + L columns (unwritten columns: zeros), or fills
    columns l_off .. l_off + L - 1 of `out`, the dict an earlier call (or `empty_regional`) returned for the same R and C."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), clim=(clim, clim_slots), weight=(lat_weight, "lat_weight"),
                  members=("ldc_rollout_regional", MAX_REGIONAL_MEMBERS))
    H, W, dev = r.H, r.W, r.f.device
    R = int(n_regions)
    if not 1 <= R <= MAX_REGIONS:
        raise ValueError(f"{R} regions: ldc_rollout_regional takes 1 .. {MAX_REGIONS} per call")
    if isinstance(region_mask, torch.Tensor) and region_mask.is_cuda:
        if region_mask.dtype != torch.int32 or tuple(region_mask.shape) != (H, W):
            raise ValueError(f"a device region_mask must be int32 (H, W) = {(H, W)}")
        words = region_mask.contiguous()
    else:
        words = mask_words(region_mask, H, W)
    if l_off < 0:
        raise ValueError("l_off must not be negative")
    bufs = _out_buffers(RegionalDict._spec, out, r, l_off, R=R, C=r.C, msg=(
        "out must be the dict an earlier rollout_regional call (or empty_regional) returned for the same number of regions "
        "and channels, with room for columns l_off .. l_off + L - 1"))
    hip._dev(forecast, truth, clim, lat_weight, mean, std)
    bufs = bufs or _empty(RegionalDict._spec, l_off + r.L, dev, R=R, C=r.C)
    if not words.is_cuda:
        words = hip.upload_nonblocking(words, dev)
    args, kw = _launch_args(r, bufs[0].shape[2], l_off)
    hip.rollout_regional(*args, words, *bufs, R=R, **kw)
    return RegionalDict(*bufs)
