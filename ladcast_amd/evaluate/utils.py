"""Ensemble scoring on the device (reference: ladcast/evaluate/utils.py:9-149 and the per-lead-time block of
ladcast/evaluate/evaluate_ens_gpu.py:339-425).  Same function names and argument meaning; the forecast is read once by
one fused HIP kernel (`ldc_ensemble_scores`) instead of ~40 torch ops.  Tensors must live on a HIP device: there is no
CPU path."""
from collections import namedtuple
from typing import Callable, Dict, NamedTuple, Optional

import torch

from .. import hip


def get_lat_weights_from_lat_tensor(lat: torch.Tensor) -> torch.Tensor:
    """evaluate/utils.py:9-37 (host-side table, L values)"""
    lat_rad = torch.deg2rad(lat)
    midpoints = (lat_rad[:, :-1] + lat_rad[:, 1:]) / 2
    B = lat_rad.shape[0]
    lower = torch.full((B, 1), -torch.pi / 2, dtype=lat_rad.dtype, device=lat_rad.device)
    upper = torch.full((B, 1), torch.pi / 2, dtype=lat_rad.dtype, device=lat_rad.device)
    bounds = torch.cat([lower, midpoints, upper], dim=1)
    cell_area = torch.sin(bounds[:, 1:]) - torch.sin(bounds[:, :-1])
    return cell_area / cell_area.mean(dim=1, keepdim=True)


def get_normalized_lat_weights_based_on_cos(lat: torch.Tensor) -> torch.Tensor:
    """evaluate/utils.py:40-48"""
    weights = torch.cos(torch.deg2rad(lat))
    return weights / weights.mean()


def _as_echw(forecast: torch.Tensor, ensemble_dim: int) -> torch.Tensor:
    if forecast.dim() != 4:
        raise ValueError("forecast must be (ens, C, H, W) up to the position of the ensemble axis")
    f = forecast.movedim(ensemble_dim, 0)
    if f.dtype != torch.float32:
        raise NotImplementedError("fp32 only")
    if f.stride(-1) != 1 or f.stride(-2) != f.shape[-1]:
        f = f.contiguous()
    return f


def _scores(forecast, truth, clim, lat_weight, nan_channel, want_maps):
    f = _as_echw(forecast, 0)
    M, C, H, W = f.shape
    dev = f.device
    t = truth.to(dev, torch.float32).expand(C, H, W)
    t = t if (t.stride(-1) == 1 and t.stride(-2) == W) else t.contiguous()
    c = None
    if clim is not None:
        c = clim.to(dev, torch.float32).expand(C, H, W)
        c = c if (c.stride(-1) == 1 and c.stride(-2) == W) else c.contiguous()
    w = (torch.ones(H, device=dev) if lat_weight is None else lat_weight.to(dev, torch.float32).reshape(-1)).contiguous()
    if w.numel() != H:
        raise ValueError("lat_weight must have one value per latitude row")
    out = torch.empty(5, C, device=dev, dtype=torch.float32)
    skill = torch.empty(C, H, W, device=dev) if want_maps else None
    spread = torch.empty(C, H, W, device=dev) if want_maps else None
    hip.ensemble_scores(f, t, c, w, out, M=M, C=C, H=H, W=W, member_stride=f.stride(0), channel_stride=f.stride(1),
                        truth_channel_stride=t.stride(0), clim_channel_stride=0 if c is None else c.stride(0), nan_channel=nan_channel,
                        skill_map=skill, spread_map=spread)
    return out, skill, spread


@torch.no_grad()
def pointwise_crps_skill(forecast: torch.Tensor, truth: torch.Tensor, ensemble_dim: int) -> torch.Tensor:
    """evaluate/utils.py:51-59 for a (ens, C, H, W) forecast (ensemble axis anywhere) -> (C, H, W)"""
    f = _as_echw(forecast, ensemble_dim)
    t = truth
    if t.dim() == 4:
        t = t.movedim(ensemble_dim, 0)[0]
    return _scores(f, t, None, None, -1, True)[1]


@torch.no_grad()
def pointwise_crps_spread(forecast: torch.Tensor, ensemble_dim: int) -> torch.Tensor:
    """evaluate/utils.py:62-103 -> (C, H, W)"""
    f = _as_echw(forecast, ensemble_dim)
    zeros = torch.zeros(f.shape[1:], device=f.device)
    return _scores(f, zeros, None, None, -1, True)[2]


@torch.no_grad()
def get_crps(forecast: torch.Tensor, truth: torch.Tensor, ensemble_dim: int = 0) -> torch.Tensor:
    """evaluate/utils.py:106-120 -> (C, H, W)"""
    f = _as_echw(forecast, ensemble_dim)
    t = truth
    if t.dim() == 4:
        t = t.movedim(ensemble_dim, 0)[0]
    _, skill, spread = _scores(f, t, None, None, -1, True)
    return skill - 0.5 * spread


@torch.no_grad()
def get_acc(forecast: torch.Tensor, truth: torch.Tensor, climate: torch.Tensor, lat_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """evaluate/utils.py:123-149 for (C, H, W) fields and lat_weight broadcastable as (1, H, 1) -> (C,)"""
    out, _, _ = _scores(forecast.unsqueeze(0), truth, climate, None if lat_weight is None else lat_weight.reshape(-1), -1, False)
    return out[0]


@torch.no_grad()
def ensemble_scores(dec_t: torch.Tensor, ref_t: torch.Tensor, clim_t: torch.Tensor, lat_weight: torch.Tensor, sst_channel: int) -> Dict[str, torch.Tensor]:
    """One lead time of evaluate/evaluate_ens_gpu.py:339-425: dec_t (ens, C, H, W) (any member / channel strides, e.g. a
    `[:, :, t]` view of the (ens, C, T, H, W) array), ref_t / clim_t (C, H, W), lat_weight (H,) -> (C,) device tensors
    ens_acc, ens_mse, crps_spread, crps_skill, crps; channel `sst_channel` is averaged with nanmean, the others with mean."""
    out, _, _ = _scores(dec_t, ref_t, clim_t, lat_weight, sst_channel, False)
    return dict(ens_acc=out[0], ens_mse=out[1], crps_spread=out[2], crps_skill=out[3], crps=out[4])


SCORE_NAMES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")  # the planes of the kernels' `out`, in order


def _plane_table(t: torch.Tensor, slots, C: int, L: int, H: int, W: int, what: str):
    """truth / climatology for ldc_rollout_scores: -> (tensor, slot_stride, channel_stride, host slot list).  Without slots a
    (C, L, H, W) tensor, lead l in slot l; with slots an (N, C, H, W) table.  Slots are checked here, on the host: the kernel trusts them."""
    if t.dtype != torch.float32:
        raise NotImplementedError("fp32 only")
    if slots is None:
        if tuple(t.shape) != (C, L, H, W):
            raise ValueError(f"{what} must be (C, L, H, W) = {(C, L, H, W)} without slots, got {tuple(t.shape)}")
        if t.stride(-1) != 1 or t.stride(-2) != W:
            t = t.contiguous()
        return t, t.stride(1), t.stride(0), list(range(L))
    if t.dim() != 4 or tuple(t.shape[1:]) != (C, H, W):
        raise ValueError(f"{what} must be an (N, C, H, W) = (N, {C}, {H}, {W}) table with slots, got {tuple(t.shape)}")
    slots = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
    if len(slots) != L:
        raise ValueError(f"{what}: {len(slots)} slots for {L} lead times")
    if any(not 0 <= s < t.shape[0] for s in slots):
        raise ValueError(f"{what}: slots {slots} reach outside the table's {t.shape[0]} entries")
    if t.stride(-1) != 1 or t.stride(-2) != W:
        t = t.contiguous()
    return t, t.stride(0), t.stride(1), slots


# What the ten rollout_* / validation_scores wrappers (here, in regional.py, score_maps.py and energy.py) share.  Each runs every check that needs no device first
# (ValueError, NotImplementedError): `_prologue`, its own limits, `l_off`, `out`; then `hip._dev` on the tensors it cannot take from the host.
def _forecast_view(forecast: torch.Tensor, lead_dim: int):
    """-> (f, M, C, L, H, W): the forecast as (ens, C, L, H, W) with a contiguous (H, W) plane, any member / lead / channel strides"""
    if forecast.dim() != 5 or lead_dim not in (0, 2):
        raise ValueError("forecast must be (ens, C, L, H, W), or (L, ens, C, H, W) with lead_dim=0")
    if forecast.dtype != torch.float32:
        raise NotImplementedError("fp32 only")
    f = forecast if lead_dim == 2 else forecast.permute(1, 2, 0, 3, 4)
    if f.stride(-1) != 1 or f.stride(-2) != f.shape[-1]:
        f = f.contiguous()
    return (f, *f.shape)


def _channel_affine(mean, std, C: int, dev):
    """`mean` / `std` of the fused inverse normalisation -> two contiguous fp32 (C,) vectors on `dev`, or (None, None)"""
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is None:
        return None, None
    if mean.numel() != C or std.numel() != C:
        raise ValueError(f"mean / std must hold one value per channel ({C})")
    return mean.to(dev, torch.float32).reshape(-1).contiguous(), std.to(dev, torch.float32).reshape(-1).contiguous()


def _upload_slots(slots, dev) -> torch.Tensor:
    """a host list of ints (or a list of such lists) -> an int32 device tensor, without stalling the host"""
    return hip.upload_nonblocking(torch.tensor(slots, dtype=torch.int32), dev)


# What `_prologue` found: the forecast view and its sizes; truth / clim as `_plane_table` gives them - None: the wrapper takes none,
# (None, 0, 0, None): it takes a climatology and none was given; the row weight and the channel affine on the device.
_Rollout = namedtuple("_Rollout", "f M C L H W truth clim w mn sd target_std")


def _launch_args(r: _Rollout, L_total: int, l_off: int):
    """After `hip._dev`: the slots go up in one upload.  -> (the device tensors a `hip.rollout_*` binding begins with, its common keywords)"""
    f = r.f
    kw = dict(M=r.M, C=r.C, L=r.L, H=r.H, W=r.W, member_stride=f.stride(0), lead_stride=f.stride(2), channel_stride=f.stride(1),
              mean=r.mn, std=r.sd, target_std=r.target_std, L_total=L_total, l_off=l_off)
    if r.truth is None:
        return (f,), kw
    t, kw["truth_slot_stride"], kw["truth_channel_stride"], t_slots = r.truth
    if r.clim is None:
        return (f, t, _upload_slots(t_slots, f.device), r.w), kw
    c, kw["clim_slot_stride"], kw["clim_channel_stride"], c_slots = r.clim
    slots = _upload_slots([t_slots, c_slots if c_slots is not None else t_slots], f.device)
    return (f, t, slots[0], c, None if c is None else slots[1], r.w), kw


def _prologue(forecast, lead_dim: int, mean, std, target_std: float, *, truth=None, clim=None, weight=None, members=None) -> _Rollout:
    """What every wrapper does before its own checks, in one order: the forecast view (its errors win), the ensemble size, the truth
    table, the climatology table, the row weight, the channel affine.  truth: (tensor, slots); clim: (tensor or None, slots), or None for
    a wrapper without a climatology argument; weight: (tensor, its name in error messages); members: (the entry point, its largest M)."""
    f, M, C, L, H, W = _forecast_view(forecast, lead_dim)
    if members is not None and not 1 <= M <= members[1]:
        raise ValueError(f"{M} members: {members[0]} serves 1 .. {members[1]}")
    t = None if truth is None else _plane_table(*truth, C, L, H, W, "truth")
    c = clim if clim is None else (None, 0, 0, None) if clim[0] is None else _plane_table(*clim, C, L, H, W, "clim")
    if weight is not None and weight[0].numel() != H:
        raise ValueError(f"{weight[1]} must have one value per latitude row")
    w = None if weight is None else weight[0].to(f.device, torch.float32).reshape(-1).contiguous()
    return _Rollout(f, M, C, L, H, W, t, c, w, *_channel_affine(mean, std, C, f.device), target_std)


class _Buf(NamedTuple):
    """One device buffer of a result type, stated once in the type's `_spec`: `_empty` builds it and `_out_buffers` holds an `out` to it."""

    shape: Callable  # (L_total, **the type's sizes) -> the shape; None: this call does not ask for the buffer
    dtype: torch.dtype
    fill: float  # of the columns no call has written
    lead: int  # the axis of length L_total
    unasked: str = ""  # an optional buffer the call does not ask for: "none" - it must be None; "kept" - it is left alone


def _empty(spec, L_total: int, device, **sizes) -> tuple:
    """the buffers of `spec` before any column is written"""
    shapes = [b.shape(L_total, **sizes) for b in spec]
    return tuple(None if s is None else torch.full(s, b.fill, device=device, dtype=b.dtype) for b, s in zip(spec, shapes))


def _out_buffers(spec, out, r: _Rollout, l_off: int, msg: str, room: bool = True, **sizes):
    """the buffers behind a wrapper's `out` (None without one), held to `spec`: their count, None-ness, shape, dtype, contiguity, device
    and (`room`) columns l_off .. l_off + L - 1; ValueError(msg) otherwise"""
    if out is None:
        return None
    bufs = out if isinstance(out, tuple) else getattr(out, "_buffers", None)
    ok = bufs is not None and len(bufs) == len(spec)
    if ok:
        asked = [b.shape(0, **sizes) is not None for b in spec]
        Lt = next((t.shape[b.lead] for b, t, a in zip(spec, bufs, asked) if a and isinstance(t, torch.Tensor) and t.dim() > b.lead), None)
        ok = Lt is not None and (not room or l_off + r.L <= Lt)
        for b, t, a in zip(spec, bufs, asked):
            if a:
                ok = ok and isinstance(t, torch.Tensor) and tuple(t.shape) == b.shape(Lt, **sizes) and t.dtype == b.dtype and t.is_contiguous() \
                    and t.device == r.f.device
            elif b.unasked == "none":
                ok = ok and t is None
    if not ok:
        raise ValueError(msg)
    return tuple(bufs)


@torch.no_grad()
def rollout_scores(forecast: torch.Tensor, truth: torch.Tensor, clim: Optional[torch.Tensor], lat_weight: torch.Tensor, sst_channel: int, *,
                   lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0,
                   truth_slots=None, clim_slots=None, out: Optional[Dict[str, torch.Tensor]] = None,
                   lead_offset: int = 0) -> Dict[str, torch.Tensor]:
    """Every lead time of evaluate/evaluate_ens_gpu.py:339-425 in one launch (`ldc_rollout_scores`): column l of each result holds the
    bits `ensemble_scores` gives for lead time l.

    forecast: (ens, C, L, H, W), or with `lead_dim=0` the (L, ens, C, H, W) view of the decoder's frame-major output; any member / lead /
    channel strides, the (H, W) plane contiguous.  `mean` / `std` (C,) device vectors and `target_std`: the forecast is still normalised
    and every value is de-normalised as it is loaded, (x / target_std) * std[c] + mean[c] - bit-equal to scoring
    `inverse_normalize_transform_3D(forecast, mean, std, target_std)`.  truth / clim: (C, L, H, W), or with `truth_slots` / `clim_slots`
    (one host int per lead time) an (N, C, H, W) table of which lead l reads entry slots[l] (a year of frames, the (366 x 4)
    climatology); clim None = no ACC; they are never transformed.  Returns the dict of five (C, L_total) device tensors under
    `ensemble_scores`' names: a fresh one (L_total = lead_offset + L, unwritten columns NaN), or `out` - the dict an earlier call
    returned - of which columns lead_offset .. lead_offset + L - 1 are written."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slots), clim=(clim, clim_slots), weight=(lat_weight, "lat_weight"))
    buf = _score_buffer(out, SCORE_NAMES, r, lead_offset, "rollout_scores")
    hip._dev(forecast, truth, clim, lat_weight, mean, std)
    if buf is None:
        buf, = _empty(ScoreDict._spec, lead_offset + r.L, r.f.device, n=len(SCORE_NAMES), C=r.C)
    args, kw = _launch_args(r, buf.shape[2], lead_offset)
    hip.rollout_scores(*args, buf, nan_channel=sst_channel, **kw)
    return ScoreDict(buf)


class ScoreDict(dict):
    """{name: (C, L_total) view} over one contiguous (len(names), C, L_total) device buffer: the arrays travel to the host in one copy"""

    _spec = (_Buf(lambda Lt, n, C: (n, C, Lt), torch.float32, float("nan"), 2),)

    def __init__(self, buf: torch.Tensor, names=SCORE_NAMES):
        super().__init__({k: buf[i] for i, k in enumerate(names)})
        self._buffer = buf


def _score_buffer(out, names, r: _Rollout, l_off: int, who: str):
    """the buffer behind `out`, the dict an earlier call of `who` returned, or that buffer itself; None when there is no `out`.  Room for the
    columns is left to the library, which refuses and writes nothing"""
    if out is None:
        return None
    buf = out if isinstance(out, torch.Tensor) else getattr(out, "_buffer", None)
    msg = f"out must be the dict an earlier {who} call returned (or its contiguous ({len(names)}, C, L_total) fp32 buffer)"
    return _out_buffers(ScoreDict._spec, (buf,), r, l_off, msg, room=False, n=len(names), C=r.C)[0]


VALIDATION_SCORE_NAMES = ("ens_mse", "single_mse", "crps")  # the planes of ldc_validation_scores' `out`, in order


@torch.no_grad()
def validation_scores(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, *, lead_dim: int = 2,
                      mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0, truth_slots=None,
                      out: Optional[Dict[str, torch.Tensor]] = None, lead_offset: int = 0) -> Dict[str, torch.Tensor]:
    """The three scores of the validation hook (train_AR.py:281-312) for every lead time in one launch (`ldc_validation_scores`):
        ens_mse = mean_hw[(mean_i x_i - t)^2 w],  single_mse = mean_{i,hw}[(x_i - t)^2 w],  crps = mean_hw[(skill - spread / 2) w]
    with the plain mean everywhere: one NaN among a point's members or in its truth makes the three scores of that (channel, lead time)
    NaN.  `ens_mse` and `crps` hold the bits `rollout_scores(forecast, truth, None, lat_weight, -1, ...)` gives.

    forecast, `lead_dim`, `mean` / `std` / `target_std`, truth / `truth_slots`, `out` / `lead_offset`: as `rollout_scores`.  Returns the
    dict of three (C, L_total) device tensors over one contiguous (3, C, L_total) buffer (`VALIDATION_SCORE_NAMES`); unwritten columns of
    a fresh one are NaN."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slots), weight=(lat_weight, "lat_weight"))
    buf = _score_buffer(out, VALIDATION_SCORE_NAMES, r, lead_offset, "validation_scores")
    hip._dev(forecast, truth, lat_weight, mean, std)
    if buf is None:
        buf, = _empty(ScoreDict._spec, lead_offset + r.L, r.f.device, n=len(VALIDATION_SCORE_NAMES), C=r.C)
    args, kw = _launch_args(r, buf.shape[2], lead_offset)
    hip.validation_scores(*args, buf, **kw)
    return ScoreDict(buf, VALIDATION_SCORE_NAMES)


RELIABILITY_NAMES = ("ens_mse", "ens_var", "ssr")  # the planes of ldc_rollout_reliability's `out`, in order
MAX_RELIABILITY_MEMBERS = 1024


class ReliabilityDict(dict):
    """{ens_mse, ens_var, ssr: (C, L_total) fp32; rank_hist: (C, L_total, M + 1) int32; rank_hist_weighted: the same in fp32;
    n_invalid: (C, L_total) int32} over the four device buffers `ldc_rollout_reliability` fills"""

    _spec = (_Buf(lambda Lt, M, C: (len(RELIABILITY_NAMES), C, Lt), torch.float32, float("nan"), 2), _Buf(lambda Lt, M, C: (C, Lt, M + 1), torch.int32, 0, 1),
             _Buf(lambda Lt, M, C: (C, Lt, M + 1), torch.float32, 0, 1), _Buf(lambda Lt, M, C: (C, Lt), torch.int32, 0, 1))

    def __init__(self, buf, hist, hist_w, n_invalid):
        super().__init__({k: buf[i] for i, k in enumerate(RELIABILITY_NAMES)})
        self.update(rank_hist=hist, rank_hist_weighted=hist_w, n_invalid=n_invalid)
        self._buffers = (buf, hist, hist_w, n_invalid)


def empty_reliability(M: int, C: int, L_total: int, device) -> ReliabilityDict:
    """the result of `rollout_reliability` before any column is written: scores NaN, histograms and `n_invalid` zero"""
    return ReliabilityDict(*_empty(ReliabilityDict._spec, L_total, device, M=M, C=C))


@torch.no_grad()
def rollout_reliability(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, sst_channel: int, *, lead_dim: int = 2,
                        mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0, truth_slot=None,
                        out: Optional[Dict[str, torch.Tensor]] = None, l_off: int = 0) -> Dict[str, torch.Tensor]:
    """Spread-skill ratio and rank histogram of every lead time in one launch (`ldc_rollout_reliability`; not in the reference).  Per
    grid point with members x_i, truth t: mean = sum_i x_i / M, se = (mean - t)^2, var = sum_i (x_i - mean)^2 / (M - 1) (NaN for one
    member), rank bin = #{x_i < t} + (#{x_i == t} >> 1): a truth that ties k members takes the deterministic mid-rank.
        ens_mse = <w se>,  ens_var = <w var>,  ssr = sqrt((M + 1) / M) * sqrt(ens_var / ens_mse)
    averaged with mean (one NaN point -> NaN), channel `sst_channel` with nanmean.  `rank_hist[c, l, b]` counts the points whose truth has
    rank b among the members, `rank_hist_weighted` sums their latitude weights, `n_invalid` counts the points left out: those with a NaN
    member or a NaN truth (+-inf are ordinary ordered values).  1 <= M <= 1024.

    forecast, `lead_dim`, `mean` / `std` / `target_std`: as `rollout_scores`.  truth: (C, L, H, W), or with `truth_slot` (one host int
    per lead time) an (N, C, H, W) table.  Returns a dict of device tensors with L_total = l_off + L columns (unwritten columns: NaN, empty
    histograms), or fills columns l_off .. l_off + L - 1 of `out`, the dict an earlier call returned."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), weight=(lat_weight, "lat_weight"),
                  members=("ldc_rollout_reliability", MAX_RELIABILITY_MEMBERS))
    bufs = _out_buffers(ReliabilityDict._spec, out, r, l_off, M=r.M, C=r.C, msg=(
        "out must be the dict an earlier rollout_reliability call returned for the same ensemble size and channels"))
    hip._dev(forecast, truth, lat_weight, mean, std)
    bufs = bufs or _empty(ReliabilityDict._spec, l_off + r.L, r.f.device, M=r.M, C=r.C)
    args, kw = _launch_args(r, bufs[0].shape[2], l_off)
    hip.rollout_reliability(*args, *bufs, nan_channel=sst_channel, **kw)
    return ReliabilityDict(*bufs)


SPECTRUM_NAMES = ("spec_members", "spec_mean", "spec_truth")  # the planes of ldc_rollout_spectrum's `out`, in order
MAX_SPECTRUM_MEMBERS = 1024
MIN_SPECTRUM_W, MAX_SPECTRUM_W = 4, 512


class SpectrumDict(dict):
    """{spec_members, spec_mean, spec_truth: (C, L_total, W / 2 + 1) fp32; n_invalid: (C, L_total) int32} over the two device buffers
    `ldc_rollout_spectrum` fills"""

    _spec = (_Buf(lambda Lt, C, W: (len(SPECTRUM_NAMES), C, Lt, W // 2 + 1), torch.float32, float("nan"), 2), _Buf(lambda Lt, C, W: (C, Lt), torch.int32, 0, 1))

    def __init__(self, buf, n_invalid):
        super().__init__({k: buf[i] for i, k in enumerate(SPECTRUM_NAMES)})
        self.update(n_invalid=n_invalid)
        self._buffers = (buf, n_invalid)


def empty_spectrum(C: int, L_total: int, W: int, device) -> SpectrumDict:
    """the result of `rollout_spectrum` before any column is written: spectra NaN, `n_invalid` zero"""
    return SpectrumDict(*_empty(SpectrumDict._spec, L_total, device, C=C, W=W))


@torch.no_grad()
def rollout_spectrum(forecast: torch.Tensor, truth: torch.Tensor, row_weight: torch.Tensor, *, lead_dim: int = 2,
                     mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0, truth_slot=None,
                     out: Optional[Dict[str, torch.Tensor]] = None, l_off: int = 0) -> Dict[str, torch.Tensor]:
    """Zonal power spectra of every lead time in one launch (`ldc_rollout_spectrum`; not in the reference).  Per latitude row of W points,
    for a real sequence y: Y_k = sum_j y_j exp(-2 pi i j k / W), P_k(y) = s_k |Y_k|^2 / W^2 for k = 0 .. W / 2 (s_k = 1 at k = 0 and W / 2,
    2 otherwise), so that sum_k P_k(y) = mean_j y_j^2.  With members x_i, truth t and the ensemble mean m = sum_i x_i / M:
        spec_members = <(1 / M) sum_i P_k(x_i)>,  spec_mean = <P_k(m)>,  spec_truth = <P_k(t)>,   <.> = sum_h w_h (.) / sum_h w_h
    over the rows h of positive `row_weight` that hold no NaN among their members and truth; `n_invalid` counts the rows of positive
    weight left out, and a (channel, lead time) without a valid row is NaN.  A row of weight 0 is not read: this is how a latitude band
    is selected.  The row mean is removed before the transform (P_0 is its square), so a field's large mean puts no noise floor under
    the bins k >= 1.  1 <= M <= 1024; W even, 4 <= W <= 512.

    `row_weight` (H,): non-negative.  A host tensor is checked here (ValueError for a negative or NaN weight); a device tensor is the
    caller's responsibility: the kernel treats a weight that is not > 0 as 0.  forecast, `lead_dim`, `mean` / `std` / `target_std`, truth /
    `truth_slot`, `out` / `l_off`: as `rollout_reliability`.  Returns a dict of device tensors with L_total = l_off + L columns (unwritten
    columns: NaN, `n_invalid` 0), or fills columns l_off .. l_off + L - 1 of `out`, the dict an earlier call (or `empty_spectrum`) returned."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), weight=(row_weight, "row_weight"),
                  members=("ldc_rollout_spectrum", MAX_SPECTRUM_MEMBERS))
    if r.W % 2 or not MIN_SPECTRUM_W <= r.W <= MAX_SPECTRUM_W:
        raise ValueError(f"{r.W} points per row: ldc_rollout_spectrum serves even W in {MIN_SPECTRUM_W} .. {MAX_SPECTRUM_W}")
    if not row_weight.is_cuda and not bool((row_weight >= 0).all()):  # NaN fails the comparison too
        raise ValueError("row_weight must be non-negative (0 leaves a row out) and not NaN")
    bufs = _out_buffers(SpectrumDict._spec, out, r, l_off, C=r.C, W=r.W, msg=(
        "out must be the dict an earlier rollout_spectrum call (or empty_spectrum) returned for the same channels and W"))
    hip._dev(forecast, truth, mean, std)
    bufs = bufs or _empty(SpectrumDict._spec, l_off + r.L, r.f.device, C=r.C, W=r.W)
    args, kw = _launch_args(r, bufs[0].shape[2], l_off)
    hip.rollout_spectrum(*args, *bufs, **kw)
    return SpectrumDict(*bufs)


PRODUCT_STAT_NAMES = ("mean", "std", "min", "max")  # the planes of ldc_rollout_products' `stats`, in order
MAX_PRODUCT_QUANTILES, MAX_PRODUCT_THRESHOLDS = hip.PRODUCTS_MAX_QUANTILES, hip.PRODUCTS_MAX_THRESHOLDS
MAX_PRODUCT_MEMBERS, MAX_PRODUCT_SORT_MEMBERS = hip.PRODUCTS_MAX_MEMBERS, hip.PRODUCTS_MAX_SORT_MEMBERS


class ProductsDict(dict):
    """{mean, std, min, max: (Cs, L_total, H, W); quantiles: (Q, Cs, L_total, H, W); exceed: (P, Cs, L_total, H, W)}, fp32 views over the
    three device buffers `ldc_rollout_products` fills; a buffer that is None (output not asked for) leaves its keys out"""

    _spec = tuple(_Buf(lambda Lt, Cs, H, W, n, k=k: (n[k], Cs, Lt, H, W) if n[k] else None, torch.float32, float("nan"), 2, "kept") for k in range(3))  # n: planes of each

    def __init__(self, stats, quant, exceed):
        super().__init__()
        if stats is not None:
            self.update({k: stats[i] for i, k in enumerate(PRODUCT_STAT_NAMES)})
        if quant is not None:
            self["quantiles"] = quant
        if exceed is not None:
            self["exceed"] = exceed
        self._buffers = (stats, quant, exceed)


def empty_products(Cs: int, L_total: int, H: int, W: int, device, *, n_quantiles: int = 0, n_thresholds: int = 0, stats: bool = True) -> ProductsDict:
    """the result of `rollout_products` before any column is written: NaN everywhere"""
    return ProductsDict(*_empty(ProductsDict._spec, L_total, device, Cs=Cs, H=H, W=W, n=(len(PRODUCT_STAT_NAMES) if stats else 0, n_quantiles, n_thresholds)))


@torch.no_grad()
def rollout_products(forecast: torch.Tensor, *, quantiles=(), thresholds=None, threshold_dirs=None, channels=None, stats: bool = True,
                     lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, target_std: float = 1.0,
                     out: Optional[Dict[str, torch.Tensor]] = None, l_off: int = 0) -> Dict[str, torch.Tensor]:
    """Ensemble products of every lead time in one launch (`ldc_rollout_products`; not in the reference): per grid point, with the M
    members x_i in member order, `mean` = sum_i x_i / M, `std` = sqrt(sum_i (x_i - mean)^2 / (M - 1)) (NaN for one member), `min`, `max`,
    `quantiles[k]` = numpy's `quantile(x, q_k, method="linear")` and `exceed[p]` = the fraction of members above (direction +1) or below
    (-1) `thresholds[p, channel]`.  A point with a NaN member is NaN in every product, a NaN threshold makes its plane NaN; +-inf are
    ordinary ordered values.  1 <= M <= 1024 without quantiles, M <= 64 with (the members are sorted in registers).

    `quantiles`: up to 16 values in [0, 1].  `thresholds`: (P, Cs) fp32, P <= 8, in physical units (after the inverse normalisation), one
    row per threshold and one column per selected channel; `threshold_dirs`: P values +1 / -1 (default: all +1).  `channels`: indices into
    the forecast's C channels in any order (default: all); the outputs hold these Cs channels in this order and `mean` / `std` stay
    indexed by the original channel.  `stats=False` leaves mean / std / min / max out.  forecast, `lead_dim`, `mean` / `std` /
    `target_std`: as `rollout_scores`.  Returns a `ProductsDict` of device views with L_total = l_off + L columns (unwritten columns NaN),
    or fills columns l_off .. l_off + L - 1 of `out`, the dict an earlier call (or `empty_products`) returned."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, members=("ldc_rollout_products", MAX_PRODUCT_MEMBERS))
    M, C, H, W, dev = r.M, r.C, r.H, r.W, r.f.device
    qs = [float(q) for q in (quantiles.tolist() if isinstance(quantiles, torch.Tensor) else quantiles)]
    if qs and M > MAX_PRODUCT_SORT_MEMBERS:
        raise ValueError(f"{M} members: quantiles need the members sorted in registers, at most {MAX_PRODUCT_SORT_MEMBERS}")
    if channels is None:
        chan = None
        Cs = C
    else:
        chan = [int(c) for c in (channels.tolist() if isinstance(channels, torch.Tensor) else channels)]
        if not chan or any(not 0 <= c < C for c in chan):
            raise ValueError(f"channels {chan} must be a non-empty list of indices into the forecast's {C} channels")
        Cs = len(chan)
    P = 0
    if thresholds is not None:
        thresholds = torch.as_tensor(thresholds, dtype=torch.float32)
        if thresholds.dim() != 2 or thresholds.shape[1] != Cs or thresholds.shape[0] < 1:
            raise ValueError(f"thresholds must be (P, Cs) = (P, {Cs}), one row per threshold, got {tuple(thresholds.shape)}")
        P = thresholds.shape[0]
    dirs = [1] * P if threshold_dirs is None else [int(d) for d in (threshold_dirs.tolist() if isinstance(threshold_dirs, torch.Tensor) else threshold_dirs)]
    if len(dirs) != P:
        raise ValueError(f"{len(dirs)} threshold directions for {P} thresholds")
    desc = hip.products_desc(qs, M, dirs)  # ValueError: too many, q outside [0, 1] or NaN, a direction that is not +-1
    Q = len(qs)
    if not (stats or Q or P):
        raise ValueError("nothing to compute: no stats, no quantiles, no thresholds")
    if l_off < 0:
        raise ValueError("l_off must not be negative")
    bufs = _out_buffers(ProductsDict._spec, out, r, l_off, Cs=Cs, H=H, W=W,
                                                 n=(len(PRODUCT_STAT_NAMES) if stats else 0, Q, P), msg=(
        "out must be the dict an earlier rollout_products call (or empty_products) returned for the same channels, "
        "quantiles, thresholds and grid, with room for columns l_off .. l_off + L - 1"))
    hip._dev(forecast)
    bufs = bufs or empty_products(Cs, l_off + r.L, H, W, dev, n_quantiles=Q, n_thresholds=P, stats=stats)._buffers
    st, qu, ex = (b if n else None for b, n in zip(bufs, (stats, Q, P)))  # a buffer not asked for in this call is left alone
    L_total = next(b.shape[2] for b in (st, qu, ex) if b is not None)
    chan_d = None if chan is None else _upload_slots(chan, dev)
    thr_d = None if P == 0 else (thresholds if thresholds.is_cuda else hip.upload_nonblocking(thresholds.contiguous(), dev)).contiguous()
    args, kw = _launch_args(r, L_total, l_off)
    hip.rollout_products(*args, desc, Cs=Cs, channels=chan_d, thr=thr_d, stats=st, quant=qu, exceed=ex, **kw)
    return ProductsDict(*bufs)


MAX_EVENTS, MAX_EVENT_MEMBERS = hip.EVENTS_MAX, hip.EVENTS_MAX_MEMBERS
EVENT_DIRECTIONS = {"gt": 1, "lt": -1}  # an event's direction as the command lines spell it (products.DIRECTIONS)


class Event(NamedTuple):
    """a threshold event of one channel: the value (`anomaly`: the value minus the climatology) lies above (`gt`) or below (`lt`) `threshold`"""

    channel: int
    direction: str
    threshold: float
    anomaly: bool = False


class EventsDict(dict):
    """{event_hist: (E, L_total, M + 1, 2) int32; event_hist_weighted: the same in fp32; event_n_invalid: (E, L_total) int32} over the
    three device buffers `ldc_rollout_events` fills: entry [e, l, n, o] holds the points at which n members show event e and the truth
    does (o = 1) or does not (o = 0)"""

    _spec = (_Buf(lambda Lt, M, E: (E, Lt, M + 1, 2), torch.int32, 0, 1), _Buf(lambda Lt, M, E: (E, Lt, M + 1, 2), torch.float32, 0, 1),
             _Buf(lambda Lt, M, E: (E, Lt), torch.int32, 0, 1))

    def __init__(self, hist, hist_w, n_invalid):
        super().__init__(event_hist=hist, event_hist_weighted=hist_w, event_n_invalid=n_invalid)
        self._buffers = (hist, hist_w, n_invalid)


def empty_events(M: int, E: int, L_total: int, device) -> EventsDict:
    """the result of `rollout_events` before any column is written: empty histograms, `event_n_invalid` zero"""
    return EventsDict(*_empty(EventsDict._spec, L_total, device, M=M, E=E))


def _event_list(events, C: int, has_clim: bool):
    """`events` (Event, or (channel, direction, threshold[, anomaly]) tuples) -> the (channel, dir, thr, anomaly) rows of `hip.events_desc`;
    every mistake is a ValueError"""
    rows = []
    for ev in events:
        ev = Event(*ev)
        if ev.direction not in EVENT_DIRECTIONS:
            raise ValueError(f"event {tuple(ev)}: the direction is 'gt' or 'lt'")
        c, thr = int(ev.channel), float(ev.threshold)
        if not 0 <= c < C:
            raise ValueError(f"event {tuple(ev)}: channel {c} is not one of the forecast's {C}")
        if thr != thr:
            raise ValueError(f"event {tuple(ev)}: the threshold must not be NaN")
        if ev.anomaly and not has_clim:
            raise ValueError(f"event {tuple(ev)}: an anomaly event needs the climatology (clim)")
        rows.append((c, EVENT_DIRECTIONS[ev.direction], thr, 1 if ev.anomaly else 0))
    if not 1 <= len(rows) <= MAX_EVENTS:
        raise ValueError(f"{len(rows)} events: ldc_rollout_events takes 1 .. {MAX_EVENTS} per call")
    return rows


@torch.no_grad()
def rollout_events(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, events, *, clim: Optional[torch.Tensor] = None,
                   clim_slots=None, lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
                   target_std: float = 1.0, truth_slot=None, out: Optional[Dict[str, torch.Tensor]] = None,
                   l_off: int = 0) -> Dict[str, torch.Tensor]:
    """The verification histogram of threshold events for every lead time in one launch (`ldc_rollout_events`; not in the reference).
    Per grid point of event e = `Event(channel, "gt" | "lt", threshold, anomaly)`, with the members x_i of that channel, truth t and
    climatology a: u_i = x_i and v = t, or with `anomaly` u_i = x_i - a and v = t - a (one fp32 subtraction each);
        n = #{u_i > threshold} in 0 .. M,  o = (v > threshold) in {0, 1}      ("lt": < in place of >)
    `event_hist[e, l, n, o]` counts the points, `event_hist_weighted` sums their latitude weights and `event_n_invalid[e, l]` counts the
    points left out: those with a NaN member, a NaN truth or (anomaly events) a NaN climatology; +-inf are ordinary ordered values.
    Histograms add over initial times; `event_scores` turns a (pooled) histogram into the Brier score and its decomposition, the
    reliability curve and the ROC curve.  1 <= M <= 1024, at most 32 events; thresholds in physical units.

    forecast, `lead_dim`, `mean` / `std` / `target_std`, truth / `truth_slot`, `out` / `l_off`: as `rollout_reliability`.  `clim` /
    `clim_slots`: as `rollout_scores`; needed by anomaly events only.  Returns an `EventsDict` of device tensors with L_total = l_off + L
    columns (unwritten columns: empty histograms), or fills columns l_off .. l_off + L - 1 of `out`, the dict an earlier call (or
    `empty_events`) returned for the same ensemble size and number of events."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), clim=(clim, clim_slots), weight=(lat_weight, "lat_weight"),
                  members=("ldc_rollout_events", MAX_EVENT_MEMBERS))
    desc = hip.events_desc(_event_list(events, r.C, clim is not None))
    E = desc.n_events
    if l_off < 0:
        raise ValueError("l_off must not be negative")
    bufs = _out_buffers(EventsDict._spec, out, r, l_off, M=r.M, E=E, msg=(
        "out must be the dict an earlier rollout_events call (or empty_events) returned for the same ensemble size and "
        "number of events, with room for columns l_off .. l_off + L - 1"))
    hip._dev(forecast, truth, clim, lat_weight, mean, std)
    bufs = bufs or _empty(EventsDict._spec, l_off + r.L, r.f.device, M=r.M, E=E)
    args, kw = _launch_args(r, bufs[0].shape[1], l_off)
    hip.rollout_events(*args, desc, *bufs, **kw)
    return EventsDict(*bufs)


EVENT_SCORE_NAMES = ("brier", "reliability", "resolution", "uncertainty", "bss", "base_rate", "forecast_mean", "roc_area")


def event_scores(hist_weighted) -> Dict[str, "numpy.ndarray"]:  # noqa: F821
    """Every score of a threshold event from its verification histogram, on the host in float64 (numpy; no device).

    hist_weighted: (..., M + 1, 2) weights (or counts): entry [n, o] is the weight of the points at which n of the M members showed the
    event and the truth did (o = 1) or did not (o = 0) - `event_hist_weighted` of `rollout_events`, pooled over any number of initial
    times.  With p_n = n / M, W_n = W_n0 + W_n1, W = sum_n W_n, obar = sum_n W_n1 / W and o_n = W_n1 / W_n:
        brier         sum_n [W_n0 p_n^2 + W_n1 (p_n - 1)^2] / W
        reliability   sum_n W_n (p_n - o_n)^2 / W            resolution   sum_n W_n (o_n - obar)^2 / W
        uncertainty   obar (1 - obar)                        brier = reliability - resolution + uncertainty, exactly: p takes M + 1 values
        bss           1 - brier / uncertainty (NaN when the uncertainty is 0)
        base_rate     obar                                   forecast_mean  sum_n W_n p_n / W
        rel_prob, rel_obs, rel_weight   (..., M + 1): the reliability curve (p_n, o_n, W_n / W)
        roc_pofd, roc_pod   (..., M + 2): "warn when n >= k" for k = M + 1 .. 0, from (0, 0) to (1, 1): pod_k = sum_{n >= k} W_n1 / sum_n W_n1,
                      pofd_k = sum_{n >= k} W_n0 / sum_n W_n0
        roc_area      the trapezoid rule over those points (NaN when one class is empty)
    Empty bins contribute 0 to the sums and NaN to the curve; W == 0 gives NaN throughout.  Returns a dict of float64 arrays of shape
    (...) (`EVENT_SCORE_NAMES`) and the curves."""
    import numpy as np

    h = np.asarray(hist_weighted, dtype=np.float64)
    if h.ndim < 2 or h.shape[-1] != 2 or h.shape[-2] < 2:
        raise ValueError(f"a verification histogram is (..., M + 1, 2) with M >= 1, got {h.shape}")
    M = h.shape[-2] - 1
    p = np.arange(M + 1, dtype=np.float64) / M
    w0, w1 = h[..., 0], h[..., 1]
    wn = w0 + w1
    W, W1, W0 = wn.sum(-1), w1.sum(-1), w0.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        obar = W1 / W
        on = w1 / wn  # NaN in an empty bin
        brier = (w0 * p ** 2 + w1 * (p - 1.0) ** 2).sum(-1) / W
        filled = wn > 0
        rel = np.where(filled, wn * (p - np.where(filled, on, 0.0)) ** 2, 0.0).sum(-1) / W
        res = np.where(filled, wn * (np.where(filled, on, 0.0) - obar[..., None]) ** 2, 0.0).sum(-1) / W
        unc = obar * (1.0 - obar)
        bss = np.where(unc > 0, 1.0 - brier / np.where(unc > 0, unc, 1.0), np.nan)
        bss = np.where(np.isnan(unc), np.nan, bss)
        fmean = (wn * p).sum(-1) / W
        rel_weight = wn / W[..., None]
        # "warn when n >= k", k = M + 1 (never) .. 0 (always): cumulative sums from the top bin down, a leading zero for k = M + 1
        zero = np.zeros(h.shape[:-2] + (1,))
        hits = np.concatenate([zero, np.cumsum(w1[..., ::-1], -1)], -1)
        fals = np.concatenate([zero, np.cumsum(w0[..., ::-1], -1)], -1)
        pod, pofd = hits / hits[..., -1:], fals / fals[..., -1:]  # the totals as the cumulative sums end: the curve closes at exactly (1, 1)
        area = (0.5 * (pod[..., 1:] + pod[..., :-1]) * (pofd[..., 1:] - pofd[..., :-1])).sum(-1)
        area = np.where((W1 > 0) & (W0 > 0), area, np.nan)
    return dict(brier=brier, reliability=rel, resolution=res, uncertainty=unc, bss=bss, base_rate=obar, forecast_mean=fmean, roc_area=area,
                rel_prob=np.broadcast_to(p, on.shape).copy(), rel_obs=on, rel_weight=rel_weight, roc_pofd=pofd, roc_pod=pod)


MAX_FSS_SCALES = hip.FSS_SCALES_MAX
FSS_SUM_NAMES = ("w", "w_pf", "w_po", "w_pf2", "w_po2", "w_d2")  # the six sums of ldc_rollout_fss, in order
FSS_SCORE_NAMES = ("fss", "fss_target", "obs_fraction", "fcst_fraction", "freq_bias")


class FssDict(dict):
    """{event_fss_sums: (E, S, L_total, 6) float64; event_fss_n_invalid: (E, L_total) int32} over the two device buffers `ldc_rollout_fss`
    fills: entry [e, s, l] holds the sums of `FSS_SUM_NAMES` over the contributing centres of event e at radius s"""

    _spec = (_Buf(lambda Lt, E, S: (E, S, Lt, len(FSS_SUM_NAMES)), torch.float64, 0, 2), _Buf(lambda Lt, E, S: (E, Lt), torch.int32, 0, 1))

    def __init__(self, sums, n_invalid):
        super().__init__(event_fss_sums=sums, event_fss_n_invalid=n_invalid)
        self._buffers = (sums, n_invalid)


def empty_fss(E: int, S: int, L_total: int, device) -> FssDict:
    """the result of `rollout_fss` before any column is written: zeros"""
    return FssDict(*_empty(FssDict._spec, L_total, device, E=E, S=S))


def _radius_list(radii, W: int):
    """`radii` -> a list of 1 .. 16 non-negative integers with 2 r + 1 <= W; every mistake is a ValueError"""
    rs = list(radii.tolist() if isinstance(radii, torch.Tensor) else radii)
    if not 1 <= len(rs) <= MAX_FSS_SCALES:
        raise ValueError(f"{len(rs)} radii: ldc_rollout_fss takes 1 .. {MAX_FSS_SCALES} per call")
    if any(isinstance(r, bool) or int(r) != r for r in rs):
        raise ValueError(f"radii are whole numbers of grid points, got {rs}")
    rs = [int(r) for r in rs]
    if any(r < 0 for r in rs):
        raise ValueError(f"a radius must not be negative, got {rs}")
    if any(2 * r + 1 > W for r in rs):
        raise ValueError(f"radii {rs}: a window of 2 r + 1 points must not be wider than the {W} points of a row (it would meet itself)")
    return rs


@torch.no_grad()
def rollout_fss(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, events, radii, *, clim: Optional[torch.Tensor] = None,
                clim_slots=None, lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
                target_std: float = 1.0, truth_slot=None, out: Optional[Dict[str, torch.Tensor]] = None,
                l_off: int = 0) -> Dict[str, torch.Tensor]:
    """Neighbourhood verification of threshold events for every lead time in one call (`ldc_rollout_fss`; not in the reference): the
    sufficient statistics of the fractions skill score (Roberts & Lean 2008).  Every grid point q of event e is classified exactly as in
    `rollout_events`: n(q) of the M members show the event, the truth does (o(q) = 1) or does not, and q is valid or not.  For a radius r
    in GRID POINTS the window of a centre p = (i, j) is rows i - r .. i + r clipped to the grid and columns j - r .. j + r modulo W
    (longitude is periodic); over its valid points N = #valid, Sn = sum n, So = sum o.  A centre contributes when it is valid itself.  In
    float64, each operation rounded on its own, with w = lat_weight[i]:
        Pf = Sn / (M N),  Po = So / N,  a = w Pf,  b = w Po,  d = Pf - Po,   terms (w, a, b, a Pf, b Po, (w d) d)
    `event_fss_sums[e, s, l]` holds the sums of the six terms over the contributing centres, `event_fss_n_invalid[e, l]` the centres left
    out (equal to `event_n_invalid` of `rollout_events`).  Sums add over initial times; `fss_scores` turns (pooled) sums into the
    score.  The window is not corrected for the convergence of the meridians: its width in kilometres shrinks towards the poles.
    1 <= M <= 1024, at most 32 events and 16 radii, 2 r + 1 <= W.

    Every other argument, `out` / `l_off` included, as `rollout_events`.  Returns an `FssDict` of device tensors with L_total = l_off + L
    columns (unwritten columns: zeros), or fills columns l_off .. l_off + L - 1 of `out`, the dict an earlier call (or `empty_fss`)
    returned for the same number of events and radii."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), clim=(clim, clim_slots), weight=(lat_weight, "lat_weight"),
                  members=("ldc_rollout_fss", MAX_EVENT_MEMBERS))
    desc = hip.events_desc(_event_list(events, r.C, clim is not None))
    rs = _radius_list(radii, r.W)
    E, S = desc.n_events, len(rs)
    if l_off < 0:
        raise ValueError("l_off must not be negative")
    bufs = _out_buffers(FssDict._spec, out, r, l_off, E=E, S=S, msg=(
        "out must be the dict an earlier rollout_fss call (or empty_fss) returned for the same number of events and "
        "radii, with room for columns l_off .. l_off + L - 1"))
    hip._dev(forecast, truth, clim, lat_weight, mean, std)
    bufs = bufs or _empty(FssDict._spec, l_off + r.L, r.f.device, E=E, S=S)
    args, kw = _launch_args(r, bufs[0].shape[2], l_off)
    hip.rollout_fss(*args, desc, rs, *bufs, **kw)
    return FssDict(*bufs)


def fss_scores(sums, radii=None) -> Dict[str, "numpy.ndarray"]:  # noqa: F821
    """The fractions skill score and its companions from the sums of `rollout_fss`, on the host in float64 (numpy; no device).

    sums: (..., 6) = (s0 .. s5) = the sums of `FSS_SUM_NAMES`, pooled over any number of initial times.
        fss            1 - s5 / (s3 + s4), NaN where the denominator is 0 (no event in forecast and truth)
        obs_fraction   s2 / s0            fcst_fraction  s1 / s0            freq_bias  s1 / s2
        fss_target     0.5 + obs_fraction / 2: the level from which a forecast counts as useful (Roberts & Lean 2008)
    With `radii` (one per entry of the scale axis, which is axis -3 of `sums`: (..., S, L, 6)) also
        useful_scale   (..., L) int64: the smallest of `radii` at which fss >= fss_target, -1 where there is none
    A NaN score compares false.  s0 == 0 gives NaN fractions."""
    import numpy as np

    s = np.asarray(sums, dtype=np.float64)
    if s.ndim < 1 or s.shape[-1] != len(FSS_SUM_NAMES):
        raise ValueError(f"fss sums are (..., {len(FSS_SUM_NAMES)}), got {s.shape}")
    s0, s1, s2, s3, s4, s5 = (s[..., k] for k in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        den = s3 + s4
        fss = np.where(den > 0, 1.0 - s5 / np.where(den > 0, den, 1.0), np.nan)
        fss = np.where(np.isnan(den), np.nan, fss)
        obs, fc, bias = s2 / s0, s1 / s0, s1 / s2
        target = 0.5 + obs / 2.0
    res = dict(fss=fss, fss_target=target, obs_fraction=obs, fcst_fraction=fc, freq_bias=bias)
    if radii is not None:
        r = np.asarray(list(radii), dtype=np.int64)
        if s.ndim < 3 or r.ndim != 1 or s.shape[-3] != r.shape[0]:
            raise ValueError(f"{r.shape[0] if r.ndim == 1 else r.shape} radii for sums of shape {s.shape}: the scale axis is axis -3")
        with np.errstate(invalid="ignore"):
            useful = fss >= target  # (..., S, L); NaN compares false
        big = np.iinfo(np.int64).max
        cand = np.where(useful, r.reshape((-1, 1)), big).min(-2)
        res["useful_scale"] = np.where(cand == big, -1, cand)
    return res
