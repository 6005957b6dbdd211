"""Derived fields (not in the reference): quantities that are no decoded channel but a function of a few of them - wind speed
sqrt(u^2 + v^2), a difference such as the 500 - 1000 hPa thickness, the vertical wind shear sqrt((u1 - u2)^2 + (v1 - v2)^2) - computed
on the device from the de-normalised channels (`ldc_derive_fields`) and appended to the decode batch, the truth and the climatology as
channels C', C' + 1, ...: every scorer and `products` then verify them as they verify a decoded channel.  A score of a nonlinear
field is no function of its components' scores, and the members exist only for the length of a decode batch: the derivation happens
where the batch lies.

    python -m ladcast_amd.evaluate.evaluate_ens_gpu ... --derive wind_speed_10m speed 10m_u_component_of_wind 10m_v_component_of_wind \\
        --derive thickness_500_1000 diff geopotential_level500 geopotential_level1000 --event wind_speed_10m gt 17.2

Arithmetic: `diff` is one fp32 subtraction of the de-normalised inputs; `speed` and `shear` take differences, squares, sum and root
in double and round once to fp32, so nothing overflows, underflows or depends on contraction.  A derived field reads decoded channels
only, never another derived field.

`vorticity` and `divergence` of a wind (u, v) need horizontal derivatives (`ldc_derive_sphere`): centred
differences on the latitude-longitude grid in double, the polar-cap mean on a pole row, one rounding to fp32.  The per-row constants
are made here, in float64 (`sphere_row_tables`).  Both are linear in (u, v): their climatology is the field of the climatology.

        --derive vort850 vorticity u_component_of_wind_level850 v_component_of_wind_level850 --event_anomaly vort850 gt 5e-5"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from .utils import Event, _channel_affine, _forecast_view, _plane_table, _upload_slots

SPHERE_KINDS = {"vorticity": hip.SPHERE_VORTICITY, "divergence": hip.SPHERE_DIVERGENCE}  # served by ldc_derive_sphere; channels (u, v)
KINDS = {"speed": hip.DERIVE_SPEED, "diff": hip.DERIVE_DIFF, "shear": hip.DERIVE_SHEAR, **SPHERE_KINDS}  # the code within the kind's entry point
KIND_CHANNELS = {"speed": 2, "diff": 2, "shear": 4, "vorticity": 2, "divergence": 2}  # (a, b), (a, b), (a, b, c, d), (u, v), (u, v)
NONLINEAR_KINDS = ("speed", "shear")  # the climatology of the field is not the field of the climatology
MAX_DERIVED = hip.DERIVE_MAX_FIELDS
EARTH_RADIUS_M = 6_371_000.0
POLE_TOLERANCE_DEG = 1e-6  # a row within this of +-90 degrees is a pole row
SPHERE_SCALE_LENGTH_M = 1.0e5  # a sphere field's default energy scale: a wind difference of one standard deviation over 100 km


class Derived(NamedTuple):
    """a derived field: `speed` sqrt(a^2 + b^2), `diff` a - b or `shear` sqrt((a - c)^2 + (b - d)^2) of the DECODED channels
    `channels` = (a, b[, c, d]), or the relative `vorticity` / the `divergence` of the wind `channels` = (u, v); `scale`: what an
    energy-score group divides this channel by (default: sqrt(sum of std[c]^2 over its source channels), the standard deviation of a
    difference of independent components; for a sphere field that over `SPHERE_SCALE_LENGTH_M`)"""

    name: str
    kind: str
    channels: Tuple[int, ...]
    scale: Optional[float] = None


def _field_list(derived, C: int) -> List[Derived]:
    """`derived` (Derived, or (name, kind, channels[, scale]) tuples) checked against the C decoded channels; every mistake is a ValueError"""
    fields = [Derived(*d) for d in derived]
    if not 1 <= len(fields) <= MAX_DERIVED:
        raise ValueError(f"{len(fields)} derived fields: ldc_derive_fields takes 1 .. {MAX_DERIVED} per call")
    out = []
    for f in fields:
        if f.kind not in KINDS:
            raise ValueError(f"derived field {f.name!r}: kind {f.kind!r} is not one of {sorted(KINDS)}")
        ch = tuple(int(c) for c in f.channels)
        if len(ch) != KIND_CHANNELS[f.kind]:
            raise ValueError(f"derived field {f.name!r}: {f.kind} reads {KIND_CHANNELS[f.kind]} channels, got {len(ch)}")
        if any(not 0 <= c < C for c in ch):
            raise ValueError(f"derived field {f.name!r}: channels {list(ch)} are not all among the {C} decoded channels")
        if f.scale is not None and not (0.0 < float(f.scale) < math.inf):
            raise ValueError(f"derived field {f.name!r}: the scale must be positive and finite, got {f.scale}")
        out.append(f._replace(channels=ch))
    return out


def sphere_row_tables(lat_deg, W: int) -> Tuple[np.ndarray, float]:
    """The per-row constants of `ldc_derive_sphere` for rows at latitudes `lat_deg` (degrees, H of them, strictly ascending or
    descending, any spacing) and W longitudes on a full circle -> (float64 (4, H) = c, q, r, pc, and k), all made in float64 with numpy:
    the kernel and a host reference that take them from here share their bits.  With phi in radians, jn = min(j + 1, H - 1),
    js = max(j - 1, 0) and a pole row one with 90 - |lat| < 1e-6:
        c[j] = cos(phi[j]), exactly 0 on a pole row (a pole neighbour then drops out of the meridional difference by itself)
        q[j] = 1 / (phi[jn] - phi[js])       the sign is right for either order of the rows
        r[j] = 1 / (R c[j]), exactly 0 on a pole row: that marks the row for the kernel
        pc[j] = s c[jp] / (R (1 - s sin(phi[jp]))) on a pole row, s = +1 at the north pole and -1 at the south pole, jp the one
                adjacent row: circulation (or outward flux) around the adjacent latitude circle over the area of the cap it bounds
        k = 1 / (2 (2 pi / W))
    ValueError: H < 2, W < 3, latitudes that are not finite and strictly monotonic, |lat| > 90 + 1e-6, a pole row that is not the
    first or the last."""
    lat = np.asarray(lat_deg, dtype=np.float64).reshape(-1)
    H, W = int(lat.size), int(W)
    if H < 2 or W < 3:
        raise ValueError(f"a sphere field needs H >= 2 rows and W >= 3 longitudes, got H = {H}, W = {W}")
    step = np.diff(lat)
    if not np.isfinite(lat).all() or not (bool((step > 0).all()) or bool((step < 0).all())):
        raise ValueError("the row latitudes must be finite and strictly ascending or strictly descending")
    if bool((np.abs(lat) > 90.0 + POLE_TOLERANCE_DEG).any()):
        raise ValueError("the row latitudes must lie within [-90, 90] degrees")
    pole = 90.0 - np.abs(lat) < POLE_TOLERANCE_DEG
    if bool(pole[1:-1].any()):
        raise ValueError("a pole row can only be the first or the last row")
    phi = np.deg2rad(lat)
    jn, js = np.minimum(np.arange(H) + 1, H - 1), np.maximum(np.arange(H) - 1, 0)
    c = np.where(pole, 0.0, np.cos(phi))
    q = 1.0 / (phi[jn] - phi[js])
    r = np.zeros(H)
    r[~pole] = 1.0 / (EARTH_RADIUS_M * c[~pole])
    pc = np.zeros(H)
    for j in np.flatnonzero(pole):
        jp = 1 if j == 0 else H - 2
        s = 1.0 if lat[j] > 0 else -1.0
        pc[j] = s * c[jp] / (EARTH_RADIUS_M * (1.0 - s * np.sin(phi[jp])))
    k = 1.0 / (2.0 * (2.0 * np.pi / W))
    return np.stack([c, q, r, pc]), float(k)


_HOST_TABLES = {}  # (latitude bytes or the default grid's H, W) -> (latitudes, (float64 (4, H), k)): checked and made once per grid
_ROW_TABLES = {}  # (latitude bytes, W, device) -> (device fp64 (4, H), k): a run uses one grid, a handful at most


def _host_row_tables(lat_deg, H: int, W: int):
    """-> (latitudes, `sphere_row_tables` of them) for the (H, W) grid; `lat_deg` None: the rows every driver here scores on.  Every
    mistake is a ValueError."""
    if lat_deg is None:
        key = (int(H), int(W))
        if key not in _HOST_TABLES:
            from .rollout_metrics import row_latitudes

            lat = np.ascontiguousarray(row_latitudes(H), dtype=np.float64)
            _HOST_TABLES[key] = (lat, sphere_row_tables(lat, W))
        return _HOST_TABLES[key]
    lat = np.ascontiguousarray(lat_deg.detach().cpu().numpy() if isinstance(lat_deg, torch.Tensor) else lat_deg, dtype=np.float64).reshape(-1)
    if lat.size != H:
        raise ValueError(f"lat_deg holds {lat.size} latitudes, the planes have {H} rows")
    key = (lat.tobytes(), int(W))
    if key not in _HOST_TABLES:
        if len(_HOST_TABLES) >= 16:
            _HOST_TABLES.clear()
        _HOST_TABLES[key] = (lat, sphere_row_tables(lat, W))
    return _HOST_TABLES[key]


def _device_row_tables(lat: np.ndarray, host, W: int, dev):
    key = (lat.tobytes(), int(W), str(torch.device(dev)))
    if key not in _ROW_TABLES:
        if len(_ROW_TABLES) >= 16:
            _ROW_TABLES.clear()
        _ROW_TABLES[key] = (torch.from_numpy(host[0]).to(dev), host[1])
    return _ROW_TABLES[key]


def _runs(fields: Sequence[Derived]):
    """the maximal runs of fields of one family, in the caller's order: [(first output channel, fields, sphere?)] - one launch each"""
    runs = []
    for k, f in enumerate(fields):
        sphere = f.kind in SPHERE_KINDS
        if runs and runs[-1][2] == sphere:
            runs[-1][1].append(f)
        else:
            runs.append((k, [f], sphere))
    return runs


def _launch_runs(fields, src, out, channel_axis: int, common: dict, H: int, W: int, tables):
    """Each run of point-wise fields goes to `ldc_derive_fields`, each run of sphere fields to `ldc_derive_sphere`, `out` narrowed to the
    run's channels: a field's bits do not depend on what else the list holds.  tables: `_device_row_tables`' pair, None without a
    sphere field."""
    for k0, run, sphere in _runs(fields):
        o = out.narrow(channel_axis, k0, len(run))
        if sphere:
            hip.derive_sphere(src, o, hip.sphere_desc([(KINDS[f.kind], f.channels) for f in run]), tables[0], tables[1], H=H, W=W, **common)
        else:
            hip.derive_fields(src, o, hip.derive_desc([(KINDS[f.kind], f.channels) for f in run]), HW=H * W, **common)


def _out_view(out, shape, what: str):
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.stride(-1) != 1 \
            or out.stride(-2) != shape[-1]:
        raise ValueError(f"out must be an fp32 {what} = {tuple(shape)} tensor (any view with a contiguous (H, W) plane)")


@torch.no_grad()
def derive_forecast(forecast: torch.Tensor, derived, *, lead_dim: int = 2, mean: Optional[torch.Tensor] = None,
                    std: Optional[torch.Tensor] = None, target_std: float = 1.0, out: Optional[torch.Tensor] = None, lat_deg=None) -> torch.Tensor:
    """The D derived fields of a forecast in physical units, one `ldc_derive_fields` / `ldc_derive_sphere` call per run of fields of one
    family (a list of one family: one call): -> (ens, D, L, H, W), or with `lead_dim=0` (L, ens, D, H, W).  forecast, `lead_dim`,
    `mean` / `std` / `target_std`: as `rollout_scores` - an input holds the bits the scorers load for that channel; mean None: the
    forecast is physical already.  `out`: a tensor of the result's shape to write to, any view with a contiguous (H, W) plane, e.g. the
    tail channels of an extended (L, ens, C + D, H, W) tensor whose head is the forecast.  `lat_deg`: the H row latitudes in degrees
    for `vorticity` / `divergence` (`sphere_row_tables` states what is accepted); None: `rollout_metrics.row_latitudes(H)`."""
    f, M, C, L, H, W = _forecast_view(forecast, lead_dim)
    fields = _field_list(derived, C)
    D = len(fields)
    rows = _host_row_tables(lat_deg, H, W) if any(fl.kind in SPHERE_KINDS for fl in fields) else None
    mn, sd = _channel_affine(mean, std, C, f.device)
    shape = (M, D, L, H, W) if lead_dim == 2 else (L, M, D, H, W)
    if out is not None:
        _out_view(out, shape, "(ens, D, L, H, W)" if lead_dim == 2 else "(L, ens, D, H, W)")
    hip._dev(forecast, mean, std, out)
    if out is None:
        out = torch.empty(shape, device=f.device, dtype=torch.float32)
    o = out if lead_dim == 2 else out.permute(1, 2, 0, 3, 4)
    common = dict(outer_stride=f.stride(0), lead_stride=f.stride(2), channel_stride=f.stride(1), n_outer=M, L=L, C=C, out_outer_stride=o.stride(0),
                  out_lead_stride=o.stride(2), out_channel_stride=o.stride(1), mean=mn, std=sd, target_std=target_std)
    _launch_runs(fields, f, o, 1, common, H, W, None if rows is None else _device_row_tables(rows[0], rows[1], W, f.device))
    return out


@torch.no_grad()
def derive_table(table: torch.Tensor, slots, derived, *, out: Optional[torch.Tensor] = None, lat_deg=None) -> torch.Tensor:
    """The D derived fields of a truth / climatology table, which is physical and never transformed: -> (L, D, H, W).  With `slots` (one
    host int per lead time) `table` is (N, C, H, W) and lead l reads entry slots[l]; with slots None it is a (C, L, H, W) tensor.
    Slots are checked here, on the host.  `out`, `lat_deg`: as `derive_forecast`, `out` of shape (L, D, H, W)."""
    if not isinstance(table, torch.Tensor) or table.dim() != 4:
        raise ValueError("table must be (N, C, H, W) with slots, or (C, L, H, W) without")
    if slots is None:
        C, L, H, W = table.shape
    else:
        slots = [int(s) for s in (slots.tolist() if isinstance(slots, torch.Tensor) else slots)]
        (_, C, H, W), L = table.shape, len(slots)
    if L < 1:
        raise ValueError("at least one lead time")
    fields = _field_list(derived, C)
    D = len(fields)
    t, lead_stride, channel_stride, _ = _plane_table(table, slots, C, L, H, W, "table")
    rows = _host_row_tables(lat_deg, H, W) if any(fl.kind in SPHERE_KINDS for fl in fields) else None
    if out is not None:
        _out_view(out, (L, D, H, W), "(L, D, H, W)")
    hip._dev(table, out)
    if out is None:
        out = torch.empty(L, D, H, W, device=t.device, dtype=torch.float32)
    common = dict(outer_stride=0, lead_stride=lead_stride, channel_stride=channel_stride, n_outer=1, L=L, C=C, out_outer_stride=0,
                  out_lead_stride=out.stride(0), out_channel_stride=out.stride(1), slot=None if slots is None else _upload_slots(slots, t.device))
    _launch_runs(fields, t, out, 1, common, H, W, None if rows is None else _device_row_tables(rows[0], rows[1], W, t.device))
    return out


def field_scales(fields: Sequence[Derived], std) -> List[float]:
    """what an energy-score group divides each field by: its `scale`, by default sqrt(sum of std[c]^2 over its source channels) (float64);
    for `vorticity` / `divergence` that over `SPHERE_SCALE_LENGTH_M`, a wind difference of one standard deviation over 100 km - this
    project's convention, not a published one"""
    s = [float(v) for v in torch.as_tensor(std).reshape(-1).tolist()]

    def default(f):
        root = math.sqrt(sum(s[c] ** 2 for c in f.channels))
        return root / SPHERE_SCALE_LENGTH_M if f.kind in SPHERE_KINDS else root

    return [float(f.scale) if f.scale is not None else default(f) for f in fields]


def extended_scales(fields: Sequence[Derived], std) -> torch.Tensor:
    """`std` (C,) followed by the fields' energy scales: the default `energy_scales` of the extended channels, float64 on the host (what
    `inverse_scale2` computes in)"""
    s = torch.as_tensor(std).detach().cpu().to(torch.float64).reshape(-1)
    return torch.cat([s, torch.tensor(field_scales(fields, s), dtype=torch.float64)])


def parse_derived(entries: Sequence[Sequence[str]], names: Sequence[str]) -> List[Derived]:
    """`--derive NAME KIND CHANNEL [CHANNEL ...]` entries -> the `Derived` list; CHANNEL is a name of `names` (the decoded channels) or
    an index into them, resolved as `--event` resolves it"""
    from .products import resolve_channels

    if len(entries) > MAX_DERIVED:
        raise ValueError(f"--derive: {len(entries)} fields, at most {MAX_DERIVED} are served")
    fields: List[Derived] = []
    for entry in entries:
        if len(entry) < 3:
            raise ValueError(f"--derive {' '.join(entry)}: a name, a kind and the channels are needed")
        name, kind, chans = str(entry[0]), str(entry[1]), [str(c) for c in entry[2:]]
        if kind not in KINDS:
            raise ValueError(f"--derive {name} {kind}: the kind is one of {sorted(KINDS)}")
        if len(chans) != KIND_CHANNELS[kind]:
            raise ValueError(f"--derive {name} {kind}: {kind} reads {KIND_CHANNELS[kind]} channels, got {len(chans)}")
        if name in names or name.lstrip("-").isdigit():
            raise ValueError(f"--derive {name}: the name must differ from the decoded channels' names and be no number")
        if any(name == f.name for f in fields):
            raise ValueError(f"--derive {name}: given twice")
        taken = [c for c in chans if any(c == f.name for f in fields)]
        if taken:
            raise ValueError(f"--derive {name}: {taken[0]} is a derived field; a derived field reads decoded channels only")
        fields.append(Derived(name, kind, tuple(resolve_channels(chans, names))))
    return fields


def derived_metadata(fields: Sequence[Derived], names: Sequence[str], std=None) -> List[dict]:
    """what derived.json and products.json say about each field: name, kind, source channel indices and names, `index` - its channel
    in the extended numbering (decoded channels first) - and `scale` (None where neither the field nor `std` gives one)"""
    scales = field_scales(fields, std) if std is not None else [None if f.scale is None else float(f.scale) for f in fields]
    return [dict(name=f.name, kind=f.kind, channels=list(f.channels), channel_names=[names[c] for c in f.channels], index=len(names) + k,
                 scale=s) for k, (f, s) in enumerate(zip(fields, scales))]


def check_scoring_fields(fields: Sequence[Derived], C: int, sst_channel: int, events=()) -> None:
    """what the scoring driver refuses before anything is decoded: a field that reads the SST channel (one channel only is averaged
    with nanmean: its NaN land points would make every score of the field NaN), and an anomaly event on a `speed` / `shear` field (its
    climatology planes are NaN: the climatology of the field is not the field of the climatology)"""
    for f in fields:
        if sst_channel in f.channels:
            raise ValueError(f"derived field {f.name!r} reads channel {sst_channel}, the SST channel: NaN over land, and only that channel is averaged with nanmean")
    for ev in events or ():
        ev = Event(*ev)
        k = int(ev.channel) - C
        if ev.anomaly and 0 <= k < len(fields) and fields[k].kind in NONLINEAR_KINDS:
            raise ValueError(f"an anomaly event on the {fields[k].kind} field {fields[k].name!r}: a nonlinear field has no climatology here")


class ExtendedBatch:
    """The decode batch, the truth and the climatology with the derived fields as channels C .. C + D - 1, for the drivers: buffers
    allocated at the first batch and reused.  The head of the forecast stays normalised and keeps its bits, the tail is physical:
    `mean` / `std` are extended with 0 / 1, with which the scorers' inverse normalisation is the identity (but for -0.0 -> +0.0)."""

    def __init__(self, derived, mean_d: torch.Tensor, std_d: torch.Tensor):
        self.C = int(mean_d.numel())
        self.fields = _field_list(derived, self.C)
        self.D = len(self.fields)
        self.mean_d, self.std_d = mean_d, std_d
        self.mean = torch.cat([mean_d.reshape(-1), torch.zeros(self.D, device=mean_d.device, dtype=mean_d.dtype)])
        self.std = torch.cat([std_d.reshape(-1), torch.ones(self.D, device=std_d.device, dtype=std_d.dtype)])
        self.y = None
        self._tables = {}

    def buffer(self, per: int, ens: int, H: int, W: int, dev) -> torch.Tensor:
        """the (per, ens, C + D, H, W) decode batch, lead-major; the caller copies decoder outputs into `[:, :, :C]`"""
        if self.y is None:
            self.y = torch.empty(per, ens, self.C + self.D, H, W, device=dev, dtype=torch.float32)
        return self.y

    def derive(self, nl: int) -> torch.Tensor:
        """fills the tail channels of the first `nl` lead times from their head -> that (nl, ens, C + D, H, W) view"""
        y = self.y[:nl]
        derive_forecast(y[:, :, : self.C], self.fields, lead_dim=0, mean=self.mean_d, std=self.std_d, out=y[:, :, self.C :])
        return y

    def table(self, which: str, table: torch.Tensor, slots: Sequence[int], per: int) -> torch.Tensor:
        """-> the (nl, C + D, H, W) table of one batch, entry l = entry slots[l] of `table` (N, C, H, W) followed by its derived fields;
        which == "clim": the planes of `speed` / `shear` fields are NaN"""
        nl, (_, C, H, W) = len(slots), table.shape
        buf = self._tables.get(which)
        if buf is None:
            buf = self._tables[which] = torch.empty(max(per, nl), C + self.D, H, W, device=table.device, dtype=torch.float32)
        t = buf[:nl]
        derive_table(table, slots, self.fields, out=t[:, C:])  # checks the slots on the host
        t[:, :C].copy_(table.index_select(0, _upload_slots(list(slots), table.device)))
        if which == "clim":
            for k, f in enumerate(self.fields):
                if f.kind in NONLINEAR_KINDS:
                    t[:, C + k].fill_(float("nan"))
        return t
