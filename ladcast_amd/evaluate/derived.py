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
only, never another derived field."""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import hip
from .utils import Event, _channel_affine, _forecast_view, _plane_table, _upload_slots

KINDS = {"speed": hip.DERIVE_SPEED, "diff": hip.DERIVE_DIFF, "shear": hip.DERIVE_SHEAR}
KIND_CHANNELS = {k: hip.DERIVE_INPUTS[v] for k, v in KINDS.items()}  # speed (a, b): 2, diff (a, b): 2, shear (a, b, c, d): 4
NONLINEAR_KINDS = ("speed", "shear")  # the climatology of the field is not the field of the climatology
MAX_DERIVED = hip.DERIVE_MAX_FIELDS


class Derived(NamedTuple):
    """a derived field: `speed` sqrt(a^2 + b^2), `diff` a - b or `shear` sqrt((a - c)^2 + (b - d)^2) of the DECODED channels
    `channels` = (a, b[, c, d]); `scale`: what an energy-score group divides this channel by (default: sqrt(sum of std[c]^2 over its
    source channels), the standard deviation of a difference of independent components)"""

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


def _desc(fields: Sequence[Derived]):
    return hip.derive_desc([(KINDS[f.kind], f.channels) for f in fields])


def _out_view(out, shape, what: str):
    if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.stride(-1) != 1 \
            or out.stride(-2) != shape[-1]:
        raise ValueError(f"out must be an fp32 {what} = {tuple(shape)} tensor (any view with a contiguous (H, W) plane)")


@torch.no_grad()
def derive_forecast(forecast: torch.Tensor, derived, *, lead_dim: int = 2, mean: Optional[torch.Tensor] = None,
                    std: Optional[torch.Tensor] = None, target_std: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The D derived fields of a forecast in physical units, in one `ldc_derive_fields` call: -> (ens, D, L, H, W), or with `lead_dim=0`
    (L, ens, D, H, W).  forecast, `lead_dim`, `mean` / `std` / `target_std`: as `rollout_scores` - an input holds the bits the scorers
    load for that channel; mean None: the forecast is physical already.  `out`: a tensor of the result's shape to write to, any view
    with a contiguous (H, W) plane, e.g. the tail channels of an extended (L, ens, C + D, H, W) tensor whose head is the forecast."""
    f, M, C, L, H, W = _forecast_view(forecast, lead_dim)
    fields = _field_list(derived, C)
    desc, D = _desc(fields), len(fields)
    mn, sd = _channel_affine(mean, std, C, f.device)
    shape = (M, D, L, H, W) if lead_dim == 2 else (L, M, D, H, W)
    if out is not None:
        _out_view(out, shape, "(ens, D, L, H, W)" if lead_dim == 2 else "(L, ens, D, H, W)")
    hip._dev(forecast, mean, std, out)
    if out is None:
        out = torch.empty(shape, device=f.device, dtype=torch.float32)
    o = out if lead_dim == 2 else out.permute(1, 2, 0, 3, 4)
    hip.derive_fields(f, o, desc, outer_stride=f.stride(0), lead_stride=f.stride(2), channel_stride=f.stride(1), n_outer=M, L=L, C=C, HW=H * W,
                      out_outer_stride=o.stride(0), out_lead_stride=o.stride(2), out_channel_stride=o.stride(1), mean=mn, std=sd,
                      target_std=target_std)
    return out


@torch.no_grad()
def derive_table(table: torch.Tensor, slots, derived, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The D derived fields of a truth / climatology table, which is physical and never transformed: -> (L, D, H, W).  With `slots` (one
    host int per lead time) `table` is (N, C, H, W) and lead l reads entry slots[l]; with slots None it is a (C, L, H, W) tensor.
    Slots are checked here, on the host.  `out`: as `derive_forecast`, of shape (L, D, H, W)."""
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
    desc, D = _desc(fields), len(fields)
    t, lead_stride, channel_stride, _ = _plane_table(table, slots, C, L, H, W, "table")
    if out is not None:
        _out_view(out, (L, D, H, W), "(L, D, H, W)")
    hip._dev(table, out)
    if out is None:
        out = torch.empty(L, D, H, W, device=t.device, dtype=torch.float32)
    hip.derive_fields(t, out, desc, outer_stride=0, lead_stride=lead_stride, channel_stride=channel_stride, n_outer=1, L=L, C=C, HW=H * W,
                      out_outer_stride=0, out_lead_stride=out.stride(0), out_channel_stride=out.stride(1),
                      slot=None if slots is None else _upload_slots(slots, t.device))
    return out


def field_scales(fields: Sequence[Derived], std) -> List[float]:
    """what an energy-score group divides each field by: its `scale`, by default sqrt(sum of std[c]^2 over its source channels) (float64)"""
    s = [float(v) for v in torch.as_tensor(std).reshape(-1).tolist()]
    return [float(f.scale) if f.scale is not None else math.sqrt(sum(s[c] ** 2 for c in f.channels)) for f in fields]


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
