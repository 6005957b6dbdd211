"""Energy score of a decoded ensemble (`ldc_rollout_energy`, csrc/energy.hip; not in the reference): the
multivariate generalisation of the CRPS (Gneiting & Raftery 2007),

    ES = mean_i ||x_i - t|| - 1/2 mean_{i,j} ||x_i - x_j||,      ||.|| the latitude-weighted RMS norm of a whole field,

per (channel, lead time) and per group of channels, each channel of a group divided by its scale.  Every pointwise score is blind to
what this one sees: shuffling the members of each grid point independently leaves every per-point CRPS as it was and changes ES.

    groups = [EnergyGroup("z500_t850", (7, 23))]
    out = rollout_energy(forecast, truth, lat_weight, groups=groups, scales=std)     # (C, L) and (G, L) float64 device tensors

The score is not additive over initial times: the pooled value is the mean of the per-initial-time values."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Sequence

import torch

from .. import hip
from .utils import _Buf, _empty, _launch_args, _out_buffers, _prologue

MAX_ENERGY_MEMBERS, MAX_ENERGY_GROUPS = hip.ENERGY_MAX_MEMBERS, hip.ENERGY_MAX_GROUPS
ENERGY_NAMES = ("energy_score", "energy_score_fair", "energy_skill", "energy_spread", "energy_weight")  # the planes of `energy`, in order
ENERGY_GROUP_NAMES = tuple(n.replace("energy_", "energy_group_") for n in ENERGY_NAMES)  # the planes of `energy_group`, in order


class EnergyGroup(NamedTuple):
    """a group of channels scored together as one multivariate field: `channels` are indices into the forecast's channels"""

    name: str
    channels: tuple


def _group_list(groups, C: int):
    """`groups` (EnergyGroup, or (name, channels) pairs) -> a list of EnergyGroup with int channel tuples; every mistake is a ValueError"""
    out = []
    for gr in groups or ():
        try:
            gr = EnergyGroup(*gr)
            chans = tuple(gr.channels.tolist() if isinstance(gr.channels, torch.Tensor) else gr.channels)
        except TypeError:
            raise ValueError(f"a group is EnergyGroup(name, channels), got {gr!r}") from None
        if not chans:
            raise ValueError(f"group {gr.name!r} holds no channel")
        if any(isinstance(c, bool) or not isinstance(c, int) and int(c) != c for c in chans):
            raise ValueError(f"group {gr.name!r}: channels are indices, got {chans}")
        chans = tuple(int(c) for c in chans)
        if any(not 0 <= c < C for c in chans):
            raise ValueError(f"group {gr.name!r}: channels {chans} are not all among the forecast's {C}")
        if len(set(chans)) != len(chans):
            raise ValueError(f"group {gr.name!r}: a channel is named twice in {chans}")
        out.append(EnergyGroup(str(gr.name), chans))
    if len(out) > MAX_ENERGY_GROUPS:
        raise ValueError(f"{len(out)} groups: ldc_rollout_energy takes at most {MAX_ENERGY_GROUPS} per call")
    names = [g.name for g in out]
    if len(set(names)) != len(names):
        raise ValueError(f"group names must differ, got {names}")
    return out


def group_words(groups: Sequence[EnergyGroup], C: int) -> torch.Tensor:
    """-> int32 host tensor (C,): bit g of word c says that channel c belongs to groups[g]"""
    words = [0] * C
    for g, gr in enumerate(groups):
        for c in gr.channels:
            words[c] |= 1 << g
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


def inverse_scale2(scales, C: int) -> torch.Tensor:
    """`scales` (C,) positive and finite -> float64 host tensor 1 / scale^2, each formed as 1 / (s * s) in float64"""
    s = torch.as_tensor(scales).detach().cpu().to(torch.float64).reshape(-1)
    if s.numel() != C:
        raise ValueError(f"scales must hold one value per channel ({C}), got {s.numel()}")
    if not bool((torch.isfinite(s) & (s > 0)).all()):
        raise ValueError("scales must be positive and finite")
    return 1.0 / (s * s)


class EnergyDict(dict):
    """{energy_score, energy_score_fair, energy_skill, energy_spread, energy_weight: (C, L_total) float64; energy_n_invalid: (C, L_total)
    int32; with groups energy_group_score, ... : (G, L_total) float64; when asked energy_dist2: (C, L_total, M + 1, M + 1) float64} over
    the device buffers `ldc_rollout_energy` fills"""

    _spec = (_Buf(lambda Lt, M, C, G, dist2: (hip.ENERGY_PLANES, C, Lt), torch.float64, float("nan"), 2), _Buf(lambda Lt, M, C, G, dist2: (C, Lt), torch.int32, 0, 1),
             _Buf(lambda Lt, M, C, G, dist2: (hip.ENERGY_PLANES, G, Lt) if G else None, torch.float64, float("nan"), 2, "none"),
             _Buf(lambda Lt, M, C, G, dist2: (C, Lt, M + 1, M + 1) if dist2 else None, torch.float64, float("nan"), 1, "none"))

    def __init__(self, energy, n_invalid, energy_group=None, dist2=None):
        super().__init__({k: energy[i] for i, k in enumerate(ENERGY_NAMES)})
        self["energy_n_invalid"] = n_invalid
        if energy_group is not None:
            self.update({k: energy_group[i] for i, k in enumerate(ENERGY_GROUP_NAMES)})
        if dist2 is not None:
            self["energy_dist2"] = dist2
        self._buffers = (energy, n_invalid, energy_group, dist2)


def empty_energy(M: int, C: int, G: int, L_total: int, device, dist2: bool = False) -> EnergyDict:
    """the result of `rollout_energy` before any column is written: scores NaN, weights NaN, `energy_n_invalid` zero, `energy_dist2` NaN"""
    return EnergyDict(*_empty(EnergyDict._spec, L_total, device, M=M, C=C, G=G, dist2=dist2))


@torch.no_grad()
def rollout_energy(forecast: torch.Tensor, truth: torch.Tensor, lat_weight: torch.Tensor, *, groups: Optional[Sequence] = None, scales=None,
                   return_dist2: bool = False, lead_dim: int = 2, mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None,
                   target_std: float = 1.0, truth_slot=None, out: Optional[Dict[str, torch.Tensor]] = None,
                   l_off: int = 0) -> Dict[str, torch.Tensor]:
    """The energy score of every (channel, lead time) and of every group of channels in one call (`ldc_rollout_energy`; not in the
    reference).  Per (channel, lead time), with the M members y_0 .. y_{M-1} and the truth y_M as whole fields: a point is valid when no
    member and not the truth is NaN (the others are left out and counted in `energy_n_invalid`; +-inf are ordinary values);
        D2[a][b] = sum over valid points of w (y_a - y_b)^2      the difference and its square in fp32, the sum in fp64
        Wv = sum over valid points of w,    norm(a, b) = sqrt(D2[a][b] / Wv)
        energy_skill = mean_i norm(i, M),   energy_spread = sum_{i != j} norm(i, j) / M^2
        energy_score = skill - spread / 2,  energy_score_fair = skill - sum_{i != j} norm(i, j) / (2 M (M - 1))   (M == 1: the skill)
    all NaN without a valid point; `energy_weight` = Wv.  The score is in the channel's unit; for a single point
    `energy_score_fair` is that point's CRPS.  1 <= M <= 256.

    `groups`: a sequence of `EnergyGroup(name, channels)` (at most 32, may overlap), with `scales` (C,) positive and finite: group g has
    D2_g = sum over its channels, ascending, of D2_c / scale_c^2 and Wv_g = sum of Wv_c, and the same five quantities as
    `energy_group_score`, ... (G, L_total).  A channel with fewer valid points (SST over land) contributes fewer coordinates.
    `return_dist2`: also `energy_dist2` (C, L_total, M + 1, M + 1), the matrix D2 (symmetric, zero diagonal; index M is the truth).

    forecast, `lead_dim`, `mean` / `std` / `target_std`, truth / `truth_slot`, `out` / `l_off`: as `rollout_regional`.  Returns an
    `EnergyDict` of float64 device tensors with L_total = l_off + L columns (unwritten columns: NaN), or fills columns
    l_off .. l_off + L - 1 of `out`, the dict an earlier call (or `empty_energy`) returned for the same M, C, groups and `return_dist2`."""
    r = _prologue(forecast, lead_dim, mean, std, target_std, truth=(truth, truth_slot), weight=(lat_weight, "lat_weight"),
                  members=("ldc_rollout_energy", MAX_ENERGY_MEMBERS))
    C, dev = r.C, r.f.device
    grs = _group_list(groups, C)
    G = len(grs)
    if G and scales is None:
        raise ValueError("groups need scales: one positive value per channel")
    inv_s2 = None if scales is None else inverse_scale2(scales, C)
    if l_off < 0:
        raise ValueError("l_off must not be negative")
    bufs = _out_buffers(EnergyDict._spec, out, r, l_off, M=r.M, C=C, G=G, dist2=return_dist2, msg=(
        "out must be the dict an earlier rollout_energy call (or empty_energy) returned for the same ensemble size, "
        "channels, number of groups and return_dist2, with room for columns l_off .. l_off + L - 1"))
    hip._dev(forecast, truth, lat_weight, mean, std)
    bufs = bufs or _empty(EnergyDict._spec, l_off + r.L, dev, M=r.M, C=C, G=G, dist2=return_dist2)
    args, kw = _launch_args(r, bufs[0].shape[2], l_off)
    words = hip.upload_nonblocking(group_words(grs, C), dev) if G else None
    inv_d = hip.upload_nonblocking(inv_s2.contiguous(), dev) if G else None
    hip.rollout_energy(*args, bufs[0], bufs[1], group_mask=words, inv_scale2=inv_d, G=G, energy_group=bufs[2], dist2=bufs[3], **kw)
    return EnergyDict(*bufs)
