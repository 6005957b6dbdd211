"""ladcast/metric/utils.py with the reference's names and signatures, and the one entry to the fused scores kernel
(`ldc_recon_scores`) that `LpLoss`, `MSELoss` and the reconstruction evaluation share.  Device tensors only: no CPU path."""
from typing import Optional, Tuple

import torch

from .. import hip


def remove_channel(tensor: torch.Tensor, channel_idx: int) -> torch.Tensor:
    """metric/utils.py:6-17: (B, C, ...) without channel `channel_idx`"""
    return torch.cat([tensor[:, :channel_idx, ...], tensor[:, channel_idx + 1 :, ...]], dim=1)


def process_tensor_for_loss(reconstructed: torch.Tensor, target: torch.Tensor, nan_mask: torch.Tensor, sst_chanel_idx: int,
                            sur_pressure_channel_idx_to_remove: Optional[int] = None, nan_mask_val: int = -2.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """metric/utils.py:20-63: both tensors with `nan_mask_val` where nan_mask (B, H, W) is set in the SST channel.  This returns the two
    masked tensors, as the reference does, for callers that want them; the evaluation never makes them - `recon_scores` takes the mask
    itself and applies it while it reads."""
    hip._dev(reconstructed, target, nan_mask)
    if sur_pressure_channel_idx_to_remove is not None:
        assert sst_chanel_idx < sur_pressure_channel_idx_to_remove, (
            "The sea surface temperature channel index must be less than the surface pressure channel index")
        target = remove_channel(target, sur_pressure_channel_idx_to_remove)
    m = nan_mask.to(torch.bool)
    out = []
    for t in (reconstructed, target):
        t = t.clone()
        t[:, sst_chanel_idx].masked_fill_(m, nan_mask_val)
        out.append(t)
    return out[0], out[1]


def _lat_weight(weight, H, device):
    """weight None or broadcastable from (1, 1, H, 1) -> (H,) fp32 device vector"""
    if weight is None:
        return torch.ones(H, device=device, dtype=torch.float32)
    hip._dev(weight)
    shape = tuple(weight.shape)
    lead = shape[:-2] if len(shape) >= 2 else ()
    if weight.dtype != torch.float32 or len(shape) > 4 or len(shape) < 2 or shape[-1] != 1 or shape[-2] != H or any(s != 1 for s in lead):
        raise NotImplementedError(f"the device path takes a fp32 weight broadcastable from (1, 1, H, 1) = one value per latitude row; got "
                                  f"{weight.dtype} {shape}")
    return weight.reshape(H).contiguous()


def recon_scores(pred: torch.Tensor, target: torch.Tensor, static: Optional[torch.Tensor] = None, nan_mask: Optional[torch.Tensor] = None,
                 sst_channel: int = -1, lat_weight: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None,
                 std: Optional[torch.Tensor] = None, want_abs: bool = False):
    """One pass over pred (B, Cp, H, W) and target (B, C, H, W) [+ static (1 or B, S, H, W), Cp = C + S]: ->
    (rel (B, Cp), abs (B, Cp) | None, lw_mse (Cp,)) as `ldc_recon_scores` defines them (mean / std None: 0 / 1)."""
    hip._dev(pred, target, static, nan_mask, lat_weight, mean, std)
    if pred.dim() != 4 or target.dim() != 4:
        raise NotImplementedError(f"the device path scores (B, C, H, W) fields; got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise NotImplementedError(f"the device path is fp32; got {pred.dtype} and {target.dtype}")
    B, Cp, H, W = pred.shape
    C = target.shape[1]
    S = 0 if static is None else static.shape[1]
    if tuple(target.shape) != (B, C, H, W) or C + S != Cp:
        raise ValueError(f"pred {tuple(pred.shape)} does not match target {tuple(target.shape)} + {S} static channels")
    sbs = 0
    if static is not None:
        if static.dim() != 4 or static.dtype != torch.float32 or tuple(static.shape[2:]) != (H, W) or static.shape[0] not in (1, B):
            raise ValueError(f"static must be fp32 (1 or {B}, S, {H}, {W}); got {static.dtype} {tuple(static.shape)}")
        static = static.contiguous()
        sbs = 0 if static.shape[0] == 1 else S * H * W
    dev = pred.device
    if nan_mask is not None:
        if tuple(nan_mask.shape) != (B, H, W):
            raise ValueError(f"nan_mask must be ({B}, {H}, {W}); got {tuple(nan_mask.shape)}")
        nan_mask = (nan_mask.view(torch.uint8) if nan_mask.dtype == torch.bool else nan_mask).contiguous()
        if nan_mask.dtype != torch.uint8:
            raise ValueError("nan_mask must be bool or uint8")
    w = _lat_weight(lat_weight, H, dev) if (lat_weight is None or lat_weight.dim() != 1) else lat_weight.to(torch.float32).contiguous()
    if w.numel() != H:
        raise ValueError("lat_weight must have one value per latitude row")
    mean = torch.zeros(Cp, device=dev) if mean is None else mean.to(torch.float32).reshape(-1).contiguous()
    std = torch.ones(Cp, device=dev) if std is None else std.to(torch.float32).reshape(-1).contiguous()
    if mean.numel() != Cp or std.numel() != Cp:
        raise ValueError(f"mean / std must hold {Cp} values (fields + static channels)")
    rel = torch.empty(B, Cp, device=dev, dtype=torch.float32)
    lw = torch.empty(Cp, device=dev, dtype=torch.float32)
    absn = torch.empty(B, Cp, device=dev, dtype=torch.float32) if want_abs else None
    hip.recon_scores(pred.contiguous(), target.contiguous(), static, nan_mask, w, mean, std, rel, lw, B=B, C=C, S=S, H=H, W=W,
                     static_batch_stride=sbs, sst_channel=sst_channel, abs_norm=absn)
    return rel, absn, lw
