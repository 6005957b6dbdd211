"""ladcast/metric/loss.py with the reference's names and signatures, on the device.  The norms and means over the grid come from
the fused kernel `ldc_recon_scores` (one pass over both tensors); what is left is arithmetic on (B, C) values.  Served: what the
evaluation uses - d = 2, p = 2 on (B, C, H, W) fp32 device tensors, weight None or broadcastable from (1, 1, H, 1).  Anything else
raises NotImplementedError; there is no CPU path."""
from typing import Optional

import torch

from .utils import recon_scores


def _per_var(diff, channels, num_atm_vars, num_levels, ref):
    """get_loss_per_var's grouping of a (B, C) / (1, C) table: one mean per atmospheric variable (its levels), one per other channel"""
    cutoff = num_atm_vars * num_levels
    batch_mean = torch.empty(channels - cutoff + num_atm_vars, device=ref.device, dtype=ref.dtype)
    for i in range(num_atm_vars):
        batch_mean[i] = diff[:, i * num_levels : (i + 1) * num_levels].mean()
    for i in range(0, channels - cutoff):
        batch_mean[i + num_atm_vars] = diff[:, i].mean()  # (the reference indexes from 0 here, not from the cutoff: kept)
    return batch_mean


class LpLoss(object):
    """metric/loss.py:7-157: relative (default) / absolute Lp loss over the last d dimensions"""

    def __init__(self, d=1, p=2, reduce_dims=0, reductions="sum"):
        super().__init__()
        self.d = d
        self.p = p
        if isinstance(reduce_dims, int):
            self.reduce_dims = [reduce_dims]
        else:
            self.reduce_dims = reduce_dims
        if self.reduce_dims is not None:
            if isinstance(reductions, str):
                assert reductions == "sum" or reductions == "mean"
                self.reductions = [reductions] * len(self.reduce_dims)
            else:
                for j in range(len(reductions)):
                    assert reductions[j] == "sum" or reductions[j] == "mean"
                self.reductions = reductions

    def reduce_all(self, x):
        for j in range(len(self.reduce_dims)):
            if self.reductions[j] == "sum":
                x = torch.sum(x, dim=self.reduce_dims[j], keepdim=True)
            else:
                x = torch.mean(x, dim=self.reduce_dims[j], keepdim=True)
        return x

    def _norms(self, x, y, weight, want_abs):
        if self.d != 2 or self.p != 2:
            raise NotImplementedError(f"the device path serves d = 2, p = 2 (the reconstruction evaluation); got d = {self.d}, p = {self.p}")
        rel, absn, _ = recon_scores(x, y, lat_weight=weight, want_abs=want_abs)
        return rel, absn

    def abs(self, x, y, weight: Optional[torch.Tensor] = None):
        diff = self._norms(x, y, weight, True)[1]
        if self.reduce_dims is not None:
            diff = self.reduce_all(diff).squeeze()
        return diff

    def rel(self, x, y, weight: Optional[torch.Tensor] = None):
        diff = self._norms(x, y, weight, False)[0]  # (B, C)
        if self.reduce_dims is not None:
            diff = self.reduce_all(diff).squeeze()
        return diff

    def __call__(self, y_pred, y, weight: Optional[torch.Tensor] = None):
        return self.rel(y_pred, y, weight=weight)

    @torch.no_grad()
    def get_loss_per_var(self, y_pred, y, num_atm_vars, num_levels=13, weight: Optional[torch.Tensor] = None):
        """Assuming input of order [atm_vars, sur_vars] -> (num_atm_vars + num_sur_vars,)"""
        diff = self._norms(y_pred, y, weight, False)[0]
        return _per_var(diff, y_pred.shape[1], num_atm_vars, num_levels, y_pred)


class MSELoss:
    """metric/loss.py:160-196"""

    def __init__(self, reduction="mean"):
        self.reduction = reduction

    def __call__(self, y_pred, y):
        if self.reduction not in ("mean", "sum"):
            raise NotImplementedError(f"the device path reduces to one value ('mean' or 'sum'); got reduction = {self.reduction!r}")
        lw = recon_scores(y_pred, y)[2]  # per-channel mean of (y_pred - y)^2 over (b, h, w): planes of equal size
        return lw.mean() if self.reduction == "mean" else lw.sum() * (y_pred.numel() // y_pred.shape[1])

    @torch.no_grad()
    def get_loss_per_var(self, y_pred, y, num_atm_vars, num_levels=13, weight: Optional[torch.Tensor] = None):
        """Assuming input of order [atm_vars, sur_vars] -> (num_atm_vars + num_sur_vars,)"""
        lw = recon_scores(y_pred, y, lat_weight=weight)[2]  # mean of weight * (y_pred - y)^2 per channel
        return _per_var(lw[None], y_pred.shape[1], num_atm_vars, num_levels, y_pred)
