"""The three scores of the reference's validation hook (ladcast/train_AR.py:281-312) restated in torch fp32; pinned to the reference's own
code by tests/test_validation_cpu.py through tests/golden/validation_ref.npz."""
import torch

from oracle.scoring import get_crps

NAMES = ("ens_mse", "single_mse", "crps")


def validation_scores(decoded: torch.Tensor, ref: torch.Tensor, lat_weight: torch.Tensor):
    """decoded (ens, C, T, H, W), ref (C, T, H, W), lat_weight (H,) -> {name: (C, T)}; plain means, so a NaN propagates"""
    w = lat_weight.to(decoded.dtype)
    single = ((decoded - ref.unsqueeze(0)) ** 2) * w.view(1, 1, 1, -1, 1)
    ens = ((decoded.mean(dim=0) - ref) ** 2) * w.view(1, 1, -1, 1)
    crps = get_crps(decoded, ref, ensemble_dim=0) * w.view(1, 1, -1, 1)
    return {"ens_mse": ens.mean(dim=(2, 3)), "single_mse": single.mean(dim=(0, 3, 4)), "crps": crps.mean(dim=(2, 3))}
