"""Bulk encode of raw fields into the latent store, with the latent statistics taken on the way (reference:
ladcast/preprocecss/encode_data.py, `encode_latents_and_save_zarr_hf_dataset` and `main`; the latent statistics JSON is shipped by the
reference without the code that made it).

    python -m ladcast_amd.preprocess.encode_data --frames era5_1979.npy era5_1980.npy ... --normalization_json ERA5_normal.json \\
        --encdec_model DCAE/ --lsm_path lsm.npy --orography_path orography.npy --output latents.npy --latent_normal_json latent_normal.json

Per batch of ``--batch_size`` raw frames (N, C_in, H_in, W) fp32: upload, `preprocess_batch` (south-pole crop, the surface pressure
dropped, normalise, SST NaN -> -2: one kernel), `vae.encode` with the z-scored static planes, `FieldMoments.update` on the latents where
they are, and a copy into the NaN-prefilled (N, latent_channels, h, w) host array that ``--output`` saves.  The reference encodes one
frame per call; the batched encoder gives the same latents (tests/test_gpu_dcae.py).  ``--latent_normal_json`` receives
``{"mean": [...], "std": [...]}`` over all frames and latent pixels (population std).  The static planes are .npy or torch .pt files:
the land-sea mask (H_in, W) and the orography fields (4, H_in, W), as the reference's static/ folder holds them.  zarr, xarray and
multi-rank splitting are out of scope.
"""
from __future__ import annotations

import argparse
import json
import os
import warnings
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from .. import hip
from .compute_mean_std_era5 import channel_count, frame_batches, load_names, open_frames
from .stats import FieldMoments, latent_normal_dict


@torch.no_grad()
def encode_frames(vae, batches: Iterable[torch.Tensor], total_frames: int, mean: torch.Tensor, std: torch.Tensor,
                  static_conditioning_tensor: Optional[torch.Tensor] = None, sst_channel_idx: Optional[int] = 82,
                  crop_south_pole: bool = True, incl_sur_pressure: bool = False) -> Tuple[np.ndarray, Optional[FieldMoments]]:
    """batches: raw fp32 frames (B, C_in, H_in, W), `total_frames` in all; mean / std: one value per kept channel;
    static_conditioning_tensor: (S, H, W), already cropped and z-scored (`build_static_conditioning`).
    -> (latents (N, latent_channels, h, w) fp32 host array, NaN where no frame arrived; the latents' `FieldMoments`, None without frames)"""
    from ..evaluate.evaluate_encdec_model import preprocess_batch

    dev = vae.device
    mean_d, std_d = mean.to(dev, torch.float32).reshape(-1), std.to(dev, torch.float32).reshape(-1)
    static = None if static_conditioning_tensor is None else static_conditioning_tensor.to(dev, torch.float32).unsqueeze(0).contiguous()
    out, fm, i0 = None, None, 0
    for raw in batches:
        raw = hip.upload_nonblocking(torch.as_tensor(raw), dev)
        x = preprocess_batch(raw, mean_d, std_d, crop_south_pole=crop_south_pole, sst_channel_idx=sst_channel_idx, incl_sur_pressure=incl_sur_pressure)
        if sst_channel_idx is not None:
            x = x[0]
        latent = vae.encode(x, static_conditioning_tensor=static).latent
        if out is None:
            out = np.full((total_frames,) + tuple(latent.shape[1:]), np.nan, dtype=np.float32)
            fm = FieldMoments(latent.shape[1], dev)
        if i0 + latent.shape[0] > total_frames:
            raise ValueError(f"more than the announced {total_frames} frames arrived")
        fm.update(latent)
        out[i0 : i0 + latent.shape[0]] = latent.detach().cpu().numpy()
        i0 += latent.shape[0]
    if out is None:
        out = np.empty((0,), dtype=np.float32)
    return out, fm


def _load_planes(path: str) -> torch.Tensor:
    if path.endswith(".npy"):
        return torch.from_numpy(np.load(path).astype(np.float32))
    return torch.load(path, weights_only=True).float()


def main(argv=None):
    ap = argparse.ArgumentParser(description="Encode raw .npy frames into the latent store and write the latent statistics")
    ap.add_argument("--frames", nargs="+", required=True, metavar="PATH", help=".npy files of raw fp32 frames (N, C_in, H_in, W)")
    ap.add_argument("--normalization_json", required=True, help="per-variable mean / std JSON (compute_mean_std_era5)")
    ap.add_argument("--variable_names_json", default=None, help="JSON with channel_names, pressure_levels, num_atm_vars of the ENCODED channels")
    ap.add_argument("--encdec_model", required=True, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--lsm_path", default=None, help="land-sea mask (H_in, W), .npy or .pt")
    ap.add_argument("--orography_path", default=None, help="orography fields (4, H_in, W), .npy or .pt")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--sst_channel_idx", type=int, default=82, help="channel whose NaNs become -2 after normalisation; -1: none")
    ap.add_argument("--keep_south_pole", action="store_true", help="do not crop the first latitude row")
    ap.add_argument("--incl_sur_pressure", action="store_true", help="keep the last channel of the frames")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    ap.add_argument("--output", required=True, help="latents .npy (N, latent_channels, h, w)")
    ap.add_argument("--latent_normal_json", required=True, help="the latent statistics JSON to write")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    names, levels, n_atm = load_names(args.variable_names_json)
    C = channel_count(names, levels, n_atm)
    arrs = open_frames(args.frames, C + (0 if args.incl_sur_pressure else 1))
    total = sum(a.shape[0] for a in arrs)
    if total == 0:
        raise SystemExit("--frames hold no frame")

    from ..evaluate.pred_rollout import build_static_conditioning
    from ..evaluate.track import mean_std_from_json
    from ..models import AutoencoderDC

    with open(args.normalization_json) as f:
        mean_t, std_t = mean_std_from_json(json.load(f), names)
    if mean_t.numel() != C:
        raise SystemExit(f"{args.normalization_json}: {mean_t.numel()} channel statistics for {C} channels")
    if os.path.isdir(args.encdec_model) and any(n.endswith((".safetensors", ".bin")) for n in os.listdir(args.encdec_model)):
        model = AutoencoderDC.from_pretrained(args.encdec_model)
    else:
        cfg_path = os.path.join(args.encdec_model, "config.json") if os.path.isdir(args.encdec_model) else args.encdec_model
        with open(cfg_path) as f:
            model = AutoencoderDC.from_config(json.load(f))
        warnings.warn(f"{args.encdec_model}: no weights found, the DC-AE keeps its initial weights")
    model = model.to("cuda").eval()
    model.set_gemm_precision(args.gemm_precision)
    crop = not args.keep_south_pole
    static = build_static_conditioning(None if args.lsm_path is None else _load_planes(args.lsm_path),
                                       None if args.orography_path is None else _load_planes(args.orography_path), crop_pole=crop)

    latents, fm = encode_frames(model, frame_batches(arrs, args.batch_size), total, mean_t, std_t, static,
                                sst_channel_idx=None if args.sst_channel_idx < 0 else args.sst_channel_idx, crop_south_pole=crop,
                                incl_sur_pressure=args.incl_sur_pressure)
    np.save(args.output, latents)
    lat_mean, lat_std = fm.mean_std()
    with open(args.latent_normal_json, "w") as f:
        json.dump(latent_normal_dict(lat_mean, lat_std), f, indent=4)
    print(f"encoded {total} frames into {latents.shape}: saved to {args.output}; latent mean / std to {args.latent_normal_json}")
    return latents


if __name__ == "__main__":
    main()
