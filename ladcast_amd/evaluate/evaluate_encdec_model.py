"""DC-AE reconstruction evaluation on the device (reference: ladcast/evaluate/evaluate_encdec_model.py): the relative L2 loss
`val_loss_fn_loss` and one latitude-weighted RMSE per variable and level, in physical units, per year.

Per batch: `ldc_recon_preprocess` (crop, drop the surface pressure, normalise, SST NaN -> -2 + mask; one pass over the raw frames)
-> the autoencoder's forward with `return_static=True` -> `ldc_recon_scores` (mask, relative L2 per (b, c), un-normalise, squared
error, latitude-weighted mean; one pass over the reconstruction and its target, the static channels read where they are).  The
sums over batches stay on the device; the host waits once, at the end of a year.

    python -m ladcast_amd.evaluate.evaluate_encdec_model --frames 2018=f18.npy 2019=f19.npy --normalization_json ERA5_normal.json \\
        --settings_json settings.json --encdec_model DCAE/ [--static_path static.npy] --csv_path dcae_eval.csv

Frames are .npy arrays (N, C_in, H_in, W) of raw fields (xarray / the streaming dataset are out of scope), one file per year; the
settings JSON holds `channel_names` (variables, atmospheric first), `static_names`, and optionally `pressure_levels`,
`num_atm_vars`, `num_sur_vars` (defaults: the reference's 13 levels, 6, 6).  Multi-rank gathering is out of scope.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import warnings
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..metric.utils import recon_scores

PRESSURE_LEVELS = [50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000]
NUM_ATM_VARS = 6
NUM_SUR_VARS = 6


def preprocess_batch(batch: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, crop_south_pole: bool = True,
                     sst_channel_idx: Optional[int] = None, incl_sur_pressure: bool = True):
    """weather_dataset_preprocess_batch (dataloader/weather_dataset.py:203-224) for a raw fp32 device batch (B, C_in, H_in, W): the
    crop and the dropped channel are strides of one kernel launch.  -> (batch (B, C, H, W), nan_mask (B, H, W) bool) or the batch alone
    when sst_channel_idx is None.  mean / std: device vectors with one value per kept channel (any shape)."""
    hip._dev(batch, mean, std)
    if batch.dim() != 4 or batch.dtype != torch.float32:
        raise NotImplementedError(f"the device path preprocesses fp32 (B, C, H, W) batches; got {batch.dtype} {tuple(batch.shape)}")
    if batch.stride(3) != 1:
        batch = batch.contiguous()
    B, C_in, H_in, W = batch.shape
    C, H = C_in - (0 if incl_sur_pressure else 1), H_in - (1 if crop_south_pole else 0)
    mean, std = mean.to(torch.float32).reshape(-1).contiguous(), std.to(torch.float32).reshape(-1).contiguous()
    if C < 1 or H < 1 or mean.numel() != C or std.numel() != C:
        raise ValueError(f"{C} channels x {H} rows are kept of {tuple(batch.shape)}; mean / std hold {mean.numel()} / {std.numel()} values")
    x = batch[:, :, 1:] if crop_south_pole else batch
    out = torch.empty(B, C, H, W, device=batch.device, dtype=torch.float32)
    mask = torch.empty(B, H, W, device=batch.device, dtype=torch.uint8) if sst_channel_idx is not None else None
    hip.recon_preprocess(x, mean, std, out, mask, B=B, C=C, H=H, W=W, batch_stride=x.stride(0), channel_stride=x.stride(1), row_stride=x.stride(2),
                         sst_channel=-1 if sst_channel_idx is None else int(sst_channel_idx))
    return out if mask is None else (out, mask.view(torch.bool))


def normalize_static(static_conditioning_tensor: torch.Tensor):
    """evaluate_encdec_model.py:135-141: (S, H, W) z-scored per plane with the UNBIASED std -> (static, static_mean (S,), static_std (S,))"""
    m = static_conditioning_tensor.mean((1, 2), keepdim=True)
    s = static_conditioning_tensor.std((1, 2), keepdim=True)
    return (static_conditioning_tensor - m) / s, m.flatten(), s.flatten()


@torch.no_grad()
def evaluate_reconstruction(encdec, batches: Iterable[torch.Tensor], mean: torch.Tensor, std: torch.Tensor,
                            static_conditioning_tensor: Optional[torch.Tensor], lat_weight: torch.Tensor, sst_channel_idx: int = 82,
                            crop_south_pole: bool = True, incl_sur_pressure: bool = False) -> Tuple[float, torch.Tensor]:
    """One year of evaluate_encdec_model.py:153-239.  batches: raw fp32 frames (B, C_in, H_in, W), any B per batch (uploaded when on the
    host); mean / std (C,): the fields' statistics; static_conditioning_tensor: raw static planes (S, H, W) on the evaluated grid (already
    cropped), z-scored here, or None; lat_weight (H,).  -> (val_loss_fn_loss, val_lw_rmse (C + S,) on the host)."""
    dev = encdec.device
    mean_d, std_d = mean.to(dev, torch.float32).reshape(-1), std.to(dev, torch.float32).reshape(-1)
    static = None
    proc_mean, proc_std = mean_d, std_d
    if static_conditioning_tensor is not None:
        static, smean, sstd = normalize_static(static_conditioning_tensor.to(dev, torch.float32))
        static = static.unsqueeze(0).contiguous()  # (1, S, H, W): broadcast over the batch by encode() and by the scores kernel
        proc_mean, proc_std = torch.cat([mean_d, smean]), torch.cat([std_d, sstd])
    w = lat_weight.to(dev, torch.float32).reshape(-1).contiguous()
    lw_acc = loss_acc = None
    total = 0
    for raw in batches:
        raw = hip.upload_nonblocking(torch.as_tensor(raw), dev)
        x, mask = preprocess_batch(raw, mean_d, std_d, crop_south_pole=crop_south_pole, sst_channel_idx=sst_channel_idx,
                                   incl_sur_pressure=incl_sur_pressure)
        B = x.shape[0]
        pred = encdec(x, return_static=True, static_conditioning_tensor=static).sample
        rel, _, lw = recon_scores(pred, x, static, mask, sst_channel_idx, w, proc_mean, proc_std)
        loss = rel.mean(dim=0, keepdim=True).mean(dim=1).reshape(())  # LpLoss(reduce_dims=[0, 1], reductions="mean")
        lw_acc = lw * B if lw_acc is None else lw_acc + lw * B
        loss_acc = loss * B if loss_acc is None else loss_acc + loss * B
        total += B
    if total == 0:
        raise ValueError("no batches to evaluate")
    out = torch.cat([(loss_acc / total).reshape(1), torch.sqrt(lw_acc / total)]).cpu()  # the one synchronisation
    return float(out[0]), out[1:]


# ---- CSV (evaluate_encdec_model.py:241-271) ---------------------------------------------------------------------------------
def rmse_column_names(settings: Dict) -> List[str]:
    """the reference's column names, in channel order: val_lw_rmse_<var>_level_<p>, val_lw_rmse_<surface var>, val_lw_rmse_<static>"""
    names = settings["channel_names"]
    levels = settings.get("pressure_levels", PRESSURE_LEVELS)
    n_atm, n_sur = int(settings.get("num_atm_vars", NUM_ATM_VARS)), int(settings.get("num_sur_vars", NUM_SUR_VARS))
    if len(names) < n_atm + n_sur:
        raise ValueError(f"channel_names holds {len(names)} variables; {n_atm} atmospheric + {n_sur} surface are expected")
    cols = [f"val_lw_rmse_{names[vi]}_level_{p}" for vi in range(n_atm) for p in levels]
    cols += [f"val_lw_rmse_{names[n_atm + si]}" for si in range(n_sur)]
    cols += [f"val_lw_rmse_{s}" for s in settings.get("static_names", [])]
    return cols


def yearly_rows(years: Sequence[Tuple[str, Callable[[], Iterable]]], evaluate: Callable, settings: Dict) -> List[Dict]:
    """one row per year: `evaluate(batches)` -> (val_loss_fn_loss, val_lw_rmse); columns `year`, `val_loss_fn_loss`, then the RMSEs"""
    cols = rmse_column_names(settings)
    rows = []
    for year, batches in years:
        loss, rmse = evaluate(batches())
        if len(rmse) != len(cols):
            raise ValueError(f"year {year}: {len(rmse)} channels were scored, the settings name {len(cols)}")
        row = {"year": year, "val_loss_fn_loss": loss}
        row.update({k: float(v) for k, v in zip(cols, rmse)})
        rows.append(row)
    return rows


def write_csv(rows: List[Dict], csv_path: str):
    with open(csv_path, "w", newline="") as f:
        wr = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
        wr.writeheader()
        wr.writerows(rows)


def npy_batches(path: str, batch_size: int):
    """a year's frames (N, C_in, H_in, W) from a .npy file (memory-mapped), `batch_size` at a time; the last batch may be smaller"""
    arr = np.load(path, mmap_mode="r")
    if arr.ndim != 4:
        raise ValueError(f"{path}: frames must be (N, C_in, H_in, W); got {arr.shape}")
    for i in range(0, arr.shape[0], batch_size):
        yield torch.from_numpy(np.array(arr[i : i + batch_size], dtype=np.float32))


def equiangular_lat_weights(H_in: int, crop_south_pole: bool) -> torch.Tensor:
    """get_normalized_lat_weights_based_on_cos on the rows kept of a pole-to-pole grid of H_in rows (121 rows, cropped: the reference's
    np.linspace(-88.5, 90, 120)), float64 -> fp32"""
    lat = np.linspace(-90.0, 90.0, H_in)[1 if crop_south_pole else 0 :]
    w = np.cos(np.deg2rad(lat))
    return torch.from_numpy(w / w.mean()).to(torch.float32)


def main(argv=None, evaluate: Optional[Callable] = None):
    """`evaluate(batches) -> (val_loss_fn_loss, val_lw_rmse)` replaces the autoencoder and the device (tests of the CSV path)"""
    ap = argparse.ArgumentParser(description="Evaluate a DC-AE's reconstructions per year (evaluate_encdec_model.py on .npy frames)")
    ap.add_argument("--frames", nargs="+", required=True, metavar="YEAR=PATH", help="one .npy of raw frames (N, C_in, H_in, W) per year")
    ap.add_argument("--normalization_json", required=True, help="per-variable mean / std JSON")
    ap.add_argument("--settings_json", required=True, help="JSON with channel_names, static_names [, pressure_levels, num_atm_vars, num_sur_vars]")
    ap.add_argument("--encdec_model", default=None, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--static_path", default=None, help=".npy of the raw static planes (S, H_in, W): land-sea mask, orography")
    ap.add_argument("--batch_size", type=int, default=2)
    ap.add_argument("--sst_channel_idx", type=int, default=82)
    ap.add_argument("--keep_south_pole", action="store_true", help="do not crop the first latitude row")
    ap.add_argument("--incl_sur_pressure", action="store_true", help="keep the last channel of the frames")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    ap.add_argument("--csv_path", required=True)
    args = ap.parse_args(argv)

    with open(args.settings_json) as f:
        settings = json.load(f)
    years, paths = [], []
    for item in args.frames:
        year, sep, path = item.partition("=")
        if not sep or not year or not path:
            raise SystemExit(f"--frames takes YEAR=PATH entries; got {item!r}")
        years.append((year, (lambda p=path: npy_batches(p, args.batch_size))))
        paths.append(path)
    if len({y for y, _ in years}) != len(years):
        raise SystemExit("--frames names a year twice")

    if evaluate is None:
        from ..models import AutoencoderDC
        from .track import mean_std_from_json

        if args.encdec_model is None:
            raise SystemExit("--encdec_model is required")
        with open(args.normalization_json) as f:
            mean_t, std_t = mean_std_from_json(json.load(f), settings["channel_names"])
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
        static = None
        if args.static_path:
            static = torch.from_numpy(np.load(args.static_path).astype(np.float32))
            static = static[:, 1:] if crop else static
        H_in = np.load(paths[0], mmap_mode="r").shape[2]
        lat_w = equiangular_lat_weights(H_in, crop)

        def evaluate(batches):
            return evaluate_reconstruction(model, batches, mean_t, std_t, static, lat_w, sst_channel_idx=args.sst_channel_idx,
                                           crop_south_pole=crop, incl_sur_pressure=args.incl_sur_pressure)

    rows = yearly_rows(years, evaluate, settings)
    write_csv(rows, args.csv_path)
    for r in rows:
        print(f"{r['year']}: val_loss_fn_loss = {r['val_loss_fn_loss']:.6g}")
    print(f"saved per-year validation metrics to {args.csv_path}")
    return rows


if __name__ == "__main__":
    main()
