"""Forecast products of a saved ensemble rollout on the device (not in the reference): the `latent_YYYYMMDDHH.npy` files a rollout wrote ->
per grid point the ensemble mean, spread, range, quantile maps and probabilities of exceeding a threshold, for a forecast that has no
truth yet.

Per initial time the latents are decoded lead-major, as `evaluate_ens_gpu.score_latent_rollout` decodes them - one lead time's members
per decoder call, a few lead times per decode batch - and every decode batch goes through one `ldc_rollout_products` launch where it
lies: the inverse normalisation is fused into the loads, only the selected channels are read, and the products - the forecast reduced by
the ensemble size - are all that leaves the device.  Decoded fields never exist beyond one decode batch.

    python -m ladcast_amd.evaluate.products --result_path rollout/ --normalization_json norm.json --encdec_model DCAE_DIR \\
        --channels 2m_temperature geopotential_level500 81 --quantiles 0.1 0.5 0.9 \\
        --exceed 2m_temperature gt 303.15 --exceed mean_sea_level_pressure lt 98000 --output products/

Channels are named as `validate_AR.column_names(track.VARIABLE_NAMES)` names them (`geopotential_level500`, `2m_temperature`, ...) or by
index.  Per `latent_YYYYMMDDHH.npy` one `products_YYYYMMDDHH.npz` with `mean`, `std`, `min`, `max` (Cs, lead time, H, W), `quantiles`
(Q, Cs, lead time, H, W) and `exceed` (P, Cs, lead time, H, W), and one `products.json` with the channel names, the quantiles, the
thresholds with their direction and the ensemble size.  `--derive NAME speed|diff|shear|vorticity|divergence CHANNEL ...` adds a derived field (`derived`) as one
more channel - `--derive wind_speed_10m speed 10m_u_component_of_wind 10m_v_component_of_wind --exceed wind_speed_10m gt 17.2` maps the
probability of gale-force wind - and `products.json` gains `derived`.  A threshold applies to its one channel: the other channels of that `exceed`
plane hold NaN.  Single rank; `.npy` / `.npz` only.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .track import LEVELS, NUM_ATM_VARS, VARIABLE_NAMES, mean_std_from_json
from .utils import MAX_PRODUCT_QUANTILES, MAX_PRODUCT_THRESHOLDS, PRODUCT_STAT_NAMES, empty_products, rollout_products
from .validate_AR import column_names

PRODUCT_KEYS = PRODUCT_STAT_NAMES + ("quantiles", "exceed")
DIRECTIONS = {"gt": 1, "lt": -1}


@torch.no_grad()
def products_of_latent_rollout(latents_or_path: Union[str, torch.Tensor], encdec_model, mean_tensor, std_tensor, *, quantiles: Sequence[float] = (),
                               thresholds=None, threshold_dirs: Optional[Sequence[int]] = None, channels: Optional[Sequence[int]] = None,
                               total_num_steps: Optional[int] = None, crop_init: bool = False, force_ens_size: Optional[int] = None,
                               decode_batch_frames: Optional[int] = None, derived: Optional[Sequence] = None) -> Dict[str, torch.Tensor]:
    """One initial time: a saved `latent_YYYYMMDDHH.npy` (or its (ens, C, T, h, w) tensor) -> fp32 CPU tensors `mean`, `std`, `min`, `max`
    (Cs, total_num_steps, H, W), and with quantiles / thresholds `quantiles` (Q, Cs, total_num_steps, H, W) / `exceed` (P, Cs,
    total_num_steps, H, W), in physical units (`mean_tensor` / `std_tensor`: one value per decoded channel).

    The T lead times are decoded lead-major, `max(1, decode_batch_frames // ens)` of them per decode batch (default: one), and each decode
    batch goes through one `rollout_products` launch where it lies: the peak memory for decoded fields is one decode batch plus one
    decoder output.  Inside a batch every lead time's members are decoded by a decoder call of their own, always `ens` frames: the
    decoder's convolutions pick their schedule from the launch size, so frames decoded in calls of different sizes differ in the last
    bits, and a performance setting must not move a forecast product.  With decoder calls of one fixed size the products hold the same
    bits under every `decode_batch_frames`.  `quantiles`, `thresholds` (P, Cs), `threshold_dirs`, `channels`: as `rollout_products`.
    Columns T .. total_num_steps - 1 stay NaN; T > total_num_steps is a ValueError.  `crop_init` drops slot 0 (the IC latent),
    `force_ens_size` keeps the first members.

    `derived`: a sequence of `derived.Derived(name, kind, channels)`; the D fields become channels C' .. C' + D - 1, which `channels`
    and the columns of `thresholds` then address like any other: every decode batch is assembled in a (lead, ens, C' + D, H, W) buffer
    whose tail `derive_forecast` fills in physical units.  The products of the decoded channels keep their bits."""
    from ..pipelines.io import load_latent_npy
    from ..pipelines.utils import _device_vector

    if isinstance(latents_or_path, (str, os.PathLike)):
        latents, _ = load_latent_npy(os.fspath(latents_or_path), crop_init=crop_init, force_ens_size=force_ens_size)
    else:
        latents = latents_or_path
        if latents.dim() != 5:
            raise ValueError(f"latents must be (ens, C, T, h, w), got {tuple(latents.shape)}")
        if crop_init:
            latents = latents[:, :, 1:]
        if force_ens_size is not None:
            latents = latents[:force_ens_size]
    ens, C, T, h, w = latents.shape
    total = T if total_num_steps is None else int(total_num_steps)
    if T > total:
        raise ValueError(f"the latents hold {T} lead times, total_num_steps is {total}")
    if ens < 1 or T < 1:
        raise ValueError(f"nothing to decode in latents of shape {tuple(latents.shape)}")
    dev = encdec_model.device
    if torch.device(dev).type != "cuda":
        raise RuntimeError("ladcast_amd products need the model on the device (no CPU fallback)")
    mean_d, std_d = _device_vector(mean_tensor, dev), _device_vector(std_tensor, dev)
    ext = None
    if derived is not None:
        from .derived import ExtendedBatch

        ext = ExtendedBatch(derived, mean_d, std_d)
    latents = latents.to(dev, torch.float32)
    quantiles = list(quantiles)
    thr_d = None if thresholds is None else torch.as_tensor(thresholds, dtype=torch.float32).to(dev)
    per = max(1, int(decode_batch_frames) // ens) if decode_batch_frames else 1  # lead times per decode batch: a lead time's members stay together
    prod = y = None
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        for k in range(nl):  # one decoder call per lead time, always `ens` frames: the same schedule, so the same bits, under every batch size
            yk = encdec_model.decode(latents[:, :, s0 + k].contiguous()).sample  # (ens, C', H, W), still normalised
            if ext is not None:  # the batch is assembled in the head channels of the extended buffer
                if yk.shape[1] != ext.C:
                    raise ValueError(f"the decoder gives {yk.shape[1]} channels, mean_tensor / std_tensor hold {ext.C}")
                ext.buffer(per, ens, yk.shape[2], yk.shape[3], dev)[k, :, : ext.C].copy_(yk)
                continue
            if nl == 1:
                y = yk.unsqueeze(0)
                break
            if y is None or y.shape[0] < nl:
                y = torch.empty(per, *yk.shape, device=dev, dtype=torch.float32)  # the decode batch, lead-major: (lead, ens, C', H, W)
            y[k].copy_(yk)
        if ext is not None:
            y = ext.derive(nl)
        if prod is None:
            Cs = y.shape[2] if channels is None else len(channels)
            prod = empty_products(Cs, total, y.shape[3], y.shape[4], dev, n_quantiles=len(quantiles),
                                  n_thresholds=0 if thr_d is None else thr_d.shape[0])
        rollout_products(y[:nl], quantiles=quantiles, thresholds=thr_d, threshold_dirs=threshold_dirs, channels=channels, lead_dim=0,
                         mean=mean_d if ext is None else ext.mean, std=std_d if ext is None else ext.std, out=prod, l_off=s0)
    return {k: v.cpu() for k, v in prod.items()}


def resolve_channels(tokens: Sequence[str], names: Sequence[str]) -> List[int]:
    """channel names (`column_names`) or indices -> indices into `names`"""
    out = []
    for tok in tokens:
        tok = str(tok)
        if tok in names:
            out.append(list(names).index(tok))
        elif tok.lstrip("-").isdigit() and 0 <= int(tok) < len(names):
            out.append(int(tok))
        else:
            raise ValueError(f"channel {tok!r} is neither one of the {len(names)} channel names nor an index into them")
    return out


def threshold_table(exceed: Sequence[Sequence[str]], channels: Sequence[int], names: Sequence[str]) -> Tuple[Optional[torch.Tensor], List[int], List[dict]]:
    """`--exceed CHANNEL gt|lt VALUE` entries -> ((P, Cs) fp32 table, NaN outside each threshold's own channel; directions; the
    entries as they go into products.json).  A channel that is not among `channels` is an error."""
    if not exceed:
        return None, [], []
    table = torch.full((len(exceed), len(channels)), float("nan"), dtype=torch.float32)
    dirs, meta = [], []
    for k, (chan, direction, value) in enumerate(exceed):
        c = resolve_channels([chan], names)[0]
        if c not in channels:
            raise ValueError(f"--exceed {chan}: channel {names[c]} is not among --channels")
        if direction not in DIRECTIONS:
            raise ValueError(f"--exceed {chan} {direction}: the direction is gt or lt")
        table[k, list(channels).index(c)] = float(value)
        dirs.append(DIRECTIONS[direction])
        meta.append(dict(channel=names[c], channel_index=c, direction=direction, threshold=float(value)))
    return table, dirs, meta


def main(argv=None, products: Optional[Callable] = None):
    """`products(path, time_str) -> {name: array}` replaces the autoencoder and the device (tests of the file handling).  Returns the
    content of `products.json`."""
    ap = argparse.ArgumentParser(description="Ensemble mean, spread, range, quantiles and exceedance probabilities of saved ensemble rollouts")
    ap.add_argument("--result_path", type=str, required=True, help="directory of the rollout's latent_YYYYMMDDHH.npy files")
    ap.add_argument("--normalization_json", type=str, default="ERA5_normal.json", help="per-variable mean / std JSON of the decoded fields")
    ap.add_argument("--encdec_model", type=str, default=None, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--output", type=str, required=True, help="directory for products_YYYYMMDDHH.npz and products.json")
    ap.add_argument("--channels", nargs="+", default=None, help="channels by name or index, in output order (default: all)")
    ap.add_argument("--quantiles", type=float, nargs="*", default=[], help=f"up to {MAX_PRODUCT_QUANTILES} values in [0, 1]")
    ap.add_argument("--exceed", nargs=3, action="append", default=[], metavar=("CHANNEL", "gt|lt", "VALUE"),
                    help=f"probability that CHANNEL is above (gt) / below (lt) VALUE, in physical units; up to {MAX_PRODUCT_THRESHOLDS} times")
    ap.add_argument("--derive", nargs="+", action="append", default=[], metavar="NAME_KIND_CHANNELS",
                    help="NAME speed|diff|shear|vorticity|divergence CHANNEL [CHANNEL ...]: a derived field (wind speed sqrt(a^2 + b^2), difference a - b, shear sqrt((a - c)^2 + (b - d)^2), "
                         "relative vorticity or divergence of the wind u v on the grid) "
                         "as one more channel, which --channels and --exceed then name; may be given several times")
    ap.add_argument("--total_num_steps", type=int, default=None, help="lead-time columns of the products (default: those of each file)")
    ap.add_argument("--crop_init", action="store_true", help="drop slot 0 of the latents (the initial condition)")
    ap.add_argument("--force_ens_size", type=int, default=None, help="use the first members only")
    ap.add_argument("--decode_batch_frames", type=int, default=None, help="decoded frames alive at once = frames per products launch (default: one lead time's members)")
    ap.add_argument("--variable_names", nargs="+", default=VARIABLE_NAMES, help="variables of the normalisation JSON, in channel order")
    ap.add_argument("--levels", type=int, nargs="+", default=LEVELS, help="pressure levels of the atmospheric variables, in channel order")
    ap.add_argument("--num_atm_vars", type=int, default=NUM_ATM_VARS, help="how many of --variable_names have one channel per level")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    args = ap.parse_args(argv)

    names = column_names(args.variable_names, args.levels, args.num_atm_vars)
    fields, derived_meta = None, []
    if args.derive:
        from .derived import derived_metadata, parse_derived

        decoded = names
        fields = parse_derived(args.derive, decoded)
        derived_meta = derived_metadata(fields, decoded)
        names = decoded + [f.name for f in fields]
    channels = list(range(len(names))) if args.channels is None else resolve_channels(args.channels, names)
    if len(args.quantiles) > MAX_PRODUCT_QUANTILES or any(not 0.0 <= q <= 1.0 for q in args.quantiles):
        raise ValueError(f"--quantiles: up to {MAX_PRODUCT_QUANTILES} values in [0, 1]")
    if len(args.exceed) > MAX_PRODUCT_THRESHOLDS:
        raise ValueError(f"--exceed: up to {MAX_PRODUCT_THRESHOLDS} thresholds")
    thr, dirs, thr_meta = threshold_table(args.exceed, channels, names)

    from ..pipelines.io import list_latent_files

    files = list_latent_files(args.result_path)
    if not files:
        raise SystemExit(f"{args.result_path}: no latent_*.npy")

    if products is None:
        if args.encdec_model is None:
            raise SystemExit("--encdec_model is required")
        from .evaluate_ens_gpu import _load_encdec

        with open(args.normalization_json) as f:
            mean_t, std_t = mean_std_from_json(json.load(f), args.variable_names)
        if fields is not None:
            derived_meta = derived_metadata(fields, decoded, std_t)
        model = _load_encdec(args.encdec_model).to("cuda").eval()
        model.set_gemm_precision(args.gemm_precision)

        def products(path, time_str):
            return products_of_latent_rollout(path, model, mean_t, std_t, quantiles=args.quantiles, thresholds=thr, threshold_dirs=dirs,
                                              channels=None if args.channels is None else channels, total_num_steps=args.total_num_steps,
                                              crop_init=args.crop_init, force_ens_size=args.force_ens_size,
                                              decode_batch_frames=args.decode_batch_frames, derived=fields)

    os.makedirs(args.output, exist_ok=True)
    ens_size = None
    for i, (time_str, path) in enumerate(files):
        print(f"processing time_str: {time_str}, remaining: {len(files) - i - 1}")
        res = products(path, time_str)
        arrays = {k: np.asarray(res[k], dtype=np.float32) for k in PRODUCT_KEYS if k in res}
        for k, a in arrays.items():
            lead = a.shape[:-3]
            if lead[-1] != len(channels):
                raise ValueError(f"{time_str}: {k} is {a.shape}, expected {len(channels)} channels")
        np.savez(os.path.join(args.output, f"products_{time_str}.npz"), **arrays)
        shape = np.load(path, mmap_mode="r").shape
        n = shape[-5] if args.force_ens_size is None else min(shape[-5], args.force_ens_size)
        if ens_size not in (None, n):
            raise ValueError(f"{path}: {n} members, the files before had {ens_size}")
        ens_size = n
    meta = dict(channels=[names[c] for c in channels], channel_indices=channels, quantiles=[float(q) for q in args.quantiles],
                thresholds=thr_meta, ensemble_size=int(ens_size), init_times=[t for t, _ in files])
    if fields is not None:
        meta["derived"] = derived_meta
    with open(os.path.join(args.output, "products.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"saved products of {len(files)} initial times x {len(channels)} channels to {args.output}")
    return meta


if __name__ == "__main__":
    main()
