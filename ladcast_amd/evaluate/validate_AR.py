"""The reference's validation hook on the device (reference: `log_validation`, ladcast/train_AR.py:55-385): from a latent store and a
checkpoint to the `merged_RMSE` and `CRPS` tables a training run logs every N steps.

Per initial time the known latents start two independent autoregressive chains - Heun ("EDM", `sampler_type="edm"`) and, with `eval_ms`,
the scheduler's multistep loop ("MS", `sampler_type="pipeline"`).  Every chunk's samples are inverse-transformed, decoded lead-major, and
the decoder's output is scored where it lies by one `ldc_validation_scores` launch per decode batch (inverse normalisation fused into the
loads, truth = the decoded store frames as a table with one slot per lead time, output columns at the chunk's offset).  No decoded forecast
outlives its chunk; the reference fills an (ens, 84, T, 120, 240) array per sampler (3.9 GB at ens 10, T 40) and then makes about a dozen
passes of torch ops over it.  One (3, C, T) buffer per sampler and initial time comes to the host.

Chunk timestamps (quirk Q12 of SURVEY.md).  The reference hands chunk `step` the time `init + step * step_size_hour` (train_AR.py:216), not
the time its first frame follows, `init + step * return_seq_len * step_size_hour`, which the rollout driver (pipelines/utils.py) uses.  The
reference's tables are made with the former, so that is the default here; `advance_by_chunk=True` gives the rollout driver's convention.

    python -m ladcast_amd.evaluate.validate_AR --latent_path lat.npy --start_date 2018-01-01 --init_times 2018-01-02T00 2018-01-05T12 \\
        --ar_model AR/ --encdec_model DCAE/ --latent_normal_json latent_normal.json --normalization_json ERA5_normal.json \\
        --channel_names_json names.json --output val/

writes `merged_RMSE.csv` and `CRPS.csv`.  Single rank; training, wandb, zarr / xarray input and more than 64 members are out of scope.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
from datetime import timedelta
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import hip
from ..pipelines.utils import _device_vector, convert_datetime_to_int, ensemble_AR_sampler, inverse_normalize_transform_3D
from .evaluate_ens_gpu import _to_datetime
from .track import LEVELS
from .utils import VALIDATION_SCORE_NAMES, get_normalized_lat_weights_based_on_cos, validation_scores

SAMPLERS = (("EDM", "edm"), ("MS", "pipeline"))  # table prefix, `sampler_type`


class NpyLatentStore:
    """(N, C, h, w) latent frames (array or memmap) `step_size_hour` apart, the first at `start_time`: the `xr_dataset["latents"]` of the
    reference.  `latents_at(times)` -> (len(times), C, h, w) fp32, as `.sel(time=times).values`; a time off the grid or outside the
    store is a KeyError, as a label that is not in the index."""

    def __init__(self, array, start_time, step_size_hour: int = 6):
        if array.ndim != 4:
            raise ValueError(f"latent frames must be (N, C, h, w), got {tuple(array.shape)}")
        self.array, self.start_time, self.step_size_hour = array, _to_datetime(start_time), int(step_size_hour)

    def index_of(self, t) -> int:
        hours, rem = divmod((_to_datetime(t) - self.start_time).total_seconds(), 3600)
        i, off = divmod(int(hours), self.step_size_hour)
        if rem or off or not 0 <= i < self.array.shape[0]:
            raise KeyError(f"{t} is not one of the store's {self.array.shape[0]} frames ({self.step_size_hour} h apart from {self.start_time})")
        return i

    def latents_at(self, times: Sequence) -> np.ndarray:
        return np.stack([np.asarray(self.array[self.index_of(t)], dtype=np.float32) for t in times])


def column_names(channel_names: Sequence[str], levels: Sequence[int] = LEVELS, num_atm_vars: int = 6) -> List[str]:
    """train_AR.py:110-119: `{var}_level{level}` for the first `num_atm_vars` names x levels, then the surface names"""
    names = list(channel_names)
    return [f"{v}_level{lv}" for v in names[:num_atm_vars] for lv in levels] + names[num_atm_vars:]


@functools.lru_cache(maxsize=8)
def _lat_weight(H: int, dev: str) -> torch.Tensor:
    return get_normalized_lat_weights_based_on_cos(torch.from_numpy(np.linspace(-88.5, 90, H))).to(dev, torch.float32)


def _decode_frames(encdec_model, frames: torch.Tensor, batch: int) -> torch.Tensor:
    """(N, C, h, w) latents -> (N, C', H, W) decoded (still normalised), at most `batch` frames per decoder call"""
    if frames.shape[0] <= batch:
        return encdec_model.decode(frames).sample
    return torch.cat([encdec_model.decode(frames[i : i + batch]).sample for i in range(0, frames.shape[0], batch)])


@torch.no_grad()
def validate_initial_time(init_time, latent_store, pipeline, encdec_model, mean_d: torch.Tensor, std_d: torch.Tensor,
                          input_seq_len: int, return_seq_len: int, latent_transform_func: Callable, latent_inv_transform_func: Callable, *,
                          total_num_steps: int, step_size_hour: int = 6, ensemble_size: int = 10, num_inference_steps: int = 20,
                          eval_ms: bool = True, sampler: Callable = ensemble_AR_sampler, decode_batch_frames: Optional[int] = None,
                          advance_by_chunk: bool = False, on_chunk: Optional[Callable] = None) -> Dict[str, torch.Tensor]:
    """One initial time of train_AR.py:157-312 -> {"EDM": (3, C, T), "MS": (3, C, T)} fp32 DEVICE buffers (planes `VALIDATION_SCORE_NAMES`;
    "MS" only with `eval_ms`).  `mean_d` / `std_d`: the field statistics as device vectors; the latitude weights are the reference's
    `get_normalized_lat_weights_based_on_cos(np.linspace(-88.5, 90, H))` (:131-133) for the H decoded rows.
    `on_chunk(name, step, samples)`: called with every chunk's (ens, C, R, h, w) samples before the inverse transform (tests)."""
    dev = mean_d.device
    init, R, T, ens = _to_datetime(init_time), int(return_seq_len), int(total_num_steps), int(ensemble_size)
    hours = timedelta(hours=step_size_hour)
    known = torch.as_tensor(latent_store.latents_at([init - hours * i for i in range(input_seq_len - 1, -1, -1)]), dtype=torch.float32)
    known = latent_transform_func(known.to(dev).permute(1, 0, 2, 3).contiguous()).unsqueeze(0)  # (1, C, T_in, h, w)
    per = max(1, int(decode_batch_frames) // ens) if decode_batch_frames else R  # lead times per decoder call: a lead time's members stay together
    # truth: the store's frames init + step .. init + T * step, decoded and de-normalised once, as the (T, C, H, W) table (:174-195)
    ref = torch.as_tensor(latent_store.latents_at([init + hours * k for k in range(1, T + 1)]), dtype=torch.float32).to(dev)
    ref = _decode_frames(encdec_model, ref, per * ens)
    if ref.shape[1] != mean_d.numel():
        raise ValueError(f"the decoder gives {ref.shape[1]} channels, the field statistics hold {mean_d.numel()}")
    truth = inverse_normalize_transform_3D(ref.unsqueeze(2), mean_d, std_d).squeeze(2)  # per-channel on (T, C, 1, H, W); target_std = 1
    C = truth.shape[1]
    lat_weight = _lat_weight(int(truth.shape[-2]), str(dev))
    names = SAMPLERS[: 2 if eval_ms else 1]
    chain = {name: known for name, _ in names}  # the chains are independent; their chunks alternate as in the reference (:219-244)
    out = {name: torch.full((len(VALIDATION_SCORE_NAMES), C, T), float("nan"), device=dev, dtype=torch.float32) for name, _ in names}
    for step in range(T // R):
        ts_host = convert_datetime_to_int(init + hours * (step * R if advance_by_chunk else step))  # Q12: see the module docstring
        ts = hip.upload_nonblocking(torch.tensor([ts_host]), dev)
        ts.host_values = [ts_host]  # spares the model a device read-back
        for name, sampler_type in names:
            smp = sampler(pipeline, sample_size=ens, return_seq_len=R, num_inference_steps=num_inference_steps, known_latents=chain[name],
                          timestamps=ts, sampler_type=sampler_type, device=dev)
            if on_chunk is not None:
                on_chunk(name, step, smp)
            chain[name] = smp[:, :, -input_seq_len:].contiguous()
            lat = latent_inv_transform_func(smp.contiguous())  # per-channel on (ens, C, R, h, w): the values of the reference's per-member calls
            for s0 in range(0, R, per):
                nl = min(per, R - s0)
                x = lat[:, :, s0 : s0 + nl].permute(2, 0, 1, 3, 4).reshape(nl * ens, lat.shape[1], *lat.shape[3:]).contiguous()  # lead-major
                y = encdec_model.decode(x).sample  # (nl * ens, C, H, W), still normalised; scored where it lies
                l0 = step * R + s0
                validation_scores(y.reshape(nl, ens, *y.shape[1:]), truth, lat_weight, lead_dim=0, mean=mean_d, std=std_d,
                                  truth_slots=list(range(l0, l0 + nl)), out=out[name], lead_offset=l0)
    return out


def _dataframe(table: torch.Tensor, step_hour_list: List[int], col_names: List[str]):
    """train_AR.py:95-108: (lead time, column) values -> DataFrame with a leading "lead time" column"""
    import pandas as pd

    rows = table.tolist()
    data = {"lead time": step_hour_list}
    for j, name in enumerate(col_names):
        data[name] = [row[j] for row in rows]
    return pd.DataFrame(data)


@torch.no_grad()
def log_validation(phase_name: str, latent_store, channel_names: Sequence[str], ar_model, full_field_mean_tensor, full_field_std_tensor,
                   input_seq_len: int, return_seq_len: int, encdec_model, latent_transform_func: Callable, latent_inv_transform_func: Callable,
                   noise_scheduler=None, timestamp_list: Sequence = (), step_size_hour: int = 6, total_lead_time_hour: int = 240,
                   ensemble_size: int = 10, num_inference_steps: int = 20, eval_ms: bool = True, eval_crps: bool = True, return_df: bool = False,
                   *, trackers: Sequence = (), sampler: Callable = ensemble_AR_sampler, decode_batch_frames: Optional[int] = None,
                   advance_by_chunk: bool = False, levels: Sequence[int] = tuple(LEVELS), num_atm_vars: int = 6):
    """train_AR.py:55-385 with the reference's argument names; `latent_store` (any object with `latents_at(list of datetimes)` ->
    (T, C, h, w) fp32, e.g. `NpyLatentStore`) replaces the xarray dataset, `channel_names` is `config.channel_names`, there is no
    accelerator (single rank), and `noise_scheduler` is the scheduler object (default: `EDMDPMSolverMultistepScheduler()`).

    Returns None unless `return_df`; then the `merged_RMSE` DataFrame ("lead time", EDM_ens_*, EDM_single_*, and with `eval_ms` MS_ens_*,
    MS_single_*), or with `eval_crps` the pair (merged_RMSE, CRPS) ("lead time", CRPS_*).  Values: the plain mean over the initial times of
    the per-time scores (a NaN propagates, as the reference's `.mean(dim=0)`), then sqrt for the RMSE table.  Each object in `trackers`
    gets `.log({"merged_RMSE": df, "CRPS": df})` (no "CRPS" without `eval_crps`).  `latent_transform_func` is called with the
    (C, T_in, h, w) known latents, `latent_inv_transform_func` with a chunk's (ens, C, R, h, w) samples: per-channel transforms, as
    `get_transform_3D` / `get_inv_transform_3D` give.  `decode_batch_frames`: frames per decoder call (whole lead times; default: a
    chunk's ens * R).  `sampler`: the chunk sampler (tests).  `advance_by_chunk`: see the module docstring.

    Where the reference's own code fails: `total_lead_time_hour % step_size_hour` raises as there; a last chunk shorter than
    `return_seq_len` cannot be assigned by the reference (:253-263) and is refused; `eval_crps=False` (a NameError at :321) works;
    `return_df` gives DataFrames with the layout of the hook's wandb tables, "lead time" first (the reference's `create_pd_dataframe` is handed
    a column list one longer than its rows and raises an IndexError for every input, :95-108,338-385); the number of column names must equal the decoded channels (the reference hard-wires 84); more than 64 members are not implemented."""
    col_names = column_names(channel_names, levels, num_atm_vars)
    if total_lead_time_hour % step_size_hour != 0:
        raise ValueError("total_lead_time_hour must be divisible by step_size_hour.")
    total_num_steps = int(total_lead_time_hour / step_size_hour)
    if total_num_steps % return_seq_len != 0:
        raise ValueError(f"{total_num_steps} lead times are not a whole number of chunks of return_seq_len = {return_seq_len}: the reference "
                         "cannot assign the last chunk (train_AR.py:253-263)")
    if ensemble_size > 64:
        raise NotImplementedError("more than 64 members are not supported by the scoring kernel")
    if ensemble_size < 1 or input_seq_len < 1:
        raise ValueError("ensemble_size and input_seq_len must be positive")
    C = int(torch.as_tensor(full_field_mean_tensor).numel())
    if len(col_names) != C:
        raise ValueError(f"{len(col_names)} column names for {C} decoded channels")
    dev = torch.device(encdec_model.device)
    if dev.type != "cuda":
        raise RuntimeError("ladcast_amd validation needs the models on the device (no CPU fallback)")
    from ..pipelines import AutoRegressive2DPipeline
    from ..schedulers import EDMDPMSolverMultistepScheduler

    pipeline = AutoRegressive2DPipeline(ar_model, scheduler=noise_scheduler if noise_scheduler is not None else EDMDPMSolverMultistepScheduler())
    step_hour_list = [i * step_size_hour for i in range(1, total_num_steps + 1)]
    mean_d, std_d = _device_vector(full_field_mean_tensor, dev), _device_vector(full_field_std_tensor, dev)
    per_time = {name: [] for name, _ in SAMPLERS[: 2 if eval_ms else 1]}
    for init in timestamp_list:
        bufs = validate_initial_time(init, latent_store, pipeline, encdec_model, mean_d, std_d, input_seq_len, return_seq_len,
                                     latent_transform_func, latent_inv_transform_func, total_num_steps=total_num_steps,
                                     step_size_hour=step_size_hour, ensemble_size=ensemble_size, num_inference_steps=num_inference_steps,
                                     eval_ms=eval_ms, sampler=sampler, decode_batch_frames=decode_batch_frames, advance_by_chunk=advance_by_chunk)
        for name, buf in bufs.items():
            per_time[name].append(buf.cpu())  # the one copy of this sampler and initial time
    if not per_time["EDM"]:
        raise ValueError("timestamp_list is empty")
    mean_scores = {name: torch.stack(v).mean(dim=0) for name, v in per_time.items()}  # (3, C, T): plain mean over the initial times
    ens_i, single_i, crps_i = (VALIDATION_SCORE_NAMES.index(k) for k in ("ens_mse", "single_mse", "crps"))
    merged_col_names, blocks = ["lead time"], []
    for name in mean_scores:
        merged_col_names += [f"{name}_ens_{c}" for c in col_names] + [f"{name}_single_{c}" for c in col_names]
        blocks += [torch.sqrt(mean_scores[name][ens_i]).T, torch.sqrt(mean_scores[name][single_i]).T]
    tables = {"merged_RMSE": _dataframe(torch.cat(blocks, dim=1), step_hour_list, merged_col_names[1:])}
    if eval_crps:
        tables["CRPS"] = _dataframe(mean_scores["EDM"][crps_i].T, step_hour_list, [f"CRPS_{c}" for c in col_names])
    for tracker in trackers:
        tracker.log(dict(tables))
    if return_df:
        return (tables["merged_RMSE"], tables["CRPS"]) if eval_crps else tables["merged_RMSE"]
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description="Validation rollout of an AR checkpoint against a latent store (train_AR.py's log_validation on .npy data)")
    ap.add_argument("--latent_path", type=str, required=True, help=".npy of latent frames (N, C, h, w), step_size_hour apart from start_date")
    ap.add_argument("--start_date", type=str, required=True, help="time of the first frame of --latent_path")
    ap.add_argument("--init_times", nargs="+", required=True, help="initial times (ISO, or YYYYMMDDHH)")
    ap.add_argument("--ar_model", type=str, required=True, help="AR checkpoint directory (config.json + weights)")
    ap.add_argument("--encdec_model", type=str, required=True, help="DC-AE checkpoint directory (config.json + weights) or a config.json")
    ap.add_argument("--latent_normal_json", type=str, required=True, help='{"mean": [...], "std": [...]} of the latents (target_std 0.5)')
    ap.add_argument("--normalization_json", type=str, required=True, help="per-variable mean / std JSON of the decoded fields")
    ap.add_argument("--channel_names_json", type=str, required=True, help="JSON list of variable names: atmospheric first, then surface")
    ap.add_argument("--output", type=str, required=True, help="directory for merged_RMSE.csv and CRPS.csv")
    ap.add_argument("--ensemble_size", type=int, default=10)
    ap.add_argument("--num_inference_steps", type=int, default=20)
    ap.add_argument("--total_lead_time_hour", type=int, default=240)
    ap.add_argument("--step_size_hour", type=int, default=6)
    ap.add_argument("--input_seq_len", type=int, default=1)
    ap.add_argument("--return_seq_len", type=int, default=4)
    ap.add_argument("--no_ms", action="store_true", help="skip the multistep (\"MS\") chain")
    ap.add_argument("--no_crps", action="store_true", help="no CRPS table")
    ap.add_argument("--advance_by_chunk", action="store_true", help="chunk timestamps as the rollout driver's (see the module docstring)")
    ap.add_argument("--decode_batch_frames", type=int, default=None, help="frames per decoder call (default: a chunk's ens * return_seq_len)")
    ap.add_argument("--levels", type=int, nargs="+", default=list(LEVELS), help="pressure levels of the atmospheric variables, in channel order")
    ap.add_argument("--num_atm_vars", type=int, default=6, help="how many of the names are atmospheric (one channel per level)")
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    args = ap.parse_args(argv)

    from ..models import LaDCastTransformer3DModel
    from ..pipelines.utils import get_inv_transform_3D, get_transform_3D
    from .evaluate_ens_gpu import _load_encdec
    from .pred_rollout import load_latent_transform_args
    from .track import mean_std_from_json

    with open(args.channel_names_json) as f:
        names = json.load(f)
    with open(args.normalization_json) as f:
        mean_t, std_t = mean_std_from_json(json.load(f), names)
    latent_args = load_latent_transform_args(args.latent_normal_json)
    ar_model = LaDCastTransformer3DModel.from_pretrained(args.ar_model).to("cuda").eval()
    encdec = _load_encdec(args.encdec_model).to("cuda").eval()
    ar_model.set_gemm_precision(args.gemm_precision)
    encdec.set_gemm_precision(args.gemm_precision)
    store = NpyLatentStore(np.load(args.latent_path, mmap_mode="r"), args.start_date, args.step_size_hour)
    times = [_to_datetime(int(t) if t.isdigit() else t) for t in args.init_times]
    res = log_validation("validation", store, names, ar_model, mean_t, std_t, args.input_seq_len, args.return_seq_len, encdec,
                         get_transform_3D("normalize", latent_args), get_inv_transform_3D("normalize", latent_args), timestamp_list=times,
                         step_size_hour=args.step_size_hour, total_lead_time_hour=args.total_lead_time_hour, ensemble_size=args.ensemble_size,
                         num_inference_steps=args.num_inference_steps, eval_ms=not args.no_ms, eval_crps=not args.no_crps, return_df=True,
                         decode_batch_frames=args.decode_batch_frames, advance_by_chunk=args.advance_by_chunk, levels=args.levels,
                         num_atm_vars=args.num_atm_vars)
    os.makedirs(args.output, exist_ok=True)
    rmse_df, crps_df = (res, None) if args.no_crps else res
    rmse_df.to_csv(os.path.join(args.output, "merged_RMSE.csv"), index=False)
    if crps_df is not None:
        crps_df.to_csv(os.path.join(args.output, "CRPS.csv"), index=False)
    print(f"saved merged_RMSE.csv{'' if crps_df is None else ' and CRPS.csv'} ({len(times)} initial times, {len(rmse_df)} lead times) to {args.output}")
    return res


if __name__ == "__main__":
    main()
