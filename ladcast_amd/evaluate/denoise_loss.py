"""The EDM denoising loss of an AR checkpoint on held-out latents: the training objective's forward half on the device (reference: one
iteration of the loop body of ladcast/train_AR.py:873-1032, everything up to and including `loss = torch.mean(...)`; the backward pass,
optimizer and EMA are out of scope).

`denoising_loss` draws (or is given) one noise level per sample from the scheduler's training schedule, noises and preconditions the target
latents in one launch (`ldc_edm_noise_inputs`), calls the model - with push-forward, slice by slice - and reduces the EDM-weighted squared
error of the preconditioned output to one value per (sample, channel, frame) plane (`ldc_edm_denoise_loss`: fp32 terms in the reference's
order, fp64 sums in a fixed order).  `loss` is the mean of that table, the number the reference logs as `train loss`; the table shows
which noise levels, lead slices and channels carry it.  The loss arithmetic is fp32 / fp64 in every GEMM precision mode; launches are eager.

Quirks of the reference kept on purpose:
  * every push-forward step after the first advances every sample's timestamp by 6 h, whatever the slice length (:935-939);
  * the loss weight is (sigma^2 + 0.5^2) / (sigma * 0.5)^2 with a literal 0.5, not the scheduler's `sigma_data` (:975-977);
  * noise-level indices address the scheduler's 1000-entry TRAINING schedule (`scheduler.timesteps` of a scheduler on which
    `set_timesteps` was never called), not an inference schedule;
  * with `lat_weighted_loss` the 15 latent rows are weighted as latitudes -83.25 .. 84.75 (:858-865).

`evaluate_denoising_loss` runs it over a latent store; as a program:

    python -m ladcast_amd.evaluate.denoise_loss --latent_path lat.npy --start_date 2018-01-01 --init_times 2018-01-02T00 2018-01-05T12 \\
        --ar_model AR/ --latent_normal_json latent_normal.json --sigma_indices 0 250 500 750 999 --output out/

writes `denoise_loss.csv` (one row per sigma index: sigma, number of samples, loss) and `denoise_loss_table.npy` (C, T).
"""
from __future__ import annotations

import argparse
import csv
import os
from dataclasses import dataclass
from datetime import timedelta
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..models.embeddings import convert_int_to_datetime
from ..models.utils import Karras_sigmas_lognormal
from ..pipelines.utils import convert_datetime_to_int, get_sigmas

PUSH_FORWARD_HOURS = 6  # per push-forward step, whatever the slice length (train_AR.py:935-939)
LOSS_LATITUDES = (-83.25, 84.75, 15)  # np.linspace arguments of the latitude weights of the 15 latent rows (train_AR.py:858-865)


@dataclass
class PushForwardStep:
    start: int  # frames [start, end) of the target are predicted by this step
    end: int
    profile: Optional[Tuple[int, int]]  # None: the caller's initial_profile; (a, b): the denoised prediction of frames [a, b)
    hours: int  # added to every sample's timestamp before this step's forward


def push_forward_plan(return_seq_len: int, num_push_forward_steps: int, input_seq_len: int) -> List[PushForwardStep]:
    """Which frames each push-forward step predicts, what it is conditioned on and by how much its timestamps have advanced
    (train_AR.py:636-641,927-964).  `num_push_forward_steps` must divide `return_seq_len`: the reference's assertion."""
    T, K = int(return_seq_len), int(num_push_forward_steps)
    if K < 1 or T % K != 0:
        raise AssertionError(f"num_push_forward_steps {K} must be a divisor of return_seq_len {T}")
    per = T // K
    if K > 1 and not 1 <= input_seq_len <= per:
        raise ValueError(f"push-forward conditions on the {input_seq_len} frames before a slice, but a slice holds only {per}")
    return [PushForwardStep(k * per, (k + 1) * per, None if k == 0 else (k * per - input_seq_len, k * per), PUSH_FORWARD_HOURS * k)
            for k in range(K)]


def advance_timestamps(stamps: Sequence[int], hours: int) -> List[int]:
    """YYYYMMDDHH integers `hours` later (calendar arithmetic on the host)"""
    return [convert_datetime_to_int(convert_int_to_datetime(int(s)) + timedelta(hours=hours)) for s in stamps]


def loss_latitude_weights(H: int) -> torch.Tensor:
    """fp32 (H,) weights cos(lat) / mean(cos(lat)) of the latent rows, evaluated in float64 numpy as the reference does"""
    if H != LOSS_LATITUDES[2]:
        raise ValueError(f"lat_weighted_loss is defined for the {LOSS_LATITUDES[2]} latent rows of the reference, got {H}")
    w = np.cos(np.deg2rad(np.linspace(*LOSS_LATITUDES)))
    return torch.from_numpy(w / w.mean()).float()


@dataclass
class DenoisingLossOutput:
    loss: torch.Tensor  # 0-d device tensor: mean of `table`
    table: torch.Tensor  # (B, C, T): mean weighted squared error of every plane
    per_sample: torch.Tensor  # (B,)
    sigmas: torch.Tensor  # (B,) fp32, host
    indices: torch.Tensor  # (B,) int64, host: entries of the training schedule
    model_pred: torch.Tensor  # (B, C, T, H, W) raw network output F
    denoised: torch.Tensor  # c_skip * noisy + c_out * F
    noisy_images: torch.Tensor
    x_in: torch.Tensor


def _check_objective(noise_scheduler, do_edm_style_training, snr_gamma):
    if "EDM" not in type(noise_scheduler).__name__:
        raise NotImplementedError("only EDM schedulers: the reference's non-EDM loss branches (train_AR.py:979-991) are not built")
    if not do_edm_style_training:
        raise NotImplementedError("do_edm_style_training=False (integer timesteps, noise target) is not built")
    if snr_gamma is not None:
        raise NotImplementedError("snr_gamma loss weighting (train_AR.py:1033 ff.) is not built")
    if len(noise_scheduler.timesteps) != noise_scheduler.config.num_train_timesteps:
        raise ValueError("the scheduler holds an inference schedule (set_timesteps was called): the objective indexes the training schedule")


@torch.no_grad()
def denoising_loss(ar_model, noise_scheduler, initial_profile, clean_images, timestamps, *, indices=None, noise=None, noise_sampler=None,
                   cur_step=0, generator=None, num_push_forward_steps=1, input_seq_len=None, lat_weighted_loss=False,
                   do_edm_style_training=True, snr_gamma=None) -> DenoisingLossOutput:
    """One iteration of train_AR.py:873-1032 without the backward pass.  initial_profile (B, C, T_in, H, W) and clean_images
    (B, C, T, H, W): fp32 device tensors; timestamps (B,): YYYYMMDDHH of the first input frame.  indices: noise-level indices into the
    scheduler's training schedule (otherwise `noise_sampler(B, cur_step=, generator=, device="cpu")`, by default a
    `Karras_sigmas_lognormal` over the scheduler's sigmas); noise: the noise tensor (otherwise drawn on the host with `generator`, after
    the indices).  input_seq_len: frames a push-forward step is conditioned on (default: those of `initial_profile`)."""
    _check_objective(noise_scheduler, do_edm_style_training, snr_gamma)
    if not (clean_images.is_cuda and clean_images.dtype == torch.float32 and clean_images.dim() == 5):
        raise RuntimeError("denoising_loss runs in HIP kernels: clean_images must be an fp32 (B, C, T, H, W) device tensor")
    dev = clean_images.device
    clean_images = clean_images.contiguous()
    B, C, T, H, W = clean_images.shape
    isl = int(initial_profile.shape[2] if input_seq_len is None else input_seq_len)
    plan = push_forward_plan(T, num_push_forward_steps, isl)

    if indices is None:
        if noise_sampler is None:
            noise_sampler = Karras_sigmas_lognormal(noise_scheduler.sigmas)
        indices = noise_sampler(B, cur_step=cur_step, generator=generator, device="cpu")
    indices = torch.as_tensor(indices, dtype=torch.int64).reshape(-1).cpu()
    if indices.numel() != B or int(indices.min()) < 0 or int(indices.max()) >= len(noise_scheduler.timesteps):
        raise ValueError(f"indices: one entry of the {len(noise_scheduler.timesteps)}-entry training schedule per sample ({B})")
    if noise is None:
        noise = torch.randn(clean_images.shape, generator=generator)
    noise = noise.to(dev, torch.float32).contiguous()
    if noise.shape != clean_images.shape:
        raise ValueError("noise has the shape of clean_images")

    timesteps = noise_scheduler.timesteps.cpu()[indices]
    sigmas = get_sigmas(noise_scheduler, timesteps, clean_images.dim(), torch.float32, device="cpu")
    c_in, c_skip, c_out, weight = (hip.upload_nonblocking(v, dev) for v in noise_scheduler.edm_coefficients(sigmas))
    sigma_d = hip.upload_nonblocking(sigmas.reshape(-1).contiguous(), dev)
    timesteps_d = hip.upload_nonblocking(timesteps.to(torch.float32), dev)

    noisy_images, x_in = torch.empty_like(clean_images), torch.empty_like(clean_images)
    hip.edm_noise_inputs(clean_images, noise, sigma_d, c_in, noisy_images, x_in)  # add_noise + precondition_inputs, one launch

    stamps0 = getattr(timestamps, "host_values", None)
    stamps0 = [int(v) for v in (stamps0 if stamps0 is not None else torch.as_tensor(timestamps).reshape(-1).tolist())]
    if len(stamps0) != B:
        raise ValueError(f"timestamps: one per sample ({B})")
    model_pred = torch.full_like(clean_images, float("nan"))
    profile = initial_profile.to(dev, torch.float32)
    for step in plan:
        if step.profile is not None:  # condition on the denoised prediction of the frames just before the slice
            a, b = step.profile
            profile = torch.empty(B, C, b - a, H, W, device=dev, dtype=torch.float32)
            hip.edm_denoise(noisy_images[:, :, a:b], model_pred[:, :, a:b], c_skip, c_out, profile)
        stamps = advance_timestamps(stamps0, step.hours) if step.hours else stamps0
        ts = hip.upload_nonblocking(torch.tensor(stamps), dev)
        ts.host_values = stamps  # the model needs the values on the host: no read-back
        out = ar_model(x_in[:, :, step.start : step.end].contiguous(), timesteps_d, profile, time_elapsed=ts, return_dict=False)[0]
        model_pred[:, :, step.start : step.end] = out

    table = torch.empty(B, C, T, device=dev, dtype=torch.float32)
    denoised = torch.empty_like(clean_images)
    lat_w = hip.upload_nonblocking(loss_latitude_weights(H), dev) if lat_weighted_loss else None
    hip.edm_denoise_loss(noisy_images, model_pred, clean_images, c_skip, c_out, weight, table, lat_weight=lat_w, denoised=denoised)
    t64 = table.double()  # B * C * T values: the two means below are bookkeeping on the kernel's result
    return DenoisingLossOutput(loss=t64.mean().float(), table=table, per_sample=t64.mean(dim=(1, 2)).float(), sigmas=sigmas.reshape(-1),
                               indices=indices, model_pred=model_pred, denoised=denoised, noisy_images=noisy_images, x_in=x_in)


@dataclass
class DenoisingLossReport:
    loss: float  # mean over all evaluated (sample, noise level) pairs
    rows: List[Tuple[int, float, int, float]]  # (sigma index, sigma, number of samples, mean loss), ascending index
    table: np.ndarray  # (C, T) float64: the per-plane table averaged over all pairs


def store_samples(latent_store, init_times, input_seq_len: int, return_seq_len: int):
    """(initial_profile (N, C, T_in, h, w), clean (N, C, T, h, w), timestamps [N]) as the reference's dataset forms a sample
    (dataloader/ar_dataloder.py:144-162): `input_seq_len` frames from the initial time at the store's step, the `return_seq_len` frames
    after them, and the integer timestamp of the FIRST input frame"""
    from .evaluate_ens_gpu import _to_datetime

    hours = timedelta(hours=latent_store.step_size_hour)
    prof, clean, stamps = [], [], []
    for t in init_times:
        t0 = _to_datetime(t)
        frames = latent_store.latents_at([t0 + hours * i for i in range(input_seq_len + return_seq_len)])  # (T_in + T, C, h, w)
        prof.append(frames[:input_seq_len])
        clean.append(frames[input_seq_len:])
        stamps.append(convert_datetime_to_int(t0))
    as_bcthw = lambda v: torch.from_numpy(np.stack(v)).permute(0, 2, 1, 3, 4).contiguous()  # noqa: E731
    return as_bcthw(prof), as_bcthw(clean), stamps


@torch.no_grad()
def evaluate_denoising_loss(latent_store, init_times, ar_model, noise_scheduler=None, *, input_seq_len=1, return_seq_len=1,
                            sigma_indices: Optional[Sequence[int]] = None, num_draws: Optional[int] = None, seed=42, batch_size=8,
                            latent_transform_func: Optional[Callable] = None, noise_sampler=None, cur_step=0, num_push_forward_steps=1,
                            lat_weighted_loss=False) -> DenoisingLossReport:
    """The denoising loss over the samples of a latent store (`NpyLatentStore`) that start at `init_times`.

    sigma_indices: every sample is evaluated at each of these entries of the training schedule; each index sees the same noise (a host
    generator seeded `seed`, re-seeded per index, consumed batch by batch), so the rows differ by the noise level alone.
    num_draws: instead, `num_draws` passes over the samples with indices drawn by `noise_sampler` (default `Karras_sigmas_lognormal`) at
    `cur_step`, indices and noise from one generator seeded `seed`.  `latent_transform_func`: applied to both device tensors of a batch
    (the latent normalisation)."""
    if (sigma_indices is None) == (num_draws is None):
        raise ValueError("give either sigma_indices or num_draws")
    from ..schedulers import EDMDPMSolverMultistepScheduler

    noise_scheduler = noise_scheduler if noise_scheduler is not None else EDMDPMSolverMultistepScheduler()
    dev = ar_model.device
    prof, clean, stamps = store_samples(latent_store, init_times, input_seq_len, return_seq_len)
    N = clean.shape[0]
    tf = latent_transform_func if latent_transform_func is not None else (lambda x: x)
    passes = [("index", int(s)) for s in sigma_indices] if sigma_indices is not None else [("draw", d) for d in range(int(num_draws))]
    gen = torch.Generator().manual_seed(seed)
    acc = {}  # sigma index -> [sigma, n, sum of per-sample losses]
    table_sum, pairs = None, 0
    for kind, value in passes:
        if kind == "index":
            gen = torch.Generator().manual_seed(seed)
        for i0 in range(0, N, batch_size):
            sl = slice(i0, min(N, i0 + batch_size))
            n = sl.stop - sl.start
            out = denoising_loss(ar_model, noise_scheduler, tf(prof[sl].to(dev)), tf(clean[sl].to(dev)), torch.tensor(stamps[sl]),
                                 indices=[value] * n if kind == "index" else None, noise_sampler=noise_sampler, cur_step=cur_step, generator=gen,
                                 num_push_forward_steps=num_push_forward_steps, input_seq_len=input_seq_len, lat_weighted_loss=lat_weighted_loss)
            per = out.per_sample.double().cpu()
            for idx, sig, v in zip(out.indices.tolist(), out.sigmas.tolist(), per.tolist()):
                a = acc.setdefault(idx, [sig, 0, 0.0])
                a[1] += 1
                a[2] += v
            t = out.table.double().sum(dim=0).cpu()
            table_sum = t if table_sum is None else table_sum + t
            pairs += n
    rows = [(idx, a[0], a[1], a[2] / a[1]) for idx, a in sorted(acc.items())]
    return DenoisingLossReport(loss=sum(a[2] for a in acc.values()) / pairs, rows=rows, table=(table_sum / pairs).numpy())


def write_report(report: DenoisingLossReport, output: str):
    os.makedirs(output, exist_ok=True)
    with open(os.path.join(output, "denoise_loss.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["sigma_index", "sigma", "num_samples", "loss"])
        for idx, sigma, n, loss in report.rows:
            w.writerow([idx, repr(float(sigma)), n, repr(float(loss))])
    np.save(os.path.join(output, "denoise_loss_table.npy"), report.table)


def build_parser():
    ap = argparse.ArgumentParser(description="EDM denoising loss of an AR checkpoint on a latent store, per noise level / lead slice / channel")
    ap.add_argument("--latent_path", type=str, required=True, help=".npy of latent frames (N, C, h, w), step_size_hour apart from start_date")
    ap.add_argument("--start_date", type=str, required=True, help="time of the first frame of --latent_path")
    ap.add_argument("--init_times", nargs="+", required=True, help="times of the samples' first input frames (ISO, or YYYYMMDDHH)")
    ap.add_argument("--ar_model", type=str, required=True, help="AR checkpoint directory (config.json + weights)")
    ap.add_argument("--latent_normal_json", type=str, required=True, help='{"mean": [...], "std": [...]} of the latents (target_std 0.5)')
    ap.add_argument("--output", type=str, required=True, help="directory for denoise_loss.csv and denoise_loss_table.npy")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--sigma_indices", type=int, nargs="+", default=None, help="entries of the 1000-entry training schedule to evaluate every sample at")
    how.add_argument("--num_draws", type=int, default=None, help="instead: this many passes with indices drawn by the training noise sampler")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--cur_step", type=int, default=0, help="training step the noise sampler's log-normal parameters are taken at (--num_draws)")
    ap.add_argument("--num_push_forward_steps", type=int, default=1)
    ap.add_argument("--lat_weighted_loss", action="store_true")
    ap.add_argument("--step_size_hour", type=int, default=6)
    ap.add_argument("--input_seq_len", type=int, default=1)
    ap.add_argument("--return_seq_len", type=int, default=4)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--gemm_precision", type=str, default="fp32", choices=("fp32", "bf16x3", "bf16"))
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.sigma_indices is None and args.num_draws is None:
        args.sigma_indices = [0, 250, 500, 750, 999]

    from ..models import LaDCastTransformer3DModel
    from ..pipelines.utils import get_transform_3D
    from .evaluate_ens_gpu import _to_datetime
    from .pred_rollout import load_latent_transform_args
    from .validate_AR import NpyLatentStore

    latent_args = load_latent_transform_args(args.latent_normal_json)
    ar_model = LaDCastTransformer3DModel.from_pretrained(args.ar_model).to("cuda").eval()
    ar_model.set_gemm_precision(args.gemm_precision)
    store = NpyLatentStore(np.load(args.latent_path, mmap_mode="r"), args.start_date, args.step_size_hour)
    times = [_to_datetime(int(t) if t.isdigit() else t) for t in args.init_times]
    report = evaluate_denoising_loss(store, times, ar_model, input_seq_len=args.input_seq_len, return_seq_len=args.return_seq_len,
                                     sigma_indices=args.sigma_indices, num_draws=args.num_draws, seed=args.seed, batch_size=args.batch_size,
                                     latent_transform_func=get_transform_3D("normalize", latent_args), cur_step=args.cur_step,
                                     num_push_forward_steps=args.num_push_forward_steps, lat_weighted_loss=args.lat_weighted_loss)
    write_report(report, args.output)
    print(f"denoising loss {report.loss:.6g} over {len(times)} samples x {len(report.rows)} noise levels; saved denoise_loss.csv and "
          f"denoise_loss_table.npy to {args.output}")
    return report


if __name__ == "__main__":
    main()
