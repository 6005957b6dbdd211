"""Per-variable mean / std of raw fields on the device -> the normalisation JSON (reference: ladcast/preprocecss/compute_mean_std_era5.py,
which writes static/ERA5_normal_1979_2017.json from a zarr store with xarray).

    python -m ladcast_amd.preprocess.compute_mean_std_era5 --frames era5_1979.npy era5_1980.npy ... --output ERA5_normal.json \\
        [--variable_names_json names.json] [--static land_sea_mask=lsm.npy ...] [--batch_size 32]

Frames are .npy arrays (N, C, H, W) of raw fp32 fields, memory-mapped and streamed ``--batch_size`` frames at a time; channel order =
the variable order of the names (atmospheric variables first, one channel per level), which default to the 84 channels of
``evaluate.track.VARIABLE_NAMES`` / ``LEVELS``.  The names JSON holds ``channel_names`` (or ``variable_names``), ``pressure_levels`` (or
``levels``) and ``num_atm_vars``, as the settings JSON of ``evaluate_encdec_model`` does.  Statistics are the population mean / std
(ddof = 0) of the non-NaN values over time and ALL rows - no south-pole crop, as the reference script takes them.  A ``--static`` file is
one variable, (H, W) or (k, H, W), all of its values pooled.  zarr, xarray and multi-rank splitting are out of scope.
"""
from __future__ import annotations

import argparse
import json
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from .stats import FieldMoments, normalization_dict


def open_frames(paths: Sequence[str], channels: Optional[int] = None) -> List[np.ndarray]:
    """memory-map the .npy frame files and check them: 4-D, fp32, one channel count and grid (SystemExit otherwise)"""
    arrs = []
    for p in paths:
        a = np.load(p, mmap_mode="r")
        if a.ndim != 4:
            raise SystemExit(f"{p}: frames must be (N, C, H, W); got {a.shape}")
        if a.dtype != np.float32:
            raise SystemExit(f"{p}: frames must be float32; got {a.dtype}")
        if arrs and a.shape[1:] != arrs[0].shape[1:]:
            raise SystemExit(f"{p}: frames are {a.shape[1:]}, the first file's are {arrs[0].shape[1:]}")
        if channels is not None and a.shape[1] != channels:
            raise SystemExit(f"{p}: {a.shape[1]} channels, the variable names give {channels}")
        arrs.append(a)
    return arrs


def frame_batches(arrs: Sequence[np.ndarray], batch_size: int) -> Iterable[torch.Tensor]:
    """the frames of all files as one sequence, ``batch_size`` at a time: a batch may span two files, the last one may be smaller"""
    pending, have = [], 0
    for a in arrs:
        i = 0
        while i < a.shape[0]:
            take = min(batch_size - have, a.shape[0] - i)
            pending.append(np.asarray(a[i : i + take]))
            have += take
            i += take
            if have == batch_size:
                yield torch.from_numpy(np.concatenate(pending) if len(pending) > 1 else np.array(pending[0]))
                pending, have = [], 0
    if have:
        yield torch.from_numpy(np.concatenate(pending) if len(pending) > 1 else np.array(pending[0]))


def compute_mean_std(batches: Iterable[torch.Tensor], C: int, device="cuda") -> FieldMoments:
    """Stream fp32 batches (B, C, H, W) (host batches are uploaded) through one `FieldMoments`, which is returned: ``.count()``, ``.mean()``
    and ``.std()`` are the statistics of everything seen.  The host never waits for the device inside the loop."""
    fm = FieldMoments(C, device)
    for x in batches:
        fm.update(hip.upload_nonblocking(torch.as_tensor(x), fm.device))
    return fm


def load_names(path: Optional[str]) -> Tuple[List[str], List[int], Optional[int]]:
    """(variable names, levels, num_atm_vars) from the names JSON, or the package's 84-channel default"""
    if path is None:
        from ..evaluate.track import LEVELS, NUM_ATM_VARS, VARIABLE_NAMES

        return list(VARIABLE_NAMES), list(LEVELS), NUM_ATM_VARS
    with open(path) as f:
        d = json.load(f)
    if isinstance(d, list):
        d = {"channel_names": d}
    names = d.get("channel_names", d.get("variable_names"))
    if not names:
        raise SystemExit(f"{path}: no channel_names / variable_names")
    from ..evaluate.track import LEVELS, NUM_ATM_VARS

    levels = d.get("pressure_levels", d.get("levels", LEVELS))
    n_atm = d.get("num_atm_vars", NUM_ATM_VARS if "pressure_levels" not in d and "levels" not in d else None)
    return list(names), [int(p) for p in levels], None if n_atm is None else int(n_atm)


def channel_count(names: Sequence[str], levels: Sequence[int], n_atm: Optional[int]) -> int:
    if n_atm is None:
        raise SystemExit("the names JSON gives levels but no num_atm_vars")
    if not 0 <= n_atm <= len(names):
        raise SystemExit(f"num_atm_vars = {n_atm} of {len(names)} variables")
    return n_atm * len(levels) + len(names) - n_atm


def main(argv=None):
    ap = argparse.ArgumentParser(description="Per-variable mean / std of raw .npy frames on the device -> the normalisation JSON")
    ap.add_argument("--frames", nargs="+", required=True, metavar="PATH", help=".npy files of raw fp32 frames (N, C, H, W)")
    ap.add_argument("--variable_names_json", default=None, help="JSON with channel_names, pressure_levels, num_atm_vars (default: the 84 channels)")
    ap.add_argument("--static", nargs="*", default=[], metavar="NAME=PATH", help="static variables: .npy (H, W) or (k, H, W), pooled")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--output", required=True, help="the normalisation JSON to write")
    args = ap.parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    names, levels, n_atm = load_names(args.variable_names_json)
    C = channel_count(names, levels, n_atm)
    arrs = open_frames(args.frames, C)
    statics = []
    for item in args.static:
        name, sep, path = item.partition("=")
        if not sep or not name or not path:
            raise SystemExit(f"--static takes NAME=PATH entries; got {item!r}")
        if name in names or name in [s[0] for s in statics]:
            raise SystemExit(f"--static names {name!r} twice")
        a = np.load(path, mmap_mode="r")
        if a.ndim not in (2, 3) or a.dtype != np.float32:
            raise SystemExit(f"{path}: a static variable is a float32 (H, W) or (k, H, W) array; got {a.dtype} {a.shape}")
        statics.append((name, a))

    fm = compute_mean_std(frame_batches(arrs, args.batch_size), C)
    mean, std = fm.mean_std()
    out = normalization_dict(mean, std, names, levels, num_atm_vars=n_atm)
    for name, a in statics:
        planes = torch.from_numpy(np.array(a, dtype=np.float32)).reshape(-1, 1, a.shape[-2], a.shape[-1])  # (k, 1, H, W): one pooled channel
        m, s = compute_mean_std([planes], 1).mean_std()
        out[name] = {"mean": float(m[0]), "std": float(s[0])}
    with open(args.output, "w") as f:
        json.dump(out, f, indent=4)
    n = int(fm.count().max()) if sum(a.shape[0] for a in arrs) else 0
    print(f"{sum(a.shape[0] for a in arrs)} frames, {C} channels (up to {n} values each): saved mean / std of {len(out)} variables to {args.output}")
    return out


if __name__ == "__main__":
    main()
