"""Day-of-year climatology of raw fields on the device -> the ``(366, 4, C, H_in, W)`` table that ``evaluate_ens_gpu`` reads as
``--climatology_path`` (the reference reads a ready-made zarr climatology through xarray; zarr and xarray are out of scope here).

    python -m ladcast_amd.preprocess.compute_climatology --frames 1990-01-01=era5_1990.npy 1991-01-01=era5_1991.npy ... \\
        --output clim.npy [--step_size_hour 6] [--window_days 61] [--window_sigma_days 10] [--start_date D --end_date D] \\
        [--batch_size 32] [--channel_block 0]

Every ``--frames`` entry is ``START=PATH``: a .npy array (N, C, H_in, W) of raw fp32 fields, memory-mapped, whose frame ``t`` has the time
``START + t * step_size_hour``; every frame must fall on hour 0 / 6 / 12 / 18.  ``--start_date`` / ``--end_date`` keep only the frames
in ``[start, end]``.  NaN marks a missing value (SST over land) and is left out of the mean.  What the table holds is defined in
``ladcast_amd.preprocess.climatology``: per (day of year, hour, channel, point) the weighted mean of all samples within
``--window_days`` days (odd, circular in the day of year), weighted by ``exp(-k^2 / (2 sigma^2))`` of their day offset ``k``
(``--window_sigma_days <= 0``: a boxcar; ``--window_days 1``: the plain mean of each slot).  The defaults, 61 days and sigma 10, are this
package's own choice and do not reproduce any published climatology.

The state is 16 bytes per table entry on the device (sum, count, output).  ``--channel_block 0`` takes all channels in one pass over the
frames when that fits in free device memory and the largest block of channels that fits otherwise; each block is one pass over the
frames that reads only its channels from the memory-mapped files.  All rows are kept (``evaluate_ens_gpu`` crops the south pole
itself).  Next to the table, ``<output stem>.json`` records the window, the files, the frames per slot and the empty entries per channel.
"""
from __future__ import annotations

import argparse
import json
import os
from datetime import timedelta
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import hip
from ..evaluate.evaluate_ens_gpu import CLIMATOLOGY_HOURS, _to_datetime
from .climatology import DEFAULT_SIGMA_DAYS, DEFAULT_WINDOW_DAYS, Climatology, slot_of, window_weights
from .compute_mean_std_era5 import frame_batches, open_frames

N_DAYS = 366
STATE_BYTES_PER_ENTRY = 16  # sum (8) + count (4) + out (4)


def parse_frames(items: Sequence[str]) -> Tuple[list, List[str]]:
    """``START=PATH`` entries -> (start datetimes, paths); SystemExit for a malformed entry"""
    starts, paths = [], []
    for item in items:
        start, sep, path = item.partition("=")
        if not sep or not start or not path:
            raise SystemExit(f"--frames takes START=PATH entries; got {item!r}")
        try:
            starts.append(_to_datetime(start))
        except ValueError:
            raise SystemExit(f"--frames {item!r}: {start!r} is not a date (YYYY-MM-DD or YYYY-MM-DDTHH)")
        paths.append(path)
    return starts, paths


def select_frames(starts, counts: Sequence[int], step_size_hour: int, start_date=None, end_date=None):
    """per file the half-open frame range inside [start_date, end_date] and the slots of those frames, in file order;
    SystemExit for a frame off the hour grid"""
    step = timedelta(hours=int(step_size_hour))
    ranges, slots, times = [], [], []
    for t0, n in zip(starts, counts):
        i0 = 0 if start_date is None or start_date <= t0 else min(n, -((t0 - start_date) // step))
        i1 = n if end_date is None else max(i0, min(n, (end_date - t0) // step + 1))
        ranges.append((i0, i1))
        for i in range(i0, i1):
            try:
                slots.append(slot_of(t0 + i * step))
            except ValueError as e:
                raise SystemExit(f"frame {i} of the file starting at {t0.isoformat()}: {e}")
        if i1 > i0:
            times += [t0 + i0 * step, t0 + (i1 - 1) * step]
    return ranges, slots, times


def pick_channel_block(C: int, plane: int, batch_size: int, free_bytes: int) -> int:
    """the largest channel block whose state (16 B per table entry) and two frame batches fit in 90 % of ``free_bytes``; 0: none fits"""
    per_channel = N_DAYS * len(CLIMATOLOGY_HOURS) * plane * STATE_BYTES_PER_ENTRY + 2 * batch_size * plane * 4
    return int(min(C, (free_bytes * 9 // 10) // per_channel))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Day-of-year climatology (366, 4, C, H_in, W) of raw .npy frames on the device")
    ap.add_argument("--frames", nargs="+", required=True, metavar="START=PATH", help="START=PATH: .npy of raw fp32 frames (N, C, H_in, W), the first at START")
    ap.add_argument("--output", required=True, help="the climatology .npy to write; <stem>.json is written next to it")
    ap.add_argument("--step_size_hour", type=int, default=6)
    ap.add_argument("--window_days", type=int, default=DEFAULT_WINDOW_DAYS, help="odd; this package's own default")
    ap.add_argument("--window_sigma_days", type=float, default=DEFAULT_SIGMA_DAYS, help="<= 0: boxcar; this package's own default")
    ap.add_argument("--start_date", default=None, help="keep only frames at or after it")
    ap.add_argument("--end_date", default=None, help="keep only frames at or before it")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--channel_block", type=int, default=0, help="channels per pass over the frames; 0: as many as fit in free device memory")
    args = ap.parse_args(argv)
    if args.batch_size < 1 or args.step_size_hour < 1 or args.channel_block < 0:
        raise SystemExit("--batch_size and --step_size_hour must be at least 1, --channel_block at least 0")
    if args.window_days < 1 or args.window_days % 2 == 0 or args.window_days > N_DAYS:
        raise SystemExit(f"--window_days must be odd and in 1 .. {N_DAYS}; got {args.window_days}")
    weights = window_weights(args.window_days, args.window_sigma_days)
    starts, paths = parse_frames(args.frames)
    try:
        start_date = None if args.start_date is None else _to_datetime(args.start_date)
        end_date = None if args.end_date is None else _to_datetime(args.end_date)
    except ValueError as e:
        raise SystemExit(f"--start_date / --end_date: {e}")
    arrs = open_frames(paths)
    ranges, slots, times = select_frames(starts, [a.shape[0] for a in arrs], args.step_size_hour, start_date, end_date)
    if not slots:
        raise SystemExit("no frames left" + ("" if start_date is None and end_date is None else " between --start_date and --end_date"))
    _, C, H, W = arrs[0].shape

    block = args.channel_block
    if block == 0:
        block = pick_channel_block(C, H * W, args.batch_size, torch.cuda.mem_get_info()[0])
        if block < 1:
            raise SystemExit(f"the state of one channel ({N_DAYS * 4 * H * W * STATE_BYTES_PER_ENTRY} bytes) does not fit in free device memory")
    block = min(block, C)

    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    table = np.lib.format.open_memmap(args.output, mode="w+", dtype=np.float32, shape=(N_DAYS, len(CLIMATOLOGY_HOURS), C, H, W))
    n_empty, frames_per_slot = np.zeros(C, dtype=np.int64), None
    for c0 in range(0, C, block):
        c1 = min(C, c0 + block)
        clim = Climatology(c1 - c0, H, W, "cuda", n_days=N_DAYS)
        pos = 0
        for x in frame_batches([a[i0:i1, c0:c1] for a, (i0, i1) in zip(arrs, ranges)], args.batch_size):
            clim.update(hip.upload_nonblocking(x, clim.device), slots[pos : pos + x.shape[0]])
            pos += x.shape[0]
        table[:, :, c0:c1] = clim.finish(args.window_days, args.window_sigma_days).cpu().numpy()
        n_empty[c0:c1] = clim.n_empty()
        frames_per_slot = clim.frames_per_slot()
        del clim
    table.flush()
    del table

    meta = dict(window_days=args.window_days, window_sigma_days=args.window_sigma_days, weights=weights.tolist(), hours=list(CLIMATOLOGY_HOURS),
                step_size_hour=args.step_size_hour,
                files=[dict(path=p, start=t.isoformat(), frames=int(a.shape[0]), first_frame_used=i0, frames_used=i1 - i0)
                       for p, t, a, (i0, i1) in zip(paths, starts, arrs, ranges)],
                first_time=min(times).isoformat(), last_time=max(times).isoformat(), frames=len(slots), shape=[N_DAYS, len(CLIMATOLOGY_HOURS), C, H, W],
                frames_per_slot=frames_per_slot.tolist(), n_empty=n_empty.tolist(), channel_block=block)
    meta_path = os.path.splitext(args.output)[0] + ".json"
    with open(meta_path, "w") as f:
        json.dump(meta, f, indent=1)
    print(f"{len(slots)} frames from {meta['first_time']} to {meta['last_time']}, {C} channels in blocks of {block}: saved the "
          f"{tuple(meta['shape'])} climatology to {args.output} and its record to {meta_path}")
    return meta


if __name__ == "__main__":
    main()
