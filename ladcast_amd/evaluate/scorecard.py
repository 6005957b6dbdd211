"""Scorecard: is run B better or worse than run A, and is the difference more than sampling noise?  (No counterpart in the reference.)

Two score directories written by `evaluate_ens_gpu` - the same forecast in two arithmetics, model sizes, ensemble sizes ... - are paired
on their common initial times, the initial times are resampled in blocks (scores of neighbouring initial times are correlated) and every
(channel, lead time) series gets the two point estimates, their difference and ratio with percentile intervals, a two-sided p-value and
a verdict.  The resampling table is made on the host (`block_bootstrap_draws`); the replicate sums, the order statistics and the sign
counts are one `ldc_paired_bootstrap` call per chunk of series (`paired_bootstrap`; include/ladcast_hip.h states every definition).

    python -m ladcast_amd.evaluate.scorecard --a scores_fp32/ --b scores_bf16x3/ --output card/ --rmse_of ens_mse --leads 4 12 20 28 40

Gaps between initial times are ignored: the blocks are runs of consecutive AVAILABLE common initial times, whatever lies between them.
float64 score files (the energy scores) are rounded to fp32 on load: the kernel reads fp32.  A pair of scores is used when both are
finite.  At most `hip.lib.ldc_paired_bootstrap_max_replicates()` (16384) replicates.  Multiple-comparison correction, studentised or
BCa intervals, resampling across members and plots are out of scope.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from .utils import SCORE_NAMES

STAT_FIELDS = ("a_hat", "b_hat", "diff_hat", "ratio_hat", "diff_lo", "diff_hi", "ratio_lo", "ratio_hi")
COUNT_FIELDS = ("n_valid", "n_used", "n_le0", "n_ge0")
KINDS = {"mean": 0, "root_mean": 1}
DEFAULT_WORKSPACE_BYTES = 256 << 20
DEFAULT_HIGHER_IS_BETTER = ("ens_acc",)


def block_bootstrap_draws(n: int, n_boot: int, block: int, seed: int) -> np.ndarray:
    """Circular moving-block bootstrap: (n_boot, n) int32, every replicate ceil(n / block) blocks of `block` consecutive indices mod n,
    truncated to n draws; the block starts are uniform in [0, n) from `np.random.Generator(np.random.PCG64(seed))`.  block == 1 is the
    iid bootstrap.  Host only, the same table for the same seed."""
    n, n_boot, block = int(n), int(n_boot), int(block)
    if n < 1 or n_boot < 1 or not 1 <= block <= n:
        raise ValueError(f"block_bootstrap_draws needs n >= 1, n_boot >= 1 and 1 <= block <= n; got n={n}, n_boot={n_boot}, block={block}")
    rng = np.random.Generator(np.random.PCG64(seed))
    n_blocks = -(-n // block)
    starts = rng.integers(0, n, size=(n_boot, n_blocks), dtype=np.int64)
    idx = (starts[:, :, None] + np.arange(block, dtype=np.int64)) % n
    return np.ascontiguousarray(idx.reshape(n_boot, n_blocks * block)[:, :n].astype(np.int32))


def tail_ppm_of(alpha: float) -> int:
    """the tail probability on each side of a 1 - alpha interval in parts per million (the ranks are integer arithmetic from there)"""
    ppm = int(round(float(alpha) * 0.5e6))
    if not 0 <= ppm < 500000:
        raise ValueError(f"alpha must lie in [0, 1), got {alpha}")
    return ppm


def p_value_from_counts(counts: np.ndarray) -> np.ndarray:
    """two-sided: min(1, 2 (min(n_le0, n_ge0) + 1) / (n_used + 1)); NaN where no replicate was used.  counts: (..., 4)"""
    counts = np.asarray(counts)
    n_used, n_le0, n_ge0 = (counts[..., i].astype(np.float64) for i in (1, 2, 3))
    p = np.minimum(1.0, 2.0 * (np.minimum(n_le0, n_ge0) + 1.0) / (n_used + 1.0))
    return np.where(n_used > 0, p, np.nan)


def result_dict(stats: np.ndarray, counts: np.ndarray, shape: Tuple[int, ...]) -> Dict[str, np.ndarray]:
    """(K, 8) stats and (K, 4) counts -> {field: array of `shape`} with `p_value`"""
    out = {f: np.ascontiguousarray(stats[:, i]).reshape(shape) for i, f in enumerate(STAT_FIELDS)}
    out.update({f: np.ascontiguousarray(counts[:, i]).reshape(shape) for i, f in enumerate(COUNT_FIELDS)})
    out["p_value"] = p_value_from_counts(counts).reshape(shape)
    return out


def paired_bootstrap(a, b, draws, kind: str = "mean", alpha: float = 0.05, max_workspace_bytes: int = DEFAULT_WORKSPACE_BYTES) -> Dict[str, np.ndarray]:
    """a, b: device tensors (N, ...) of the two runs' scores at N paired initial times (float64 is rounded to fp32); draws: (R, D) integers
    in [0, N), a host array or a device tensor.  -> host arrays of the shape of a[0]: the eight `STAT_FIELDS` (float64), the four
    `COUNT_FIELDS` (int32) and `p_value`.  kind: "mean" or "root_mean" (the square root of the mean: RMSE from `ens_mse`); the
    intervals are the alpha / 2 and 1 - alpha / 2 order statistics of the replicates.  The series axes are flattened and served in
    chunks whose workspace stays under `max_workspace_bytes`; a chunk is a column range of the same arrays (`ld`), never a copy."""
    import torch

    from .. import hip

    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    ppm = tail_ppm_of(alpha)
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda):
        raise RuntimeError("paired_bootstrap needs device tensors (no CPU fallback)")
    if a.shape != b.shape or a.dim() < 1 or a.numel() == 0:
        raise ValueError(f"a and b must have one non-empty shape (N, ...); got {tuple(a.shape)} and {tuple(b.shape)}")
    N, shape = int(a.shape[0]), tuple(a.shape[1:])
    a2, b2 = (t.to(torch.float32).reshape(N, -1).contiguous() for t in (a, b))
    K = int(a2.shape[1])
    draws_t = draws if isinstance(draws, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(draws))
    if draws_t.dim() != 2 or draws_t.numel() == 0 or draws_t.dtype.is_floating_point:
        raise ValueError(f"draws must be a non-empty (R, D) integer table, got {tuple(draws_t.shape)} {draws_t.dtype}")
    lo, hi = int(draws_t.min()), int(draws_t.max())
    if lo < 0 or hi >= N:
        raise ValueError(f"draws reach from {lo} to {hi}, outside the {N} initial times")
    R, D = int(draws_t.shape[0]), int(draws_t.shape[1])
    cap = int(hip.lib.ldc_paired_bootstrap_max_replicates())
    if R > cap:
        raise ValueError(f"{R} replicates: the kernel sorts at most {cap} per series")
    draws_d = draws_t.to(a2.device, torch.int32).contiguous()

    one = hip.paired_bootstrap_workspace_bytes(N, 1, R, D)
    per = hip.paired_bootstrap_workspace_bytes(N, 2, R, D) - one
    if one <= 0 or one > max_workspace_bytes:
        raise ValueError(f"one series of {N} initial times x {R} replicates needs a workspace of {one} bytes, the limit is {max_workspace_bytes}")
    chunk = min(K, 1 + (int(max_workspace_bytes) - one) // per)
    stats = torch.empty(K, 8, dtype=torch.float64, device=a2.device)
    counts = torch.empty(K, 4, dtype=torch.int32, device=a2.device)
    for k0 in range(0, K, chunk):
        kc = min(chunk, K - k0)
        hip.paired_bootstrap(a2[:, k0 : k0 + kc], b2[:, k0 : k0 + kc], draws_d, stats[k0 : k0 + kc], counts[k0 : k0 + kc], N=N, K=kc, ld=K, R=R, D=D,
                             kind=KINDS[kind], tail_ppm=ppm)
    return result_dict(stats.cpu().numpy(), counts.cpu().numpy(), shape)


# ---- score directories -------------------------------------------------------------------------------------------------------------
_TIME_FILE = re.compile(r"(\d{10})_crps\.npy")


def score_dir_times(path: str) -> List[int]:
    """The exact initial times (YYYYMMDDHH) of a score directory, ascending - the order of its stacked arrays - from the per-time files
    `YYYYMMDDHH_crps.npy` (`timestamp.npy` is fp32 and lossy, see `evaluate_ens_gpu.main`), cross-checked against `timestamp.npy` and
    the length of `crps.npy`."""
    times = sorted(int(m.group(1)) for m in (_TIME_FILE.fullmatch(f) for f in os.listdir(path)) if m)
    if not times:
        raise ValueError(f"{path}: no YYYYMMDDHH_crps.npy files")
    stamp = np.load(os.path.join(path, "timestamp.npy"))
    stacked = np.load(os.path.join(path, "crps.npy"), mmap_mode="r")
    if stamp.shape != (len(times),) or stacked.shape[0] != len(times):
        raise ValueError(f"{path}: {len(times)} per-time files, timestamp.npy holds {stamp.shape[0] if stamp.ndim else 1} and crps.npy {stacked.shape[0]} initial times")
    for i, t in enumerate(times):
        if np.float32(int(t)) != np.float32(stamp[i]):
            raise ValueError(f"{path}: initial time {i} is {t} by the per-time files and {float(stamp[i]):.0f} in timestamp.npy")
    return times


def pair_score_dirs(dir_a: str, dir_b: str):
    """-> (times, idx_a, idx_b, only_a, only_b): the common initial times ascending, their rows in the stacked arrays of either
    directory, and the times only one of them holds (not paired, reported)."""
    ta, tb = score_dir_times(dir_a), score_dir_times(dir_b)
    sa, sb = set(ta), set(tb)
    times = [t for t in ta if t in sb]
    pos_a, pos_b = {t: i for i, t in enumerate(ta)}, {t: i for i, t in enumerate(tb)}
    idx_a = np.array([pos_a[t] for t in times], dtype=np.int64)
    idx_b = np.array([pos_b[t] for t in times], dtype=np.int64)
    return times, idx_a, idx_b, [t for t in ta if t not in sb], [t for t in tb if t not in sa]


def _load_metric(path: str, name: str, n_times: int) -> np.ndarray:
    f = os.path.join(path, f"{name}.npy")
    if not os.path.exists(f):
        raise FileNotFoundError(f"metric {name!r}: {f} does not exist")
    x = np.load(f)
    if x.ndim != 3 or x.shape[0] != n_times:
        raise ValueError(f"metric {name!r}: {f} is {x.shape}, expected ({n_times}, C, L)")
    return x.astype(np.float32)  # float64 files are rounded to fp32 here


def verdict(diff_lo: float, diff_hi: float, higher_is_better: bool) -> str:
    """`better` / `worse` (B against A) when the interval of the difference excludes 0, `neutral` otherwise (an interval without a value too)"""
    if diff_lo > 0:
        return "better" if higher_is_better else "worse"
    if diff_hi < 0:
        return "worse" if higher_is_better else "better"
    return "neutral"


def _device_bootstrap(a, b, draws, kind, alpha):
    import torch

    return paired_bootstrap(torch.from_numpy(a).to("cuda"), torch.from_numpy(b).to("cuda"), draws, kind=kind, alpha=alpha)


def main(argv=None, bootstrap: Optional[Callable] = None):
    """`bootstrap(a, b, draws, kind, alpha) -> {field: (C, L) array}` (a, b: host fp32 arrays (N, C, L); the fields of `paired_bootstrap`)
    replaces the device (tests of the file handling).  Returns the dictionary written to `scorecard.npz`.

    Writes `scorecard.npz` ({metric}_{field}: (C, L) arrays for the eight stats, the four counts and p_value), `scorecard.json` (inputs,
    common and dropped initial times, n_boot, block, alpha, seed, the direction of every metric) and `scorecard.csv` (one row per metric,
    channel and `--leads` lead time: a, b, the relative change in % with its interval - from the ratio - p and the verdict)."""
    ap = argparse.ArgumentParser(description="Paired block-bootstrap comparison of two score directories of evaluate_ens_gpu")
    ap.add_argument("--a", type=str, required=True, help="score directory of run A (the baseline)")
    ap.add_argument("--b", type=str, required=True, help="score directory of run B")
    ap.add_argument("--output", type=str, required=True, help="directory for scorecard.npz / .json / .csv")
    ap.add_argument("--metrics", nargs="+", default=None, help="NAME of a NAME.npy (init time, C, L) present in both directories (default: the five reference scores both hold)")
    ap.add_argument("--rmse_of", nargs="+", default=[], help="also compare sqrt(mean M) as M_rmse (RMSE from ens_mse)")
    ap.add_argument("--n_boot", type=int, default=10000)
    ap.add_argument("--block", type=int, default=8, help="block length in initial times (1: the iid bootstrap)")
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--leads", type=int, nargs="+", default=None, help="lead times (1-based steps) of the .csv (default: all)")
    ap.add_argument("--channel_names_json", type=str, default=None, help="JSON list of channel names for the .csv")
    ap.add_argument("--higher_is_better", nargs="*", default=list(DEFAULT_HIGHER_IS_BETTER), help="metrics whose larger value is the better one")
    args = ap.parse_args(argv)

    times, idx_a, idx_b, only_a, only_b = pair_score_dirs(args.a, args.b)
    if not times:
        raise SystemExit(f"{args.a} and {args.b} share no initial time")
    n_a, n_b = len(idx_a) + len(only_a), len(idx_b) + len(only_b)
    names = args.metrics
    if names is None:
        names = [k for k in SCORE_NAMES if all(os.path.exists(os.path.join(d, f"{k}.npy")) for d in (args.a, args.b))]
        if not names:
            raise SystemExit("the directories share none of " + ", ".join(SCORE_NAMES))
    jobs = [(m, m, "mean") for m in names] + [(m, f"{m}_rmse", "root_mean") for m in args.rmse_of]
    if bootstrap is None:
        bootstrap = _device_bootstrap
    draws = block_bootstrap_draws(len(times), args.n_boot, args.block, args.seed)

    out, shapes = {}, {}
    for src, name, kind in jobs:
        xa, xb = _load_metric(args.a, src, n_a)[idx_a], _load_metric(args.b, src, n_b)[idx_b]
        if xa.shape != xb.shape:
            raise ValueError(f"metric {src!r}: {xa.shape[1:]} in {args.a} and {xb.shape[1:]} in {args.b}")
        res = bootstrap(np.ascontiguousarray(xa), np.ascontiguousarray(xb), draws, kind, args.alpha)
        shapes[name] = xa.shape[1:]
        for f in STAT_FIELDS + COUNT_FIELDS + ("p_value",):
            arr = np.asarray(res[f])
            if arr.shape != xa.shape[1:]:
                raise ValueError(f"{name}: {f} is {arr.shape}, expected {xa.shape[1:]}")
            out[f"{name}_{f}"] = arr

    os.makedirs(args.output, exist_ok=True)
    np.savez(os.path.join(args.output, "scorecard.npz"), **out)
    higher = set(args.higher_is_better)
    direction = {name: "higher_is_better" if (name in higher or src in higher) else "lower_is_better" for src, name, _ in jobs}
    meta = dict(a=os.path.abspath(args.a), b=os.path.abspath(args.b), metrics=[name for _, name, _ in jobs], kinds={name: kind for _, name, kind in jobs},
                n_boot=args.n_boot, block=args.block, alpha=args.alpha, seed=args.seed, n_common=len(times), common_times=[int(t) for t in times],
                only_a=[int(t) for t in only_a], only_b=[int(t) for t in only_b], direction=direction,
                note="blocks are runs of consecutive available common initial times (gaps ignored); float64 scores are rounded to fp32")
    with open(os.path.join(args.output, "scorecard.json"), "w") as f:
        json.dump(meta, f, indent=1)

    channel_names = None
    if args.channel_names_json:
        with open(args.channel_names_json) as f:
            channel_names = [str(c) for c in json.load(f)]
    with open(os.path.join(args.output, "scorecard.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["metric", "channel", "lead", "a", "b", "change_pct", "change_lo_pct", "change_hi_pct", "p_value", "verdict"])
        for _, name, _ in jobs:
            C, L = shapes[name]
            leads = list(range(1, L + 1)) if args.leads is None else args.leads
            if any(not 1 <= l <= L for l in leads):
                raise ValueError(f"--leads {leads}: {name} holds lead times 1 .. {L}")
            if channel_names is not None and len(channel_names) < C:
                raise ValueError(f"--channel_names_json names {len(channel_names)} channels, {name} holds {C}")
            g = {fld: out[f"{name}_{fld}"] for fld in STAT_FIELDS + ("p_value",)}
            for c in range(C):
                for l in leads:
                    i = (c, l - 1)
                    pct = [100.0 * (float(g[fld][i]) - 1.0) for fld in ("ratio_hat", "ratio_lo", "ratio_hi")]
                    w.writerow([name, channel_names[c] if channel_names else c, l, repr(float(g["a_hat"][i])), repr(float(g["b_hat"][i]))]
                               + [f"{v:.6g}" for v in pct]
                               + [f"{float(g['p_value'][i]):.6g}", verdict(float(g["diff_lo"][i]), float(g["diff_hi"][i]), direction[name] == "higher_is_better")])
    print(f"scorecard: {len(jobs)} metrics x {len(times)} common initial times ({len(only_a)} only in a, {len(only_b)} only in b), "
          f"{args.n_boot} replicates in blocks of {args.block} -> {args.output}")
    return out


if __name__ == "__main__":
    main()
