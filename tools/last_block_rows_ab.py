"""A/B of `LaDCastTransformer3DModel.skip_unread_rows` (the last single-stream block on the pred rows only) inside ONE build.

  python tools/last_block_rows_ab.py run {all|pred} [bench.py arguments]
      bench.py, unchanged, with the switch off (`all`: every row, what the parent commit computes) or on (`pred`: as shipped)
  python tools/last_block_rows_ab.py summarize DIR OUT.json
      DIR holds what the runs left: bench_A<i>.log / bench_B<i>.log (stdout of `run all` / `run pred`, alternated A B A B A B),
      dump_A/ dump_B/ (--dump-outputs of one run per side) and prof_A/ prof_B/ (rocprofv3 --kernel-trace --stats --output-format csv
      of one short run per side).  Writes ms_per_step and value of every run, the rel-L2 between the two dumps against the fp32
      per-chunk band, launches per forward and the summed GEMM / attention kernel time per step of both sides, and the verdict:
      every B run faster than every A run, medians apart by at least half of the predicted 6.7 ms."""
import csv
import glob
import json
import os
import runpy
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREDICTED_MS = 6.7
FORWARDS_PER_STEP = 39  # 20-step Heun chunk


def run(side, argv):
    sys.path.insert(0, ROOT)
    from ladcast_amd.models import LaDCastTransformer3DModel

    LaDCastTransformer3DModel.skip_unread_rows = {"all": False, "pred": True}[side]
    sys.argv = [os.path.join(ROOT, "bench.py")] + argv
    runpy.run_path(sys.argv[0], run_name="__main__")


def _bench_line(path):
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
    return json.loads(lines[-1])


def _profile(d):
    """kernel trace of one run -> launches per forward (dispatches of the last forward: chan_to_token .. token_to_chan) and GEMM /
    attention kernel time per step (per-forward average over the whole run x the step's forwards)"""
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        return None
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    ends = [i for i, n in enumerate(names) if "token_to_chan" in n]
    starts = [i for i, n in enumerate(names) if "chan_to_token" in n and i < ends[-1]]
    # the sample's transpose opens a forward's sample-dependent part (the conditioning path has one of its own, batched per chunk)
    last_forward = ends[-1] - starts[-1] + 1
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6  # noqa: E731
    n_fwd = len(ends)
    gemm = sum(dur(r) for r in rows if "gemm" in r["Kernel_Name"])
    attn = sum(dur(r) for r in rows if "attn_fwd" in r["Kernel_Name"] or "attn_tail_merge" in r["Kernel_Name"])
    per_kernel = {}
    for r in rows[starts[-1] : ends[-1] + 1]:
        k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:60]
        per_kernel[k] = per_kernel.get(k, 0) + 1
    return dict(trace=os.path.relpath(f[0], d), forwards=n_fwd, dispatches=len(rows), dispatches_per_forward_whole_run=round(len(rows) / n_fwd, 3),
                launches_last_forward=last_forward, launches_last_forward_by_kernel=per_kernel,
                gemm_ms_per_step=round(gemm / n_fwd * FORWARDS_PER_STEP, 3), attention_ms_per_step=round(attn / n_fwd * FORWARDS_PER_STEP, 3))


def summarize(d, out):
    import numpy as np

    sys.path.insert(0, ROOT)
    from tests.precision_bands import ceiling

    res = {"what": "skip_unread_rows A/B in one build: A = every row (the parent commit's launches), B = last single block on the pred rows only",
           "command": "python bench.py --gpus 1 --steps 20 --warmup 3, alternated A B A B A B", "predicted_saving_ms": PREDICTED_MS, "runs": []}
    for side in "AB":
        for p in sorted(glob.glob(os.path.join(d, f"bench_{side}*.log"))):
            ln = _bench_line(p)
            res["runs"].append(dict(run=os.path.basename(p)[6:-4], side=side, ms_per_step=ln["ms_per_step"], value=ln["value"]))
    a = [r["ms_per_step"] for r in res["runs"] if r["side"] == "A"]
    b = [r["ms_per_step"] for r in res["runs"] if r["side"] == "B"]
    res["median_ms_per_step"] = dict(A=statistics.median(a), B=statistics.median(b))
    res["median_saving_ms"] = round(statistics.median(a) - statistics.median(b), 3)
    res["every_B_faster_than_every_A"] = max(b) < min(a)
    res["passes"] = bool(res["every_B_faster_than_every_A"] and res["median_saving_ms"] >= PREDICTED_MS / 2)
    fa, fb = (glob.glob(os.path.join(d, f"dump_{s}", "*.npy")) for s in "AB")
    if fa and fb:
        xa, xb = np.load(fa[0]).astype(np.float64), np.load(fb[0]).astype(np.float64)
        rel = float(np.linalg.norm(xa - xb) / np.linalg.norm(xa))
        band = ceiling("chunk_375m_edm")
        res["outputs"] = dict(rel_l2_B_vs_A=rel, fp32_per_chunk_band=band, band_stage="chunk_375m_edm (tests/precision_bands.py)", inside_band=rel < band)
    res["kernel_profile"] = {s: _profile(os.path.join(d, f"prof_{s}")) for s in "AB"}
    pa, pb = res["kernel_profile"]["A"], res["kernel_profile"]["B"]
    if pa and pb:
        res["launches_per_forward_unchanged"] = pa["launches_last_forward"] == pb["launches_last_forward"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_profile"}, indent=1))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run" and sys.argv[2] in ("all", "pred"):
        run(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
