"""Regenerate tests/golden/validation_ref.npz from the reference's OWN validation hook (needs the reference tree; not run by the tests).

    python tests/golden/make_validation_golden.py [REFERENCE_ROOT]     (default: the reference checkout make_golden.py reads)

`log_validation` is compiled from the syntax tree of ladcast/train_AR.py (the module imports accelerate, diffusers, wandb and xarray, which
this tree does not have), together with the functions it calls: `get_crps`, `pointwise_crps_skill`, `pointwise_crps_spread` and
`get_normalized_lat_weights_based_on_cos` (ladcast/evaluate/utils.py), `inverse_normalize_transform_3D` (ladcast/dataloader/utils.py) and
`convert_datetime_to_int` (ladcast/dataloader/ar_dataloder.py).  It runs on the CPU over the stand-ins of tests/validation_synth.py (latent
store, recording chunk sampler, decoder: IEEE-exact elementwise operations) and the small stand-ins below for what it touches of xarray,
accelerate and the pipeline.  C = 84 on 120 x 240 (hard-wired in the reference), 3 members, 4 lead times in chunks of 2, two initial times,
eval_ms, eval_crps.

The tables are taken from the hook's wandb path (train_AR.py:360-371: `wandb.Table(data=[[lead time, *row], ...], columns=[...])` handed to
`tracker.log`), recorded by a tracker stand-in named "wandb".  Its `return_df=True` path cannot be used: `create_pd_dataframe` (:95-108) is
given the column list that already starts with "lead time" and indexes the value rows with it, one column too many - an IndexError for
every input.  `ladcast_amd.evaluate.log_validation` returns DataFrames with the wandb tables' layout.

The fixture holds both tables' values and column names and the recorded (sampler_type, timestamp) call sequence: a few KB of data."""
import ast
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pandas as pd
import torch
from einops import rearrange

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import validation_synth as VS  # noqa: E402

REF = os.path.join(sys.argv[1] if len(sys.argv) > 1 else "/root/reference", "ladcast")


# ---- stand-ins for what log_validation touches of xarray, accelerate and the pipeline -------------------------------------------------
class LatentsArray:
    """`ds["latents"]`: `.sel(time=list | slice).values` over a pandas time index (label-based: a slice includes both ends)"""

    def __init__(self, values, index):
        self.values, self.index = values, index

    def sel(self, time):
        if isinstance(time, slice):
            rows = self.index.slice_indexer(time.start, time.stop)
        else:
            rows = self.index.get_indexer(list(time))
            assert (rows >= 0).all(), time
        return LatentsArray(self.values[rows], self.index[rows])


class Table:
    """wandb.Table(data=, columns=)"""

    def __init__(self, data, columns):
        self.data, self.columns = data, columns


class Tracker:
    name = "wandb"

    def __init__(self):
        self.logged = []

    def log(self, tables):
        self.logged.append(tables)


class Accelerator:
    device = torch.device("cpu")
    process_index = 0

    def __init__(self):
        self.trackers = [Tracker()]

    def gather(self, t):
        return t


class Pipeline:
    def __init__(self, ar_model, scheduler=None):
        self.ar_model, self.scheduler = ar_model, scheduler

    @property
    def _execution_device(self):
        return torch.device("cpu")


def functions_of(path, names):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names), (path, names)
    return body


def reference_log_validation(sampler):
    ns = {"np": np, "pd": pd, "torch": torch, "math": math, "rearrange": rearrange, "Optional": None, "Union": None,
          "xr": SimpleNamespace(Dataset=None), "accelerate": SimpleNamespace(Accelerator=None), "wandb": SimpleNamespace(Table=Table),
          "instantiate_from_config": lambda cfg: cfg, "AutoRegressive2DPipeline": Pipeline, "ensemble_AR_sampler": sampler}
    body = functions_of(os.path.join(REF, "evaluate", "utils.py"),
                        {"get_crps", "pointwise_crps_skill", "pointwise_crps_spread", "get_normalized_lat_weights_based_on_cos"})
    body += functions_of(os.path.join(REF, "dataloader", "utils.py"), {"inverse_normalize_transform_3D"})
    body += functions_of(os.path.join(REF, "dataloader", "ar_dataloder.py"), {"convert_datetime_to_int"})
    body += functions_of(os.path.join(REF, "train_AR.py"), {"log_validation"})
    src = ast.Module(body=[ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)] + body, type_ignores=[])
    exec(compile(ast.fix_missing_locations(src), REF, "exec"), ns)
    return ns["log_validation"]


def main():
    sampler = VS.RecordingSampler()
    log_validation = reference_log_validation(sampler)
    index = pd.DatetimeIndex([VS.START + pd.Timedelta(hours=VS.STEP_HOURS * i) for i in range(VS.N_FRAMES)])
    ds = {"latents": LatentsArray(VS.latent_frames().numpy(), index)}
    mean, std = VS.field_statistics()
    acc = Accelerator()
    log_validation(
        "validation", ds, SimpleNamespace(channel_names=VS.CHANNEL_NAMES), None, mean, std, VS.T_IN, VS.R, VS.UpsampleDecoder(),
        VS.latent_transform, VS.latent_inv_transform, None, acc, [pd.Timestamp(t) for t in VS.INIT_TIMES],
        step_size_hour=VS.STEP_HOURS, total_lead_time_hour=VS.T * VS.STEP_HOURS, ensemble_size=VS.ENS, num_inference_steps=VS.INFERENCE_STEPS,
        eval_ms=True, eval_crps=True, return_df=False)
    (logged,) = acc.trackers[0].logged
    rmse, crps = logged["merged_RMSE"], logged["CRPS"]
    out = {
        "rmse_columns": np.array(list(rmse.columns)), "rmse_values": np.array(rmse.data, dtype=np.float64),
        "crps_columns": np.array(list(crps.columns)), "crps_values": np.array(crps.data, dtype=np.float64),
        "call_sampler_type": np.array([c[0] for c in sampler.calls]), "call_timestamp": np.array([c[1] for c in sampler.calls], dtype=np.int64),
    }
    assert np.isfinite(out["rmse_values"]).all() and np.isfinite(out["crps_values"]).all()
    path = os.path.join(HERE, "validation_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} KB, rmse {out['rmse_values'].shape}, crps {out['crps_values'].shape}, "
          f"{len(sampler.calls)} sampler calls: {sampler.calls}")


if __name__ == "__main__":
    main()
