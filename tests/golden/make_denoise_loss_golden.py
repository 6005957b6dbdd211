"""Regenerate tests/golden/denoise_loss_ref.npz from the reference's OWN training objective (needs the reference tree; not run by the tests).

    python tests/golden/make_denoise_loss_golden.py [REFERENCE_ROOT]     (default: the reference checkout make_golden.py reads)

ladcast/train_AR.py imports accelerate, diffusers, wandb and xarray, which this tree does not have, so its statements are compiled from
the syntax tree, at generation time only: the body of the training loop from `noise = torch.randn(...)` down to the statement that assigns
`loss = torch.mean(...)`, the block that builds `loss_lat_weight`, and the functions they call - `get_sigmas` (ladcast/pipelines/utils.py),
`Karras_sigmas_lognormal` (ladcast/models/utils.py), `get_normalized_lat_weights_based_on_cos` (ladcast/evaluate/utils.py),
`convert_datetime_to_int` (ladcast/dataloader/ar_dataloder.py) and `convert_int_to_datetime` (ladcast/models/embeddings.py).  They run on
the CPU with the oracle's scheduler as `noise_scheduler`, the oracle's tiny AR model as `ar_model` and the small stand-ins below for
`accelerator`, `general_config`, `args` and the two config objects; the inputs come from seeds (tests/denoise_synth.py).

Every case of `denoise_synth.cases()` (sigma indices at both ends of the schedule / one level for the batch, 1 and 2 push-forward steps,
latitude weighting on and off, epsilon and v_prediction) gives `loss_<case>` (the reference's fp32 scalar), `loss64_<case>` (the float64
mean of the reference's fp32 terms) and the raw network output `model_pred` (full for the case without push-forward at the schedule ends,
every 97th value otherwise).  Also: `sigmas_<set>`, every 97th value of `noisy_images` / `x_in` per index set, and the indices the
reference's noise sampler draws for a fixed seed at two values of `cur_step`."""
import ast
import os
import sys
from datetime import datetime
from types import SimpleNamespace

import numpy as np
import pandas as pd
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.scheduler import EDMDPMSolverMultistepScheduler  # noqa: E402
from tests import denoise_synth as DS  # noqa: E402
from tests.synth import Sub, make_ar, oracle_threads, tiny_ar_config  # noqa: E402

REF = os.path.join(sys.argv[1] if len(sys.argv) > 1 else "/root/reference", "ladcast")


def parse(*rel):
    return ast.parse(open(os.path.join(REF, *rel)).read())


def definitions_of(tree, names):
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in body} == set(names), names
    return body


def is_attr(node, base, attr):
    return isinstance(node, ast.Attribute) and node.attr == attr and isinstance(node.value, ast.Name) and node.value.id == base


def objective_statements(tree):
    """(the `if args.lat_weighted_loss:` block that builds loss_lat_weight, the loop-body statements of one iteration)"""
    lat_block = [n for n in ast.walk(tree) if isinstance(n, ast.If) and is_attr(n.test, "args", "lat_weighted_loss")
                 and any(isinstance(s, ast.Assign) and getattr(s.targets[0], "id", None) == "loss_lat_weight" for s in n.body)]
    loops = [n for n in ast.walk(tree) if isinstance(n, ast.With) and isinstance(n.items[0].context_expr, ast.Call)
             and is_attr(n.items[0].context_expr.func, "accelerator", "accumulate")]
    assert len(lat_block) == 1 and len(loops) == 1
    body = loops[0].body
    first = next(i for i, s in enumerate(body) if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", None) == "noise")
    last = next(i for i, s in enumerate(body) if isinstance(s, ast.If) and isinstance(s.test, ast.Compare) and is_attr(s.test.left, "general_config", "snr_gamma"))
    assert "loss" in {getattr(t, "id", None) for s in ast.walk(body[last]) if isinstance(s, ast.Assign) for t in s.targets}
    return lat_block[0], body[first : last + 1]


def compiled(nodes):
    mod = ast.Module(body=[ast.ImportFrom(module="__future__", names=[ast.alias(name="annotations")], level=0)] + list(nodes), type_ignores=[])
    return compile(ast.fix_missing_locations(mod), REF, "exec")


# ---- stand-ins ----------------------------------------------------------------------------------------------------------------------------
class Accelerator:
    device = torch.device("cpu")

    def gather(self, t):
        return t

    def log(self, values, step=None):
        pass


class RecordingModel:
    """the oracle model, remembering every raw output"""

    def __init__(self, model):
        self.model, self.outputs = model, []

    def __call__(self, *a, **kw):
        out = self.model(*a, **kw)
        self.outputs.append(out[0].clone())
        return out


def main():
    train = parse("train_AR.py")
    lat_block, loop_body = objective_statements(train)
    helpers = (definitions_of(parse("pipelines", "utils.py"), {"get_sigmas"}) + definitions_of(parse("models", "utils.py"), {"Karras_sigmas_lognormal"})
               + definitions_of(parse("evaluate", "utils.py"), {"get_normalized_lat_weights_based_on_cos"})
               + definitions_of(parse("dataloader", "ar_dataloder.py"), {"convert_datetime_to_int"})
               + definitions_of(parse("models", "embeddings.py"), {"convert_int_to_datetime"}))
    base = {"np": np, "pd": pd, "torch": torch, "F": F, "datetime": datetime, "Union": None, "Optional": None}
    exec(compiled(helpers), base)
    setup_code, body_code = compiled([lat_block]), compiled(loop_body)

    out = {}
    # the noise sampler on the training schedule
    sched = EDMDPMSolverMultistepScheduler()
    sampler = base["Karras_sigmas_lognormal"](sched.sigmas)
    for cur_step in DS.SAMPLER_STEPS:
        idx = sampler(DS.SAMPLER_BATCH, cur_step=cur_step, generator=torch.Generator().manual_seed(DS.SAMPLER_SEED), device="cpu")
        out[f"sampler_indices_{cur_step}"] = idx.numpy().astype(np.int64)

    oracle = make_ar(tiny_ar_config())
    for key, name, k, lat, pred in DS.cases():
        model = RecordingModel(oracle)
        indices = torch.tensor(DS.INDEX_SETS[name])
        ns = dict(base)
        ns.update(
            accelerator=Accelerator(), general_config=SimpleNamespace(do_edm_style_training=True, snr_gamma=None),
            args=SimpleNamespace(num_push_forward_steps=k, lat_weighted_loss=lat),
            noise_scheduler=EDMDPMSolverMultistepScheduler(prediction_type=pred),
            noise_scheduler_config=SimpleNamespace(target="diffusers.EDMDPMSolverMultistepScheduler"),
            train_dataloader_config=SimpleNamespace(input_seq_len=DS.T_IN, return_seq_len=DS.T),
            num_slice_per_push_forward=int(DS.T / k), noise_sampler=lambda bs, cur_step, generator, device: indices.clone(),
            noise_sampler_gen=None, global_step=0, ar_model=model,
            initial_profile=DS.initial_profile(), clean_images=DS.clean_images(), timestamps=DS.timestamps(),
        )
        with torch.no_grad(), oracle_threads():
            exec(setup_code, ns)
            torch.manual_seed(DS.NOISE_SEED)
            exec(body_code, ns)
        assert torch.equal(ns["noise"], DS.noise()) and torch.equal(ns["indices"], indices)
        w = ns["weighting"].float() if not lat else ns["loss_lat_weight"].float() * ns["weighting"].float()
        terms = w * (ns["model_pred"].float() - ns["target"].float()) ** 2  # the fp32 terms the reference averages
        assert terms.dtype == torch.float32 and torch.equal(torch.mean(terms), ns["loss"]), key
        out[f"loss_{key}"] = ns["loss"].numpy().astype(np.float32)
        out[f"loss64_{key}"] = terms.double().mean().numpy()
        raw = torch.cat(model.outputs, dim=2)
        assert raw.shape == ns["clean_images"].shape and len(model.outputs) == k
        mkey = DS.model_pred_key(name, k, pred)
        if name == "ends" and k == 1:
            out[mkey] = raw.numpy()
        else:
            s = Sub.of(raw, DS.SUB_STRIDE)
            out[mkey + "__sub"], out[mkey + "__meta"] = s.values.numpy(), np.array([s.stride, s.norm, *s.shape], dtype=np.float64)
        sig = ns["sigmas"].reshape(-1)
        if f"sigmas_{name}" in out:
            assert np.array_equal(out[f"sigmas_{name}"], sig.numpy())
        out[f"sigmas_{name}"] = sig.numpy()
        for what in ("noisy_images", "x_in"):
            out[f"{what}_{name}"] = ns[what].contiguous().flatten()[:: DS.SUB_STRIDE].numpy()
        if k > 1:
            out[f"timestamps_after_{key}"] = ns["timestamps"].numpy().astype(np.int64)
        print(f"{key}: loss {float(ns['loss']):.9g}  float64 {float(out[f'loss64_{key}']):.17g}")
    assert all(np.isfinite(v).all() for v in out.values())
    path = os.path.join(HERE, "denoise_loss_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} KB, {len(out)} arrays")


if __name__ == "__main__":
    main()
