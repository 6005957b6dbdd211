"""Regenerate tests/golden/recon_ref.npz from the reference's OWN code (needs the reference tree; not run by the tests).

    python tests/golden/make_recon_golden.py REFERENCE_ROOT

`ladcast.metric.loss` (LpLoss) and `ladcast.metric.utils` (process_tensor_for_loss, remove_channel) are imported from the reference;
`weather_dataset_preprocess_batch` is compiled from the syntax tree of ladcast/dataloader/weather_dataset.py (the module imports
`datasets`, which this tree does not have).  The un-normalise / mse_loss / latitude-weighted mean lines are those of
ladcast/evaluate/evaluate_encdec_model.py:211-231, on one process (accelerator.gather is the identity there).

The seeded inputs come from tests/recon_oracle.py.  The fixture holds the inputs of the small cases and the reference's outputs of
all; the two larger score cases ("chunks", "full") are regenerated from their seed by the tests and carry a checksum instead.

Ingredients of every score case (tests/recon_oracle.py::score_inputs): channel 0 with mean 2e5 / std 3e3 and a reconstruction error
~1e-2; channel 1 an all-zero target (zero prediction too in all but the last batch element: NaN there, inf in the last); SST
(channel 2) masked at ~30 % of the points and at every point of batch element 0.  Where the shape cannot hold all of it: C = 2
("point") has no third channel, so nothing is masked; B = 1 cases have no second batch element, so "odd" is masked at ~30 % only and
"point_all" - a single point with every ingredient, added to the table of shapes - is fully masked.

Two checks made here, printed, and quoted in tests/test_gpu_recon.py:
* the shortcut sigma^2 (p - t)^2 w differs from the reference's lw_mse in the geopotential channel of both single-point cases, so
  the bit-exactness test can fail;
* the reference's fp32 outputs lie within the 1e-5 `_close` bound of a float64 summation of the same fp32 point values.
"""
import ast
import os
import sys
from typing import Optional  # noqa: F401  (the compiled function's annotations)

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2:
    raise SystemExit(__doc__.split("\n\n")[1])
REF_ROOT = sys.argv[1]
sys.path.insert(0, ROOT)
sys.path.insert(0, REF_ROOT)

from ladcast.metric.loss import LpLoss  # noqa: E402
from ladcast.metric.utils import process_tensor_for_loss, remove_channel  # noqa: E402

from tests import recon_oracle as RO  # noqa: E402


def reference_preprocess():
    path = os.path.join(REF_ROOT, "ladcast", "dataloader", "weather_dataset.py")
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "weather_dataset_preprocess_batch"]
    assert len(body) == 1
    ns = {"torch": torch, "Optional": Optional}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns["weather_dataset_preprocess_batch"]


def main():
    torch.set_num_threads(1)  # one summation order for the fixture
    out = {}
    pre = reference_preprocess()
    for i, shape in enumerate(RO.PRE_SHAPES):
        x, mean, std = RO.pre_inputs(shape, seed=100 + i)
        out[f"pre{i}_x"], out[f"pre{i}_mean"], out[f"pre{i}_std"] = x.numpy(), mean.numpy(), std.numpy()
        for crop in (0, 1):
            for keep in (0, 1):
                C = shape[1] - (0 if keep else 1)
                y, mask = pre(x.clone(), mean[:C, None, None], std[:C, None, None], crop_south_pole=bool(crop), sst_channel_idx=RO.PRE_SST,
                              incl_sur_pressure=bool(keep))
                out[f"pre{i}_c{crop}k{keep}_y"], out[f"pre{i}_c{crop}k{keep}_mask"] = y.numpy(), mask.numpy()
                yo, mo = RO.preprocess(x, mean[:C], std[:C], bool(crop), RO.PRE_SST, bool(keep))
                assert torch.equal(torch.nan_to_num(yo), torch.nan_to_num(y)) and torch.equal(mo, mask)
        print(f"preprocess {shape}: masks hold {[int(out[f'pre{i}_c0k1_mask'][b].sum()) for b in range(shape[0])]} NaNs per batch element")

    worst_all = 0.0
    for name, case in RO.SCORE_CASES.items():
        d = RO.score_inputs(name)
        B, C, S, H, W, Bs = case["shape"]
        w4 = d["w"].view(1, 1, -1, 1)
        pred, tgt = process_tensor_for_loss(d["pred"], d["target"], d["mask"], sst_chanel_idx=d["sst"])
        if S:
            tgt = torch.cat([tgt, d["static"].expand(B, -1, -1, -1)], dim=1)
        rel = LpLoss(d=2, p=2, reduce_dims=None).rel(pred, tgt, weight=w4)
        absn = LpLoss(d=2, p=2, reduce_dims=None).abs(pred, tgt, weight=w4)
        loss_fn = LpLoss(d=2, p=2, reduce_dims=[0, 1], reductions="mean")
        loss = loss_fn(pred, tgt, weight=w4)
        loss_finite = loss_fn(remove_channel(pred, RO.ZERO), remove_channel(tgt, RO.ZERO), weight=w4)
        proc_mean, proc_std = d["mean"][:, None, None], d["std"][:, None, None]
        mse_map = torch.nn.functional.mse_loss(pred * proc_std + proc_mean, tgt * proc_std + proc_mean, reduction="none")
        lw = (mse_map * w4).mean(dim=[0, 2, 3])
        out[f"{name}_rel"], out[f"{name}_abs"], out[f"{name}_lw"] = rel.numpy(), absn.numpy(), lw.numpy()
        out[f"{name}_loss"], out[f"{name}_loss_finite"] = loss.numpy(), loss_finite.numpy()
        out[f"{name}_checksum"] = RO.checksum(d).numpy()
        if case["stored"]:
            for k in ("pred", "target", "mask", "w", "mean", "std"):
                out[f"{name}_{k}"] = d[k].numpy()
            if S:
                out[f"{name}_static"] = d["static"].numpy()
        # float64 sums of the same fp32 point values: the distance the 1e-5 bound has to cover
        r64, a64, l64 = RO.scores(d["pred"], d["target"], d["static"], d["mask"], d["sst"], d["w"], d["mean"], d["std"])
        dist = max(RO.close(rel, r64, 1e-5, name), RO.close(absn, a64, 1e-5, name), RO.close(lw, l64, 1e-5, name))
        worst_all = max(worst_all, dist)
        print(f"{name} {case['shape']}: reference fp32 vs float64 sums: {dist:.2e} of the _close scale; rel[:, :3] = {rel[:, :3].tolist()}; "
              f"loss = {float(loss)}, loss_finite = {float(loss_finite):.6g}")
        if H * W * B == 1:
            short = (d["std"] * d["std"]) * ((pred - tgt) * (pred - tgt)).flatten() * d["w"][0]
            assert float(lw[RO.GEO]) == float(l64[RO.GEO].float()), "single point: the restatement is bit-equal"
            assert float(short[RO.GEO]) != float(lw[RO.GEO]), f"{name}: the sigma^2 shortcut equals the reference here, pick another seed"
            print(f"  single point, geopotential channel: reference lw_mse {float(lw[RO.GEO])!r}, sigma^2 shortcut {float(short[RO.GEO])!r}")
    print(f"largest distance reference fp32 <-> float64 sums over all cases: {worst_all:.2e} (bound 1e-5)")
    path = os.path.join(HERE, "recon_ref.npz")
    np.savez(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
