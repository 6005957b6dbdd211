"""`ladcast_amd.evaluate.denoise_loss` end to end on the tiny AR model (B = 2) against tests/golden/denoise_loss_ref.npz: what the
reference's own training-loop statements gave on the CPU oracle (tests/golden/make_denoise_loss_golden.py).

Tolerances: `model_pred` within `precision.tolerance(mode, "forward")` rel-L2 of the oracle's; `loss` within
`precision.tolerance(mode, "denoise_loss")` of the reference's fp32 loss - a bound DERIVED from the forward tolerance and the reference's
own numbers (ladcast_amd/precision.py::DENOISE_LOSS_FACTOR), inside the 1e-4 budget for fp32 / bf16x3.  The test prints what it measures,
per case and per mode, before it asserts."""
import csv
import os
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ladcast_amd import precision  # noqa: E402
from tests import denoise_synth as DS  # noqa: E402
from tests.synth import load_fullsize_golden, make_ar, rel_l2, tiny_ar_config  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.fixture(scope="module")
def ref():
    return load_fullsize_golden(os.path.join(ROOT, "tests", "golden", "denoise_loss_ref.npz"))


@pytest.fixture(scope="module")
def model():
    from ladcast_amd.models import LaDCastTransformer3DModel

    cfg = tiny_ar_config()
    m = LaDCastTransformer3DModel.from_config(cfg)
    m.load_state_dict(make_ar(cfg).state_dict(), strict=True)
    return m.to("cuda:0").eval()


def scheduler(pred="epsilon"):
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    return EDMDPMSolverMultistepScheduler(prediction_type=pred)


def run_case(model, name, k, lat, pred):
    from ladcast_amd.evaluate.denoise_loss import denoising_loss

    return denoising_loss(model, scheduler(pred), DS.initial_profile().cuda(), DS.clean_images().cuda(), DS.timestamps(), indices=DS.INDEX_SETS[name],
                          noise=DS.noise().cuda(), num_push_forward_steps=k, input_seq_len=DS.T_IN, lat_weighted_loss=lat)


@pytest.fixture(scope="module", params=precision.MODES)
def results(request, model):
    """every fixture case in one GEMM precision mode, computed once"""
    model.set_gemm_precision(request.param)
    out = {key: run_case(model, name, k, lat, pred) for key, name, k, lat, pred in DS.cases()}
    torch.cuda.synchronize()
    return request.param, out


def test_noisy_and_x_in_are_bit_equal(results, ref):
    mode, out = results  # the noising arithmetic is fp32 whatever the GEMM mode: bit-equal in all three
    for key, name, k, lat, pred in DS.cases():
        o = out[key]
        for what in ("noisy_images", "x_in"):
            got = getattr(o, what).cpu().flatten()[:: DS.SUB_STRIDE]
            assert torch.equal(got, ref[f"{what}_{name}"]), (key, what)
        assert torch.equal(o.sigmas, ref[f"sigmas_{name}"]) and o.indices.tolist() == list(DS.INDEX_SETS[name])
        assert o.table.shape == (DS.B, DS.C, DS.T) and o.per_sample.shape == (DS.B,) and o.loss.dim() == 0 and o.loss.is_cuda
        assert float(o.loss) == float(o.table.double().mean().float())


@pytest.mark.parametrize("lat", [False, True])
@pytest.mark.parametrize("pred", DS.PREDICTION_TYPES)
def test_oracle_model_pred_through_the_loss_path(ref, lat, pred):
    """the loss path alone: the ORACLE's network output through precondition_outputs and the loss kernel"""
    import ladcast_amd.hip as hip
    from ladcast_amd.evaluate.denoise_loss import loss_latitude_weights
    from ladcast_amd.pipelines.utils import get_sigmas

    key = f"ends_k1_lat{int(lat)}_{pred}"
    s = scheduler(pred)
    clean, F = DS.clean_images().cuda(), ref[DS.model_pred_key("ends", 1, pred)].cuda()
    ts = s.timesteps[list(DS.INDEX_SETS["ends"])]
    noisy = s.add_noise(clean, DS.noise().cuda(), ts)
    sigmas = get_sigmas(s, ts, 5)
    denoised = s.precondition_outputs(noisy, F, sigmas)
    _, c_skip, c_out, weight = (v.cuda() for v in s.edm_coefficients(sigmas))
    table, den2 = torch.empty(DS.B, DS.C, DS.T, device="cuda"), torch.empty_like(clean)
    hip.edm_denoise_loss(noisy, F, clean, c_skip, c_out, weight, table, lat_weight=loss_latitude_weights(DS.H).cuda() if lat else None, denoised=den2)
    assert torch.equal(den2, denoised)
    loss = float(table.double().mean().float())
    ref32, ref64 = float(ref[f"loss_{key}"]), float(ref[f"loss64_{key}"])
    print(f"{key}: loss {loss!r}  reference fp32 {ref32!r}  float64 {ref64!r}  -> {abs(loss - ref64) / ulp32(ref64):.3f} ulp from float64 "
          f"(the reference's fp32 mean: {abs(ref32 - ref64) / ulp32(ref64):.3f} ulp)")
    assert abs(loss - ref64) <= ulp32(ref64)
    assert abs(loss - ref32) <= abs(ref32 - ref64) + ulp32(ref64)


def test_every_case_end_to_end(results, ref):
    mode, out = results
    worst_pred, worst_loss = 0.0, 0.0
    for key, name, k, lat, pred in DS.cases():
        o = out[key]
        e_pred = rel_l2(o.model_pred.cpu(), ref[DS.model_pred_key(name, k, pred)])
        ref32 = float(ref[f"loss_{key}"])
        e_loss = abs(float(o.loss) - ref32) / abs(ref32)
        print(f"denoise_loss[{mode}] {key}: model_pred rel-L2 {e_pred:.3e}  loss {float(o.loss)!r} vs {ref32!r}: rel {e_loss:.3e}")
        worst_pred, worst_loss = max(worst_pred, e_pred), max(worst_loss, e_loss)
    print(f"denoise_loss[{mode}] worst: model_pred rel-L2 {worst_pred:.3e}, loss rel {worst_loss:.3e}")
    assert worst_pred < precision.tolerance(mode, "forward")
    if mode in ("fp32", "bf16x3"):
        assert precision.tolerance(mode, "denoise_loss") <= 1e-4  # the project's budget
    assert worst_loss < precision.tolerance(mode, "denoise_loss")


def test_equal_sigmas_per_sample_path_equals_scalar_path():
    """where both apply - one noise level for the whole batch - the per-sample kernels and the scalar code path give the same bits"""
    s = scheduler()
    idx = DS.INDEX_SETS["mid"]
    assert idx[0] == idx[1]
    clean, noise, F = DS.clean_images().cuda(), DS.noise().cuda(), DS.initial_profile().expand(-1, -1, DS.T, -1, -1).contiguous().cuda()
    ts = s.timesteps[list(idx)]
    scalar = s.sigmas[idx[0]]
    per_sample = torch.stack([scalar, scalar]).reshape(2, 1, 1, 1, 1)
    noisy = s.add_noise(clean, noise, ts)
    assert torch.equal(noisy.cpu(), DS.clean_images() + DS.noise() * scalar)
    assert torch.equal(s.precondition_inputs(noisy, per_sample), s.precondition_inputs(noisy, scalar))
    assert torch.equal(s.precondition_outputs(noisy, F, per_sample), s.precondition_outputs(noisy, F, scalar))
    with pytest.raises(ValueError):
        s.precondition_inputs(noisy, torch.ones(3))


def test_driver_over_a_latent_store(model, tmp_path):
    from ladcast_amd.evaluate.denoise_loss import denoising_loss, evaluate_denoising_loss, store_samples, write_report
    from ladcast_amd.evaluate.validate_AR import NpyLatentStore

    model.set_gemm_precision("fp32")
    frames = (0.5 * torch.randn(6, DS.C, DS.H, DS.W, generator=torch.Generator().manual_seed(21))).numpy()
    start = datetime(2018, 1, 1)
    store = NpyLatentStore(frames, start, 6)
    init_times = [start + timedelta(hours=6 * i) for i in range(4)]  # 1 input frame + 2 target frames each: frames i .. i + 2
    prof, clean, stamps = store_samples(store, init_times, 1, 2)
    assert prof.shape == (4, DS.C, 1, DS.H, DS.W) and clean.shape == (4, DS.C, 2, DS.H, DS.W) and stamps == [2018010100, 2018010106, 2018010112, 2018010118]
    assert np.array_equal(clean[1, :, 0].numpy(), frames[2]) and np.array_equal(prof[3, :, 0].numpy(), frames[3])
    with pytest.raises(KeyError):
        store_samples(store, [start + timedelta(hours=24)], 1, 2)  # its last target frame is past the store
    rep = evaluate_denoising_loss(store, init_times, model, scheduler(), input_seq_len=1, return_seq_len=2, sigma_indices=[0, 999], seed=42, batch_size=4)
    write_report(rep, str(tmp_path))
    with open(tmp_path / "denoise_loss.csv") as f:
        rows = list(csv.DictReader(f))
    assert [int(r["sigma_index"]) for r in rows] == [0, 999] and [int(r["num_samples"]) for r in rows] == [4, 4]
    tables = []
    for r, idx in zip(rows, (0, 999)):
        o = denoising_loss(model, scheduler(), prof.cuda(), clean.cuda(), torch.tensor(stamps), indices=[idx] * 4, generator=torch.Generator().manual_seed(42))
        assert float(r["loss"]) == sum(o.per_sample.double().cpu().tolist()) / 4 and float(r["sigma"]) == float(o.sigmas[0])
        tables.append(o.table.double().mean(dim=0).cpu())
    assert np.allclose(np.load(tmp_path / "denoise_loss_table.npy"), ((tables[0] + tables[1]) / 2).numpy(), rtol=1e-12, atol=0)
    assert rep.table.shape == (DS.C, 2) and abs(rep.loss - (float(rows[0]["loss"]) + float(rows[1]["loss"])) / 2) <= 1e-12 * rep.loss
    with pytest.raises(ValueError):
        evaluate_denoising_loss(store, init_times, model, sigma_indices=[0], num_draws=1)
