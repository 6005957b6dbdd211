"""Host side of the denoising loss (ladcast_amd/evaluate/denoise_loss.py and what it stands on): the noise sampler and `get_sigmas`
against what the reference's own code gave (tests/golden/denoise_loss_ref.npz), the per-sample EDM coefficients bit for bit against the
oracle scheduler's expressions, the push-forward plan, the refused branches, the CLI parser and the three new ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch

from tests import denoise_synth as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(ROOT, "tests", "golden", "denoise_loss_ref.npz"))


def test_noise_sampler_draws_the_reference_indices(ref):
    from ladcast_amd.models.utils import Karras_sigmas_lognormal
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    sampler = Karras_sigmas_lognormal(EDMDPMSolverMultistepScheduler().sigmas)
    seen = []
    for cur_step in DS.SAMPLER_STEPS:
        idx = sampler(DS.SAMPLER_BATCH, cur_step=cur_step, generator=torch.Generator().manual_seed(DS.SAMPLER_SEED), device="cpu")
        assert idx.dtype == torch.int64 and idx.shape == (DS.SAMPLER_BATCH,)
        assert np.array_equal(idx.numpy(), ref[f"sampler_indices_{cur_step}"]), cur_step
        seen.append(idx)
    assert not torch.equal(seen[0], seen[1])  # the log-normal parameters move with cur_step
    late = sampler(DS.SAMPLER_BATCH, cur_step=10**9, generator=torch.Generator().manual_seed(DS.SAMPLER_SEED))  # clamped to the last step
    last = sampler(DS.SAMPLER_BATCH, cur_step=sampler.num_max_steps - 1, generator=torch.Generator().manual_seed(DS.SAMPLER_SEED))
    assert torch.equal(late, last)


def test_get_sigmas_shape_and_values(ref):
    from ladcast_amd.pipelines.utils import get_sigmas
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler

    s = EDMDPMSolverMultistepScheduler()
    for name, indices in DS.INDEX_SETS.items():
        ts = s.timesteps[list(indices)]
        got = get_sigmas(s, ts, 5, torch.float32, device="cpu")
        assert got.shape == (len(indices), 1, 1, 1, 1) and got.dtype == torch.float32
        assert np.array_equal(got.reshape(-1).numpy(), ref[f"sigmas_{name}"])
        assert torch.equal(got.reshape(-1), s.sigmas[list(indices)])
    assert get_sigmas(s, s.timesteps[[3]]).shape == (1, 1, 1, 1)  # n_dim defaults to 4
    assert get_sigmas(s, s.timesteps[[3, 4]], n_dim=1).shape == (2,)
    with pytest.raises(RuntimeError):
        get_sigmas(s, torch.tensor([0.123]))  # not an entry of the schedule


@pytest.mark.parametrize("pred", DS.PREDICTION_TYPES)
def test_edm_coefficients_are_the_oracle_expressions_bit_for_bit(pred):
    from ladcast_amd.schedulers import EDMDPMSolverMultistepScheduler
    from oracle.scheduler import EDMDPMSolverMultistepScheduler as O

    a, o = EDMDPMSolverMultistepScheduler(prediction_type=pred), O(prediction_type=pred)
    sigma = o.sigmas[:-1].clone()  # the 1000 training sigmas
    assert sigma.numel() == 1000
    c_in, c_skip, c_out, weight = a.edm_coefficients(sigma.reshape(-1, 1, 1, 1, 1))
    for v in (c_in, c_skip, c_out, weight):
        assert v.dtype == torch.float32 and v.shape == (1000,) and v.device.type == "cpu" and torch.isfinite(v).all()
    # the oracle's precondition_* on the probes (1, 0) / (0, 1) return the coefficients themselves: x * 1 and x + 0 are exact
    one, zero = torch.ones(1000), torch.zeros(1000)
    assert torch.equal(c_in, o.precondition_inputs(one, sigma))
    assert torch.equal(c_skip, o.precondition_outputs(one, zero, sigma))
    assert torch.equal(c_out, o.precondition_outputs(zero, one, sigma))
    assert torch.equal(weight, (sigma**2 + 0.5**2) / (sigma * 0.5) ** 2)
    assert bool((c_out < 0).all()) == (pred == "v_prediction")
    # the literal 0.5 of the weight is not sigma_data
    other = EDMDPMSolverMultistepScheduler(prediction_type=pred, sigma_data=1.0)
    assert torch.equal(other.edm_coefficients(sigma)[3], weight) and not torch.equal(other.edm_coefficients(sigma)[0], c_in)


def test_push_forward_plan(ref):
    from ladcast_amd.evaluate.denoise_loss import advance_timestamps, push_forward_plan

    as_tuples = lambda plan: [(s.start, s.end, s.profile, s.hours) for s in plan]  # noqa: E731
    assert as_tuples(push_forward_plan(4, 1, 1)) == [(0, 4, None, 0)]
    assert as_tuples(push_forward_plan(4, 2, 1)) == [(0, 2, None, 0), (2, 4, (1, 2), 6)]
    assert as_tuples(push_forward_plan(4, 2, 2)) == [(0, 2, None, 0), (2, 4, (0, 2), 6)]
    assert as_tuples(push_forward_plan(4, 4, 1)) == [(0, 1, None, 0), (1, 2, (0, 1), 6), (2, 3, (1, 2), 12), (3, 4, (2, 3), 18)]
    with pytest.raises(AssertionError, match="divisor"):
        push_forward_plan(4, 3, 1)
    with pytest.raises(ValueError):
        push_forward_plan(4, 4, 2)  # a one-frame slice cannot supply two conditioning frames
    # +6 h per step on every sample, across a month, a leap day and a new year; the reference's own loop left these stamps behind
    assert advance_timestamps([2018010100, 2018123121, 2020022821, 2018013118], 6) == [2018010106, 2019010103, 2020022903, 2018020100]
    assert advance_timestamps(DS.TIMESTAMPS, 18) == advance_timestamps(advance_timestamps(advance_timestamps(DS.TIMESTAMPS, 6), 6), 6)
    for key, name, k, lat, pred in DS.cases():
        if k > 1:
            assert advance_timestamps(DS.TIMESTAMPS, 6 * (k - 1)) == ref[f"timestamps_after_{key}"].tolist()


def test_unbuilt_branches_raise():
    from ladcast_amd.evaluate.denoise_loss import _check_objective, denoising_loss
    from ladcast_amd.schedulers import DDIMScheduler, EDMDPMSolverMultistepScheduler

    edm = EDMDPMSolverMultistepScheduler()
    _check_objective(edm, True, None)
    x = torch.zeros(1, 84, 1, 15, 30)
    for kw, sched in ((dict(), DDIMScheduler()), (dict(do_edm_style_training=False), edm), (dict(snr_gamma=5.0), edm)):
        with pytest.raises(NotImplementedError):
            denoising_loss(None, sched, x, x, torch.tensor([2018010100]), indices=[0], **kw)
    used = EDMDPMSolverMultistepScheduler()
    used.set_timesteps(20)
    with pytest.raises(ValueError, match="training schedule"):
        denoising_loss(None, used, x, x, torch.tensor([2018010100]), indices=[0])
    with pytest.raises(RuntimeError):
        denoising_loss(None, edm, x, x, torch.tensor([2018010100]), indices=[0])  # host tensors: there is no CPU path


def test_cli_parser():
    from ladcast_amd.evaluate.denoise_loss import build_parser

    base = ["--latent_path", "l.npy", "--start_date", "2018-01-01", "--init_times", "2018010200", "--ar_model", "AR", "--latent_normal_json", "n.json",
            "--output", "out"]
    a = build_parser().parse_args(base + ["--sigma_indices", "0", "999", "--lat_weighted_loss", "--num_push_forward_steps", "2"])
    assert a.sigma_indices == [0, 999] and a.num_draws is None and a.lat_weighted_loss and a.num_push_forward_steps == 2
    a = build_parser().parse_args(base + ["--num_draws", "3", "--seed", "7"])
    assert a.sigma_indices is None and a.num_draws == 3 and a.seed == 7
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--sigma_indices", "0", "--num_draws", "2"])


def test_library_header_and_binding_agree_on_the_new_symbols():
    import ladcast_amd.hip as hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    for name in ("ldc_edm_noise_inputs", "ldc_edm_denoise", "ldc_edm_denoise_loss"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in the header"
        assert hasattr(hip.lib, name), f"{name} is not exported by the library"
        res, args = hip.SIGNATURES[name]
        assert len(args) == len(m.group(1).split(",")), name  # one ctypes type per declared parameter
    assert re.search(r"#define\s+LDC_ABI_VERSION\s+5\b", header) and hip.ABI_VERSION == 5 and hip.lib.ldc_abi_version() == 5
    x = torch.zeros(2, 1, 1, 1, 1)
    with pytest.raises(RuntimeError):
        hip.edm_noise_inputs(x, x, torch.zeros(2), torch.zeros(2), x, x)  # host tensors are refused
