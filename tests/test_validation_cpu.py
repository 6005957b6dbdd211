"""Host side of the validation hook (ladcast_amd.evaluate.validate_AR, C ABI ldc_validation_scores): the oracle restatement of the three
scores (tests/validation_oracle.py) is pinned to the reference's own `log_validation` through tests/golden/validation_ref.npz, the header
and the built library carry the new entry points under the unchanged ABI version, and the driver's refusals, column names and latent-store
indexing need no device."""
import ctypes
import os
import re
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

from tests import validation_oracle as VO
from tests import validation_synth as VS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "validation_ref.npz"))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def host_tables():
    """the hook's loop (train_AR.py:157-358) over the stand-ins on the CPU, scores from the oracle restatement -> (rmse (T, 4C), crps (T, C),
    the sampler's recorded calls)"""
    from ladcast_amd.pipelines.utils import convert_datetime_to_int
    from oracle.scoring import get_normalized_lat_weights_based_on_cos

    frames, (mean, std), sampler, dec = VS.latent_frames(), VS.field_statistics(), VS.RecordingSampler(), VS.UpsampleDecoder()
    phys = lambda y: y * std.view(1, -1, 1, 1) + mean.view(1, -1, 1, 1)  # noqa: E731  ((N, C, H, W); x / 1 == x)
    w = get_normalized_lat_weights_based_on_cos(torch.from_numpy(np.linspace(-88.5, 90, VS.LAT_H * VS.SCALE))).float()
    index = lambda t: int((t - VS.START) / timedelta(hours=VS.STEP_HOURS))  # noqa: E731
    per_time = {"edm": [], "pipeline": []}
    for init in VS.INIT_TIMES:
        i0 = index(init)
        known = VS.latent_transform(frames[i0 - VS.T_IN + 1 : i0 + 1].permute(1, 0, 2, 3)).unsqueeze(0)
        ref = phys(dec.decode(frames[i0 + 1 : i0 + 1 + VS.T]).sample).permute(1, 0, 2, 3)  # (C, T, H, W)
        chain = {k: known for k in per_time}
        fields = {k: [] for k in per_time}
        for step in range(VS.T // VS.R):
            ts = torch.tensor([convert_datetime_to_int(init + timedelta(hours=step * VS.STEP_HOURS))])
            for k in per_time:
                smp = sampler(None, sample_size=VS.ENS, return_seq_len=VS.R, num_inference_steps=VS.INFERENCE_STEPS, known_latents=chain[k],
                              timestamps=ts, sampler_type=k)
                chain[k] = smp[:, :, -VS.T_IN:]
                lat = VS.latent_inv_transform(smp)
                fields[k].append(torch.stack([phys(dec.decode(lat[m].permute(1, 0, 2, 3)).sample).permute(1, 0, 2, 3) for m in range(VS.ENS)]))
        for k in per_time:
            per_time[k].append(VO.validation_scores(torch.cat(fields[k], dim=2), ref, w))
    mean_of = lambda k, name: torch.stack([s[name] for s in per_time[k]]).mean(dim=0)  # noqa: E731
    rmse = torch.cat([torch.sqrt(mean_of(k, n)).T for k in ("edm", "pipeline") for n in ("ens_mse", "single_mse")], dim=1)
    return rmse, mean_of("edm", "crps").T, sampler.calls


def test_oracle_restatement_reproduces_the_reference_hook(golden):
    rmse, crps, calls = host_tables()
    assert golden["rmse_values"].shape == (VS.T, 1 + 4 * VS.C) and golden["crps_values"].shape == (VS.T, 1 + VS.C)
    lead = [VS.STEP_HOURS * (i + 1) for i in range(VS.T)]
    assert golden["rmse_values"][:, 0].tolist() == lead and golden["crps_values"][:, 0].tolist() == lead
    assert _rel(rmse.numpy(), golden["rmse_values"][:, 1:]) < 1e-6
    assert _rel(crps.numpy(), golden["crps_values"][:, 1:]) < 1e-6
    assert [c[0] for c in calls] == golden["call_sampler_type"].tolist() and [c[1] for c in calls] == golden["call_timestamp"].tolist()
    # Q12: chunk `step` gets init + step * 6 h, not init + step * R * 6 h
    assert golden["call_timestamp"].tolist()[:4] == [2018010112, 2018010112, 2018010118, 2018010118]


def test_header_and_library_carry_the_entry_points_under_abi_5():
    from ladcast_amd import hip

    header = open(os.path.join(ROOT, "include", "ladcast_hip.h")).read()
    assert re.search(r"#define\s+LDC_ABI_VERSION\s+5\b", header)
    assert re.search(r"long long\s+ldc_validation_scores_workspace_bytes\(int C, int L, int H, int W\);", header)
    assert re.search(r"\bint\s+ldc_validation_scores\(const float\* forecast,", header)
    lib = ctypes.CDLL(hip.LIB_PATH)
    for name in ("ldc_validation_scores_workspace_bytes", "ldc_validation_scores"):
        assert hasattr(lib, name) and name in hip.SIGNATURES
    assert hip.lib.ldc_abi_version() == 5 and hip.ABI_VERSION == 5
    # 7 values per partial record, one record per 256 points; nothing for an empty problem
    assert hip.lib.ldc_validation_scores_workspace_bytes(3, 2, 33, 17) == 2 * 3 * 3 * 7 * 4
    assert hip.lib.ldc_validation_scores_workspace_bytes(0, 2, 33, 17) == 0
    assert hip.lib.ldc_rollout_scores_workspace_bytes(3, 2, 33, 17) == 2 * 3 * 3 * 15 * 4  # unchanged


def test_column_names_and_host_side_refusals():
    from ladcast_amd.evaluate import validate_AR as VA

    cols = VA.column_names(VS.CHANNEL_NAMES)
    assert len(cols) == 84 and cols[0] == "z_level50" and cols[12] == "z_level1000" and cols[13] == "q_level50" and cols[78:] == VS.CHANNEL_NAMES[6:]
    assert VA.column_names(["a", "b", "c"], levels=(1, 2), num_atm_vars=1) == ["a_level1", "a_level2", "b", "c"]
    mean, std = VS.field_statistics()
    store = VA.NpyLatentStore(VS.latent_frames().numpy(), VS.START, VS.STEP_HOURS)
    ident = lambda x: x  # noqa: E731

    def call(**kw):
        a = dict(channel_names=VS.CHANNEL_NAMES, total_lead_time_hour=24, step_size_hour=6, ensemble_size=3, return_seq_len=2)
        a.update(kw)
        return VA.log_validation("validation", store, a.pop("channel_names"), None, mean, std, 1, a.pop("return_seq_len"), None, ident, ident,
                                 timestamp_list=list(VS.INIT_TIMES), **a)

    with pytest.raises(ValueError, match="divisible by step_size_hour"):
        call(total_lead_time_hour=25)
    with pytest.raises(ValueError, match="cannot assign the last chunk"):
        call(return_seq_len=3)
    with pytest.raises(ValueError, match="column names"):
        call(channel_names=VS.CHANNEL_NAMES[:-1])
    with pytest.raises(NotImplementedError):
        call(ensemble_size=65)


def test_npy_latent_store_time_indexing():
    from ladcast_amd.evaluate import NpyLatentStore

    arr = np.arange(5 * 2 * 1 * 1, dtype=np.float64).reshape(5, 2, 1, 1)
    store = NpyLatentStore(arr, "2018-01-01T06", 6)
    got = store.latents_at([datetime(2018, 1, 1, 18), datetime(2018, 1, 1, 6), np.datetime64("2018-01-02T06")])
    assert got.dtype == np.float32 and got.shape == (3, 2, 1, 1) and got[:, 0, 0, 0].tolist() == [4.0, 0.0, 8.0]
    assert store.index_of(2018010112) == 1
    for bad in (datetime(2018, 1, 1, 0), datetime(2018, 1, 2, 12), datetime(2018, 1, 1, 9), datetime(2018, 1, 1, 6, 30)):
        with pytest.raises(KeyError):
            store.latents_at([bad])
    with pytest.raises(ValueError):
        NpyLatentStore(arr[0], "2018-01-01", 6)


def test_driver_structure_with_the_kernel_replaced_by_the_oracle(golden, monkeypatch):
    """`validate_initial_time` (frames read, chains, Q12 timestamps, lead-major decode batches, slots and column offsets) over the stand-ins
    on the CPU, its two device calls replaced by torch: the scorer by the oracle restatement, the truth's inverse normalisation by the
    formula.  The per-time buffers give the reference's tables; a decode batch of one lead time gives the same buffers."""
    from ladcast_amd.evaluate import validate_AR as VA

    def scores(fc, truth, w, *, lead_dim, mean, std, truth_slots, out, lead_offset):
        assert lead_dim == 0 and fc.shape[1] == VS.ENS and len(truth_slots) == fc.shape[0]
        phys = fc.permute(1, 2, 0, 3, 4) * std.view(1, -1, 1, 1, 1) + mean.view(1, -1, 1, 1, 1)
        s = VO.validation_scores(phys, truth[truth_slots].permute(1, 0, 2, 3), w)
        for i, k in enumerate(VA.VALIDATION_SCORE_NAMES):
            out[i, :, lead_offset : lead_offset + fc.shape[0]] = s[k]

    monkeypatch.setattr(VA, "validation_scores", scores)
    monkeypatch.setattr(VA, "inverse_normalize_transform_3D", lambda y, m, s: y * s.view(1, -1, 1, 1, 1) + m.view(1, -1, 1, 1, 1))
    mean, std = VS.field_statistics()
    store, sampler = VA.NpyLatentStore(VS.latent_frames().numpy(), VS.START, VS.STEP_HOURS), VS.RecordingSampler()

    def run(init, **kw):
        return VA.validate_initial_time(init, store, None, VS.UpsampleDecoder(), mean, std, VS.T_IN, VS.R, VS.latent_transform, VS.latent_inv_transform,
                                        total_num_steps=VS.T, step_size_hour=VS.STEP_HOURS, ensemble_size=VS.ENS, num_inference_steps=VS.INFERENCE_STEPS,
                                        sampler=sampler, **kw)

    bufs = [run(t) for t in VS.INIT_TIMES]
    assert [c[0] for c in sampler.calls] == golden["call_sampler_type"].tolist() and [c[1] for c in sampler.calls] == golden["call_timestamp"].tolist()
    m = {k: torch.stack([b[k] for b in bufs]).mean(dim=0) for k in ("EDM", "MS")}
    rmse = torch.cat([torch.sqrt(m[k][i]).T for k in ("EDM", "MS") for i in (0, 1)], dim=1)
    assert _rel(rmse.numpy(), golden["rmse_values"][:, 1:]) < 1e-6 and _rel(m["EDM"][2].T.numpy(), golden["crps_values"][:, 1:]) < 1e-6
    one = run(VS.INIT_TIMES[0], decode_batch_frames=VS.ENS)  # the stand-in decoder is elementwise: batching cannot change a bit
    assert all(torch.equal(one[k], bufs[0][k]) for k in one)
    only = run(VS.INIT_TIMES[0], eval_ms=False, advance_by_chunk=True)
    assert set(only) == {"EDM"} and [c[1] for c in sampler.calls[-2:]] == [2018010112, 2018010200]
