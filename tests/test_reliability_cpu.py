"""The oracle, the bounds and the planted defects of tests/reliability_refs.py judged on the CPU, and the host side of the driver's
`--reliability` flag with stubbed scores.  No GPU: the kernel itself is run by tests/test_gpu_reliability.py."""
import numpy as np
import pytest
import torch

from tests import reliability_refs as R


def _cases():
    """(name, x (M, C, H, W), t, w, nan_channel) of every case shape the GPU tests run"""
    for M in R.INT_M:
        c = R.integer_case(M)
        yield f"integers M={M}", c["x"], c["t"], c["w"], -1
    for M in R.PHYS_M:
        c = R.physical_case(M)
        for l in range(c["x"].shape[2]):
            yield f"physical M={M} lead {l}", c["x"][:, :, l], c["t"][:, l], c["w"], -1
    for H, W in R.FINISH_SHAPES:
        c = R.finish_case(H, W)
        yield f"finish {H}x{W}", c["x"], c["t"], c["w"], -1
        c = R.finish_nan_case(H, W)
        yield f"finish {H}x{W} NaN member, nanmean", c["x"], c["t"], c["w"], 0
    c = R.nan_table_case(R.NAN_M)
    for nc in range(4):
        yield f"NaN table nan_channel {nc}", c["x"], c["t"], c["w"], nc
    for case in R.GUARD_CASES:
        M, C, L, H, W, sst = case
        c = R.guard_case(*case)
        for l in range(L):
            yield f"guard {case} lead {l}", c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], sst


CASES = list(_cases())
_REF = {}


def ref_of(i):
    if i not in _REF:
        _, x, t, w, nc = CASES[i]
        _REF[i] = R.reliability_ref(x, t, w, nc)
    return _REF[i]


@pytest.mark.parametrize("fma", [False, True])
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_restatement_within_every_bound(i, fma):
    name, x, t, w, nc = CASES[i]
    got = R.kernel_f32(x, t, w, nc, fma=fma)
    r = R.check(got, ref_of(i), name)
    print(f"{name} fma={fma}: worst err / bound {r:.4f}")
    ref = ref_of(i)
    assert int(ref["hist"].sum()) + int(ref["n_invalid"].sum()) == x.shape[1] * x.shape[2] * x.shape[3]


@pytest.mark.parametrize("M", R.INT_M)
def test_integer_cases_are_exact(M):
    """the construction of integer_case holds: the fp32 restatement gives the float64 value rounded once, with or without contraction"""
    c = R.integer_case(M)
    ref = R.reliability_ref(c["x"], c["t"], c["w"])
    for fma in (False, True):
        got = R.kernel_f32(c["x"], c["t"], c["w"], fma=fma)
        for k in ("ens_mse", "ens_var"):
            assert R.same_value_bits(got[k], ref[k][0].float()), (M, k, fma)
        assert R.same_value_bits(got["hist_w"], ref["hist_w"][0].float())
    assert bool(torch.isnan(ref["ens_var"][0]).all()) == (M == 1)
    assert int((ref["hist"] > 0).sum()) >= min(M + 1, 3)  # more than one bin is hit


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for i, (name, x, t, w, nc) in enumerate(CASES):
        if x.shape[0] > 129:
            continue  # the small cases are enough to catch every defect
        try:
            R.check(R.kernel_f32(x, t, w, nc, defect=defect), ref_of(i), name)
        except AssertionError:
            caught.append(name)
    print(f"{defect}: caught by {len(caught)} of {len(CASES)} cases, e.g. {caught[:3]}")
    assert caught, defect


def test_oracle_equals_brute_force():
    g = R.gen(5)
    M, C, H, W = 4, 2, 3, 5
    x = torch.randint(-3, 4, (M, C, H, W), generator=g).float() * 0.5
    t = torch.randint(-3, 4, (C, H, W), generator=g).float() * 0.5
    x[1, 0, 0, 1] = float("nan")
    t[0, 2, 2] = float("nan")
    x[2, 0, 1, 1] = float("inf")
    x[0, 1, 1, 1] = float("-inf")
    w = R.cos_weights(H)
    for nc in (-1, 0):
        ref, want = R.reliability_ref(x, t, w, nc), R.brute_force(x, t, w, nc)
        assert torch.equal(ref["hist"], want["hist"]) and torch.equal(ref["n_invalid"], want["n_invalid"])
        assert ref["n_invalid"].tolist() == [2, 0] and int(ref["hist"].sum()) == C * H * W - 2
        torch.testing.assert_close(ref["hist_w"][0], want["hist_w"], rtol=1e-13, atol=0)
        for k in R.NAMES:
            torch.testing.assert_close(ref[k][0], want[k], rtol=1e-12, atol=0, equal_nan=True)
        assert bool(torch.isnan(ref["ens_var"][0][0])) == (nc != 0)  # inf - inf at one point: NaN by mean, dropped by nanmean


def test_ties_take_the_mid_rank():
    for M in (4, 5, 64, 100):
        x, t, bins = R.ties_case(M)
        b, valid = R.bins_of(x, t)
        assert b.reshape(-1).tolist() == bins and bool(valid.all())


# ---- the driver's flag with stubbed scores -----------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")


def _run(tmp_path, reliability, out_name):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    res.mkdir(exist_ok=True)
    for ts in (2018123000, 2018123118):
        np.save(res / f"latent_{ts}.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    C, T, M = 3, 4, 5
    calls = []

    def score(path, time_str, t_slots, c_slots):
        calls.append(time_str)
        n = len(calls)
        out = {k: np.full((C, T), float(n + i), dtype=np.float32) for i, k in enumerate(SCORES)}
        if reliability:
            hist = (np.arange(C * T * (M + 1)).reshape(C, T, M + 1) * n).astype(np.int32)
            out.update(ens_var=torch.full((C, T), 10.0 * n), ssr=torch.full((C, T), 0.5 * n), rank_hist=torch.from_numpy(hist),
                       rank_hist_weighted=torch.from_numpy(hist).float() * 0.25, n_invalid=torch.full((C, T), n, dtype=torch.int32))
        return out

    out_dir = tmp_path / out_name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + (["--reliability"] if reliability else []), score=score)
    return out, out_dir, (C, T, M)


def test_driver_accumulates_over_initial_times(tmp_path):
    plain, plain_dir, _ = _run(tmp_path, False, "plain")
    out, out_dir, (C, T, M) = _run(tmp_path, True, "rel")
    new = ("ens_var", "ssr", "rank_hist", "rank_hist_weighted", "n_invalid")
    assert sorted(p.name for p in out_dir.iterdir()) == sorted([p.name for p in plain_dir.iterdir()] + [f"{k}.npy" for k in new])
    for p in plain_dir.iterdir():  # the files of a run without the flag, byte for byte
        assert (out_dir / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(out_dir / f"{k}.npy") for k in new}
    assert a["ens_var"].shape == a["ssr"].shape == a["n_invalid"].shape == (2, C, T)
    assert a["ens_var"].dtype == a["ssr"].dtype == np.float32 and a["n_invalid"].dtype == np.int32
    assert (a["ens_var"][1] == 20.0).all() and (a["ssr"][0] == 0.5).all() and (a["n_invalid"][1] == 2).all()
    base = np.arange(C * T * (M + 1)).reshape(C, T, M + 1)
    assert a["rank_hist"].dtype == np.int64 and a["rank_hist"].shape == (C, T, M + 1) and np.array_equal(a["rank_hist"], base * 3)
    assert a["rank_hist_weighted"].dtype == np.float64 and np.array_equal(a["rank_hist_weighted"], base * 0.75)
    for k in new:
        assert np.array_equal(out[k], a[k])
    assert not any(k in plain for k in new)


def test_driver_refuses_a_scorer_without_reliability(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    res.mkdir()
    np.save(res / "latent_2018010100.npy", np.zeros((1, 1, 1, 1, 1), dtype=np.float32))
    plain = {k: np.zeros((3, 4), dtype=np.float32) for k in SCORES}
    with pytest.raises(ValueError, match="reliability"):
        EG.main(["--result_path", str(res), "--output", str(tmp_path / "o"), "--end_date", "2018-02-01", "--total_lead_time_hour", "24", "--reliability"],
                score=lambda *a: plain)
