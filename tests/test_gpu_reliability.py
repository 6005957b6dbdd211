"""The ensemble-reliability kernel (csrc/reliability.hip: ldc_rollout_reliability) through the C ABI and `rollout_reliability`, against
the float64 oracle and the COUNTED bounds of tests/reliability_refs.py (judged on the CPU by tests/test_reliability_cpu.py):
  a. integers on which every fp32 operation is exact, M = 1 .. 1024 (every register arm, the streaming kernel, several tiles per
     workgroup): histogram and n_invalid bit-exact, ens_mse / ens_var the float64 value rounded once
  b. ties and ends: the rank bins written out by hand
  c. physical scale through the fused inverse normalisation, both forecast layouts
  d. ens_mse is ldc_rollout_scores' ens_mse bit for bit for M <= 64
  e. the finish loop: 65 and 129 records, one NaN member in the last record
  f. the NaN / inf table: mean against nanmean, n_invalid, the histogram without the invalid points
  g. guard bands around every buffer, the columns outside l_off .. l_off + L - 1 left alone
  h. refused arguments launch nothing
  i. the driver's --reliability flag on the tiny synthetic DC-AE"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import reliability_refs as R
from tests.redzone import UNWRITTEN32, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    return eu


def column(d, l):
    """lead time l of a rollout_reliability result as the dict reliability_refs.check takes"""
    return dict(ens_mse=d["ens_mse"][:, l], ens_var=d["ens_var"][:, l], ssr=d["ssr"][:, l], hist=d["rank_hist"][:, l],
                hist_w=d["rank_hist_weighted"][:, l], n_invalid=d["n_invalid"][:, l])


def run_one(E, x, t, w, nan_channel=-1):
    """x (M, C, H, W), t (C, H, W) on the host -> the one lead time's result"""
    d = E.rollout_reliability(x.cuda()[:, :, None], t.cuda()[:, None], w.cuda(), nan_channel)
    assert d["rank_hist"].dtype == torch.int32 and d["n_invalid"].dtype == torch.int32 and d["rank_hist"].shape[-1] == x.shape[0] + 1
    return column(d, 0)


def mse_of_rollout_scores(E, x, t, w, nan_channel=-1):
    return E.rollout_scores(x.cuda()[:, :, None], t.cuda()[:, None], None, w.cuda(), nan_channel)["ens_mse"][:, 0]


# ---- a. integers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.INT_M)
def test_integers(E, M):
    c = R.integer_case(M)
    x, t, w = c["x"], c["t"], c["w"]
    ref = R.reliability_ref(x, t, w)
    got = run_one(E, x, t, w)
    r = R.check(got, ref, f"M={M}")
    print(f"integers M={M}: worst err / bound {r:.4f}")
    for k in ("ens_mse", "ens_var"):
        assert R.same_value_bits(got[k], ref[k][0].float()), f"M={M}: {k} {got[k].tolist()} is not the float64 value {ref[k][0].tolist()} rounded once"
    assert R.same_value_bits(got["hist_w"], ref["hist_w"][0].float())
    P = x.shape[2] * x.shape[3]
    assert got["hist"].sum(-1).tolist() == [P - int(n) for n in got["n_invalid"]] == [P, P]
    assert bool(torch.isnan(got["ens_var"]).all()) == (M == 1) and bool(torch.isnan(got["ssr"]).all()) == (M == 1)
    if M <= 64:
        assert R.same_value_bits(got["ens_mse"], mse_of_rollout_scores(E, x, t, w)), "ens_mse against ldc_rollout_scores"


# ---- b. ties and ends ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [4, 5, 64, 65, 100])
def test_ties_and_ends(E, M):
    x, t, bins = R.ties_case(M)
    got = run_one(E, x, t, torch.ones(1))
    want = torch.bincount(torch.tensor(bins), minlength=M + 1)
    assert got["hist"][0].cpu().tolist() == want.tolist(), (got["hist"][0].nonzero().reshape(-1).tolist(), bins)
    assert got["hist_w"][0].cpu().tolist() == want.float().tolist() and int(got["n_invalid"][0]) == 0


# ---- c. physical scale, d. cross-check -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale(E, M):
    c = R.physical_case(M)
    L = c["x"].shape[2]
    vd, td, wd, md, sd = c["v"].cuda(), c["t"].cuda(), c["w"].cuda(), c["mean"].cuda(), c["std"].cuda()
    d = E.rollout_reliability(vd, td, wd, -1, mean=md, std=sd, target_std=c["target_std"])
    frames = vd.permute(2, 0, 1, 3, 4).contiguous()  # the decoder's frame-major layout
    d2 = E.rollout_reliability(frames, td, wd, -1, lead_dim=0, mean=md, std=sd, target_std=c["target_std"])
    for k in d:
        a, b = d[k], d2[k]
        assert R.same_value_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b), (k, "the two forecast layouts")
    for l in range(L):
        r = R.check(column(d, l), R.reliability_ref(c["x"][:, :, l], c["t"][:, l], c["w"]), f"M={M} lead {l}")
        print(f"physical M={M} lead {l}: worst err / bound {r:.4f}")
    if M <= 64:
        roll = E.rollout_scores(vd, td, None, wd, -1, mean=md, std=sd, target_std=c["target_std"])
        assert R.same_value_bits(d["ens_mse"], roll["ens_mse"]), "ens_mse against ldc_rollout_scores"


# ---- e. the finish loop ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", R.FINISH_SHAPES)
def test_finish_loop(E, H, W):
    c = R.finish_case(H, W)
    assert R.n_records(H * W, R.FINISH_M) == -(-H * W // 256)
    got = run_one(E, c["x"], c["t"], c["w"])
    r = R.check(got, R.reliability_ref(c["x"], c["t"], c["w"]), f"{H}x{W}")
    print(f"finish loop {H}x{W}: worst err / bound {r:.4f}")
    assert R.same_value_bits(got["ens_mse"], mse_of_rollout_scores(E, c["x"], c["t"], c["w"]))
    cn = R.finish_nan_case(H, W)  # one NaN member in the last thread of the last record
    for nan_channel in (-1, 0):
        got = run_one(E, cn["x"], cn["t"], cn["w"], nan_channel)
        R.check(got, R.reliability_ref(cn["x"], cn["t"], cn["w"], nan_channel), f"{H}x{W} NaN member, nan_channel {nan_channel}")
        for k in R.NAMES:
            assert bool(torch.isnan(got[k]).all()) == (nan_channel < 0), (k, nan_channel)
        assert int(got["n_invalid"][0]) == 1 and int(got["hist"].sum()) == H * W - 1


# ---- f. NaN / inf table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan_channel", [0, 1, 2, 3])
def test_nan_inf_table(E, nan_channel):
    """channel 0: clean / NaN in one member / NaN in all members / NaN in truth (/ NaN in the climatology: clean here); channel 1: those and
    +inf, -inf in one member, +inf in truth; channel 2: NaN everywhere; channel 3: clean"""
    c = R.nan_table_case(R.NAN_M)
    x, t, w, kind = c["x"], c["t"], c["w"], c["kind"]
    ref = R.reliability_ref(x, t, w, nan_channel)
    got = run_one(E, x, t, w, nan_channel)
    R.check(got, ref, f"nan_channel {nan_channel}")
    P = x.shape[2] * x.shape[3]
    invalid = [int(((kind[0] >= 1) & (kind[0] <= 3)).sum()), int(((kind[1] >= 1) & (kind[1] <= 3)).sum()), P, 0]  # inf is no NaN
    assert got["n_invalid"].cpu().tolist() == invalid and got["hist"].sum(-1).cpu().tolist() == [P - n for n in invalid]
    for ch in range(4):
        nanmean = ch == nan_channel
        for k in ("ens_mse", "ens_var"):
            v = float(got[k][ch])
            if ch == 3:
                assert np.isfinite(v)
            elif ch == 2:
                assert np.isnan(v)  # no valid point: NaN by either rule
            elif ch == 0:
                assert np.isfinite(v) == nanmean, (ch, k, v)  # mean: one NaN point -> NaN; nanmean: the valid points
            else:  # channel 1: an inf member makes se inf and var NaN (inf - inf); an inf truth makes se inf
                assert (np.isinf(v) if k == "ens_mse" else np.isfinite(v)) == nanmean and (nanmean or np.isnan(v)), (ch, k, v)
    assert R.same_value_bits(got["ens_mse"], mse_of_rollout_scores(E, x, t, w, nan_channel))


# ---- g. guard bands --------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("case", R.GUARD_CASES)
def test_guard_bands(case, layout):
    from ladcast_amd import hip

    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    HW, ld, FMAX = H * W, H * W + 8, R.R.FLT_MAX_BITS
    inp = dict(poison=FMAX, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(c["x"].reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(c["x"].permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    gt = guarded(C, HW, ld, batch=R.N_TRUTH, batch_stride=C * ld + 16, **inp).fill(c["truth_table"].reshape(R.N_TRUTH, C, HW))
    gl = guarded(1, H, **inp).fill(c["w"])
    assert gt.bs < 4096  # a slot read from a guard word points one entry past the table, into its poisoned back guard
    gts = guarded(1, L, dtype=torch.int32, poison=R.N_TRUTH, unwritten=False).fill(torch.tensor(c["t_slots"]))
    mean, std, ts = torch.linspace(-1.0, 2.0, C), torch.linspace(0.75, 1.5, C), 0.5
    gm, gs = guarded(1, C, **inp).fill(mean), guarded(1, C, **inp).fill(std)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    nbytes = int(hip.lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    assert nbytes == 4 * L * C * R.n_records(HW, M) * (8 + 2 * (M + 1))
    gw = guarded(1, nbytes // 4, unwritten=False)
    go, gn = guarded(3 * C, Lt), guarded(C, Lt, dtype=torch.int32)
    gh, ghw = guarded(C * Lt, M + 1, dtype=torch.int32), guarded(C * Lt, M + 1)
    assert hip.lib.ldc_rollout_reliability(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gl.view), M, C, L,
                                           H, W, sst, _p(go.view), _p(gh.view), _p(ghw.view), _p(gn.view), Lt, 1, _p(gw.view), nbytes, stream) == 0
    torch.cuda.synchronize()
    for k, g in dict(forecast=gf, truth=gt, lat_weight=gl, truth_slot=gts, mean=gm, std=gs, workspace=gw, out=go, hist_count=gh, hist_weight=ghw,
                     n_invalid=gn).items():
        assert_untouched(g, k)
    out, ninv = go.payload()[0].reshape(3, C, Lt), gn.payload()[0].reshape(C, Lt)
    hist, hist_w = gh.payload()[0].reshape(C, Lt, M + 1), ghw.payload()[0].reshape(C, Lt, M + 1)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(out[:, :, col]) and _unwritten(ninv[:, col]) and _unwritten(hist[:, col]) and _unwritten(hist_w[:, col])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    for l in range(L):
        ref = R.reliability_ref(xp[:, :, l], c["truth_table"][c["t_slots"][l]], c["w"], sst)
        got = dict(ens_mse=out[0, :, 1 + l], ens_var=out[1, :, 1 + l], ssr=out[2, :, 1 + l], hist=hist[:, 1 + l], hist_w=hist_w[:, 1 + l],
                   n_invalid=ninv[:, 1 + l])
        r = R.check(got, ref, f"{case} {layout} lead {l}")
        print(f"guard bands {case} {layout} lead {l}: worst err / bound {r:.4f}")
        assert int(ref["n_invalid"][sst]) > 0 and all(np.isfinite(float(out[i, sst, 1 + l])) for i in range(3))


# ---- h. arguments ----------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    C, L, H, W = 1, 1, 4, 8
    x, t, w, slot = torch.zeros(1025, C, L, H, W, device="cuda"), torch.zeros(C, L, H, W, device="cuda"), torch.ones(H, device="cuda"), torch.zeros(
        L, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)

    def call(M, nbytes):
        go, gn = guarded(3 * C, L), guarded(C, L, dtype=torch.int32)
        gh, ghw = guarded(C * L, 1026, dtype=torch.int32), guarded(C * L, 1026)
        st = hip.lib.ldc_rollout_reliability(_p(x), x.stride(0), x.stride(2), x.stride(1), None, None, 1.0, _p(t), t.stride(1), t.stride(0), _p(slot), _p(w), M,
                                             C, L, H, W, -1, _p(go.view), _p(gh.view), _p(ghw.view), _p(gn.view), L, 0, _p(gw.view), nbytes, stream)
        torch.cuda.synchronize()
        untouched = all(_unwritten(g.payload()) for g in (go, gn, gh, ghw))
        for g in (go, gn, gh, ghw, gw):
            assert_untouched(g)
        return st, untouched

    need = int(hip.lib.ldc_rollout_reliability_workspace_bytes(5, C, L, H, W))
    assert need == 4 * (8 + 12) and hip.lib.ldc_rollout_reliability_workspace_bytes(0, C, L, H, W) == 0
    assert call(0, 1 << 18) == (-1, True)  # LDC_ERR_ARG
    assert call(-3, 1 << 18) == (-1, True)
    assert call(1025, 1 << 18) == (-3, True)  # LDC_ERR_UNSUPPORTED
    assert call(5, need - 4) == (-1, True)
    assert call(5, need) == (0, False) and call(1024, 1 << 18) == (0, False)
    with pytest.raises(ValueError):
        E.rollout_reliability(x, t, w, -1)
    out = E.empty_reliability(1025, C, L, "cuda")
    with pytest.raises(RuntimeError, match="ldc_rollout_reliability"):
        hip.rollout_reliability(x, t, slot, w, *out._buffers, M=1025, C=C, L=L, H=H, W=W, member_stride=x.stride(0), lead_stride=x.stride(2),
                                channel_stride=x.stride(1), truth_slot_stride=t.stride(1), truth_channel_stride=t.stride(0), L_total=L)
    with pytest.raises(RuntimeError):
        E.rollout_reliability(x[:5].cpu(), t, w, -1)  # device tensors only


# ---- i. the driver ---------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
NEW = ("ens_var", "ssr", "rank_hist", "rank_hist_weighted", "n_invalid")


def test_driver_reliability_flag(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.io import save_latent_npy
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    inits = [2020022812, 2020022818]  # frames from 2020-02-27 00 h, 6 h apart: frames 6 and 7; their leads are frames 7 .. 9 and 8 .. 10
    gen = torch.Generator().manual_seed(47)
    mean, std = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    names = ["geopotential", "temperature", "2m_temperature", "sea_surface_temperature"]
    lv = (300, 500, 850)
    norm = {"geopotential": {"mean": {str(p): float(mean[i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[i]) for i, p in enumerate(lv)}},
            "temperature": {"mean": {str(p): float(mean[3 + i]) for i, p in enumerate(lv)}, "std": {str(p): float(std[3 + i]) for i, p in enumerate(lv)}},
            "2m_temperature": {"mean": float(mean[6]), "std": float(std[6])}, "sea_surface_temperature": {"mean": float(mean[7]), "std": float(std[7])}}
    (tmp_path / "norm.json").write_text(json.dumps(norm))
    (tmp_path / "config.json").write_text(json.dumps(tiny_dcae_config()))
    latents = torch.randn(2, ENS, C_LAT, 1 + T, h, w_, generator=gen)
    save_latent_npy(latents, inits, str(tmp_path / "rollout"))
    truth = torch.randn(11, C, H, W, generator=gen) * std.view(1, C, 1, 1) + mean.view(1, C, 1, 1)
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.3] = float("nan")  # land
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H, W))  # sparse: zeros
    clim.flush()
    del clim

    def run(flag, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names] + (["--reliability"] if flag else [])
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, rel = run(False, "plain"), run(True, "rel")
    assert sorted(p.name for p in rel.iterdir()) == sorted([p.name for p in plain.iterdir()] + [f"{k}.npy" for k in NEW])
    for p in plain.iterdir():  # the five scores (and the time stamps) bit for bit
        assert (rel / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(rel / f"{k}.npy") for k in NEW}
    assert a["ens_var"].shape == a["ssr"].shape == a["n_invalid"].shape == (2, C, T) and a["rank_hist"].shape == a["rank_hist_weighted"].shape == (C, T, ENS + 1)
    assert a["rank_hist"].dtype == np.int64 and a["rank_hist_weighted"].dtype == np.float64 and a["n_invalid"].dtype == np.int32
    # the oracle on the fields the product decoder returns for the same frame batches
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in mean]), torch.tensor([float(v) for v in std])
    lat_w = EG.lat_weights_for(H)
    hist, hist_w, hist_b = torch.zeros(C, T, ENS + 1, dtype=torch.int64), torch.zeros(C, T, ENS + 1, dtype=torch.float64), torch.zeros(C, T, ENS + 1, dtype=torch.float64)
    for n in range(2):
        for l in range(T):
            y = model.decode(latents[n, :, :, 1 + l].contiguous().cuda()).sample
            phys = inverse_normalize_transform_3D(y.reshape(ENS, C, 1, H, W), mean32, std32).reshape(ENS, C, H, W).cpu()
            ref = R.reliability_ref(phys, truth[6 + n + 1 + l], lat_w, SST)
            R.judge(torch.from_numpy(a["ens_var"][n, :, l]), ref["ens_var"], f"init {n} lead {l} ens_var")
            R.judge(torch.from_numpy(a["ssr"][n, :, l]), ref["ssr"], f"init {n} lead {l} ssr")
            R.judge(torch.from_numpy(np.load(rel / "ens_mse.npy")[n, :, l]), ref["ens_mse"], f"init {n} lead {l} ens_mse")
            assert a["n_invalid"][n, :, l].tolist() == ref["n_invalid"].tolist() and int(ref["n_invalid"][SST]) > 0
            hist[:, l] += ref["hist"]
            hist_w[:, l] += ref["hist_w"][0]
            hist_b[:, l] += ref["hist_w"][1]
    assert np.array_equal(a["rank_hist"], hist.numpy()) and int(hist.sum()) == 2 * T * C * H * W - int(a["n_invalid"].sum())
    R.judge(torch.from_numpy(a["rank_hist_weighted"]), (hist_w, hist_b), "rank_hist_weighted")
    assert np.isfinite(a["ssr"]).all()
