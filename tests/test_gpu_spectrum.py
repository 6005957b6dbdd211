"""The zonal-spectrum kernel (csrc/spectrum.hip: ldc_rollout_spectrum) through the C ABI and `rollout_spectrum`, against the float64
oracle and the COUNTED bound of tests/spectrum_refs.py (judged on the CPU by tests/test_spectrum_cpu.py):
  a. the shapes at which the kernel can go wrong, each against the oracle within the bound
  b. pure tones at k0 = 1, W / 2 - 1, W / 2 against the analytic spectrum: the fold's end points, s_k, the pivot
  c. the fused inverse normalisation, the two forecast layouts and a truth table through slots: bit-equal
  d. NaN rows, zero-weight rows, a (c, l) without a valid row
  e. l_off columns, guard bands around every buffer, the workspace query
  f. run-to-run bit-equality; M = 1: spec_members == spec_mean bit for bit (one member IS the mean: the same sequence goes through the
     same arithmetic, and both planes are scaled by the same expression)
  g. refused arguments launch nothing
  h. the driver: score_latent_rollout(spectrum=True) and the command line's --spectrum on the tiny synthetic DC-AE"""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests import spectrum_refs as R
from tests.redzone import UNWRITTEN32, assert_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import ladcast_amd.evaluate.utils as eu

    return eu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the shared cases are read-only


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def run(E, x, t, w, **kw):
    """x (M, C, L, H, W), t (C, L, H, W), w (H,) numpy -> the result as numpy arrays"""
    d = E.rollout_spectrum(dev(x), dev(t), dev(w), **kw)
    K = x.shape[-1] // 2 + 1
    assert all(d[k].shape == (x.shape[1], x.shape[2], K) and d[k].dtype == torch.float32 for k in R.NAMES) and d["n_invalid"].dtype == torch.int32
    return host(d)


def same(a, b):
    """bit for bit (NaN payloads included)"""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32)) for k in R.NAMES + ("n_invalid",))


# ---- a. shapes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_shapes_against_the_oracle(E, shape):
    c = R.case(shape)
    if shape == (2, 1, 1, 37, 16):  # rows per workgroup (= per workspace record) RPW = 8: 37 rows are 5 records, the last of 5 rows
        assert R.RPW == 8 and -(-shape[3] // R.RPW) == 5
    got = run(E, c["x"], c["t"], c["w"])
    r = R.check(got, R.spectrum_ref(c["x"], c["t"], c["w"]), str(shape))
    print(f"{shape}: worst err / bound {r:.4f}")
    assert same(got, run(E, c["x"], c["t"], c["w"])), "two runs differ"
    if shape[0] == 1:
        assert np.array_equal(got["spec_members"].view(np.int32), got["spec_mean"].view(np.int32))


def test_pivot_case(E):
    c = R.pivot_case()
    ref = R.spectrum_ref(c["x"], c["t"], c["w"])
    r = R.check(run(E, c["x"], c["t"], c["w"]), ref, "mean 2e5, amplitude 1e-2 at W / 2 - 1")
    print(f"pivot case: worst err / bound {r:.4f}")


# ---- b. pure tones ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 6, 240])
@pytest.mark.parametrize("which", ["1", "W/2-1", "W/2"])
def test_pure_tones(E, W, which):
    """A cos(2 pi k0 j / W) + B: P_0 = B^2, P_k0 = A^2 / 2 (A^2 at k0 = W / 2), zero elsewhere.  No oracle: the bound of spectrum_refs on the
    analytic amplitudes, plus what rounding the row to fp32 can move an amplitude: d = U (|A| + |B|), s_k (2 |a_k| d + d^2)"""
    A, B = 3.0, 5.0
    k0 = dict([("1", 1), ("W/2-1", W // 2 - 1), ("W/2", W // 2)])[which]
    y, want = R.pure_tone(W, k0, A, B)
    got = run(E, y[None, None, None], y[None, None], np.ones(2, np.float32))
    s, g = R.s_k(W), R.gamma(W)
    a = np.sqrt(want / s)
    d_mu = R.n_mu(W) * R.U * (abs(A) + abs(B))
    rv = abs(A) + d_mu  # >= the residual's rms
    d = R.U * (abs(A) + abs(B))
    bound = s * (2 * a * g * rv + g * g * rv * rv) + s * (2 * a * d + d * d) + 2 * R.U * want
    bound[0] = 2 * abs(B) * (d_mu + d) + (d_mu + d) ** 2 + 2 * R.U * want[0]
    for k in R.NAMES:
        err = np.abs(got[k][0, 0].astype(np.float64) - want)
        print(f"W={W} k0={k0} {k}: worst err / bound {float((err / bound).max()):.4f}")
        assert (err <= bound).all(), (k, got[k][0, 0].tolist(), want.tolist())


# ---- c. fused inverse normalisation, layouts, truth slots --------------------------------------------------------------------------------
def test_fused_inverse_normalisation_layouts_and_slots(E):
    from ladcast_amd import hip

    M, C, L, H, W = 3, 2, 2, 3, 8
    c = R.case((M, C, L, H, W))
    g = np.random.RandomState(3)
    mean, std, ts = np.array([280.0, 5.0e4], np.float32), np.array([12.0, 900.0], np.float32), 0.5
    v = (ts * g.standard_normal((M, C, L, H, W))).astype(np.float32)  # normalised forecast
    w = c["w"]
    vd, td, wd, md, sd = dev(v), dev(c["t"]), dev(w), dev(mean), dev(std)
    fused = host(E.rollout_spectrum(vd, td, wd, mean=md, std=sd, target_std=ts))
    phys = torch.empty_like(vd)
    hip.chan_affine(vd, phys, md, sd, ts, outer=M, C=C, inner=L * H * W, inverse=True)
    first = host(E.rollout_spectrum(phys, td, wd))
    assert same(fused, first), "fused inverse normalisation against ldc_chan_affine(inverse=1) first"
    xp = R.inv_norm_f32(v, mean, std, ts)
    assert np.array_equal(xp.view(np.int32), phys.cpu().numpy().view(np.int32))
    R.check(fused, R.spectrum_ref(xp, c["t"], w), "fused")
    frames = vd.permute(2, 0, 1, 3, 4).contiguous()  # the decoder's frame-major layout
    assert same(fused, host(E.rollout_spectrum(frames, td, wd, lead_dim=0, mean=md, std=sd, target_std=ts))), "lead_dim=0"
    table = torch.full((5, C, H, W), float("nan"), device="cuda")  # lead 0 in slot 3, lead 1 in slot 1
    table[3], table[1] = td[:, 0], td[:, 1]
    assert same(fused, host(E.rollout_spectrum(frames, table, wd, lead_dim=0, mean=md, std=sd, target_std=ts, truth_slot=[3, 1]))), "truth_slot"


# ---- d. NaN and weights ------------------------------------------------------------------------------------------------------------------
def test_nan_rows_and_zero_weight_rows(E):
    clean = R.case((3, 2, 2, 3, 8))
    base = run(E, clean["x"], clean["t"], clean["w"])
    c = R.nan_case(False)  # a NaN in member 1 of row 1 of (c, l) = (1, 0)
    got = run(E, c["x"], c["t"], c["w"])
    R.check(got, R.spectrum_ref(c["x"], c["t"], c["w"]), "NaN row")
    assert got["n_invalid"].tolist() == [[0, 0], [1, 0]] and all(np.isfinite(got[k]).all() for k in R.NAMES)
    for k in R.NAMES:  # only that (c, l) moves
        assert np.array_equal(got[k][0], base[k][0]) and np.array_equal(got[k][1, 1], base[k][1, 1]) and not np.array_equal(got[k][1, 0], base[k][1, 0])
    z = R.nan_case(True)  # the same NaN (and an inf beside it) in a row of weight 0: not one bit moves, nothing is counted
    zx = z["x"].copy()
    zx[0, :, :, 1, 2] = np.inf
    zt = z["t"].copy()
    zt[:, :, 1, 0] = np.nan
    assert same(run(E, zx, zt, z["w"]), run(E, clean["x"], clean["t"], z["w"]))
    assert run(E, zx, zt, z["w"])["n_invalid"].tolist() == [[0, 0], [0, 0]]
    x = clean["x"].copy()
    x[0, 0, 0, :, 0] = np.nan  # every row of (c, l) = (0, 0)
    w = clean["w"].copy()
    w[2] = 0.0  # ... of which two have positive weight
    got = run(E, x, clean["t"], w)
    assert got["n_invalid"].tolist() == [[2, 0], [0, 0]] and all(np.isnan(got[k][0, 0]).all() and np.isfinite(got[k][0, 1]).all() for k in R.NAMES)
    R.check(got, R.spectrum_ref(x, clean["t"], w), "no valid row")
    tn = clean["t"].copy()
    tn[1, 1, 0, 7] = np.nan  # a NaN in the truth alone
    got = run(E, clean["x"], tn, clean["w"])
    assert got["n_invalid"].tolist() == [[0, 0], [0, 1]]
    R.check(got, R.spectrum_ref(clean["x"], tn, clean["w"]), "NaN truth")


# ---- e. l_off, guard bands, workspace ------------------------------------------------------------------------------------------------------
def test_l_off_columns(E):
    M, C, L, H, W = 2, 2, 4, 3, 8
    c = R.case((M, C, L, H, W))
    xd, td, wd = dev(c["x"]), dev(c["t"]), dev(c["w"])
    whole = host(E.rollout_spectrum(xd, td, wd))
    R.check(whole, R.spectrum_ref(c["x"], c["t"], c["w"]), "four lead times")
    out = E.empty_spectrum(C, L, W, "cuda")
    out._buffers[0].view(torch.int32).fill_(UNWRITTEN32)
    out._buffers[1].fill_(-77)
    before = host(out)
    part = host(E.rollout_spectrum(xd[:, :, 1:3], td[:, 1:3], wd, out=out, l_off=1))
    for k in R.NAMES:
        for col in (0, 3):
            assert np.array_equal(part[k][:, col].view(np.int32), before[k][:, col].view(np.int32)), (k, col)
        assert np.array_equal(part[k][:, 1:3].view(np.int32), whole[k][:, 1:3].view(np.int32)), k
    assert (part["n_invalid"][:, [0, 3]] == -77).all() and (part["n_invalid"][:, 1:3] == 0).all()
    two = E.rollout_spectrum(xd[:, :, :2], td[:, :2], wd, out=E.empty_spectrum(C, L, W, "cuda"), l_off=0)
    two = host(E.rollout_spectrum(xd[:, :, 2:], td[:, 2:], wd, out=two, l_off=2))
    assert same(two, whole), "two launches (l_off 0, then 2) against one of 4"
    fresh = host(E.rollout_spectrum(xd[:, :, 2:], td[:, 2:], wd, l_off=2))  # unwritten columns of a fresh result: NaN, n_invalid 0
    assert all(np.isnan(fresh[k][:, :2]).all() for k in R.NAMES) and (fresh["n_invalid"][:, :2] == 0).all()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _unwritten(t):
    return bool((t.detach().cpu().contiguous().view(torch.int32) == UNWRITTEN32).all())


@pytest.mark.parametrize("layout", ["ens_C_L_H_W", "frame_major"])
@pytest.mark.parametrize("shape", [(3, 2, 2, 11, 6), (2, 1, 1, 2, 512), (9, 1, 2, 3, 240)], ids=str)
def test_guard_bands(shape, layout):
    from ladcast_amd import hip

    M, C, L, H, W = shape
    K, HW, ld, N_TRUTH = W // 2 + 1, H * W, H * W + 8, 4
    c = R.case(shape)
    FMAX = 0x7F7FFFFF
    inp = dict(poison=FMAX, unwritten=False)  # NaN is a legal input: inputs are poisoned with the largest finite fp32
    mean, std, ts = np.linspace(-1.0, 2.0, C).astype(np.float32), np.linspace(0.75, 1.5, C).astype(np.float32), 0.5
    x = torch.from_numpy(c["x"])
    if layout == "ens_C_L_H_W":
        gf = guarded(C * L, HW, ld, batch=M, batch_stride=C * L * ld + 24, **inp).fill(x.reshape(M, C * L, HW))
        ms, cs, ls = gf.bs, L * ld, ld
    else:
        gf = guarded(M * C, HW, ld, batch=L, batch_stride=M * C * ld + 24, **inp).fill(x.permute(2, 0, 1, 3, 4).reshape(L, M * C, HW))
        ls, ms, cs = gf.bs, C * ld, ld
    slots = [(2 * l + 1) % N_TRUTH for l in range(L)]
    table = np.zeros((N_TRUTH, C, H, W), np.float32)
    for l, s in enumerate(slots):
        table[s] = c["t"][:, l]
    gt = guarded(C, HW, ld, batch=N_TRUTH, batch_stride=C * ld + 16, **inp).fill(torch.from_numpy(table).reshape(N_TRUTH, C, HW))
    w = c["w"].copy()
    w[H // 2] = 0.0
    gl = guarded(1, H, **inp).fill(torch.from_numpy(w))
    gts = guarded(1, L, dtype=torch.int32, poison=N_TRUTH, unwritten=False).fill(torch.tensor(slots))
    gm, gs = guarded(1, C, **inp).fill(torch.from_numpy(mean)), guarded(1, C, **inp).fill(torch.from_numpy(std))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lt = L + 2
    nbytes = int(hip.lib.ldc_rollout_spectrum_workspace_bytes(M, C, L, H, W))
    assert nbytes == R.workspace_bytes(M, C, L, H, W) and nbytes % 4 == 0
    gw = guarded(1, nbytes // 4, unwritten=False)
    go, gn = guarded(3 * C * Lt, K), guarded(C, Lt, dtype=torch.int32)

    def call(nb):
        st = hip.lib.ldc_rollout_spectrum(_p(gf.view), ms, ls, cs, _p(gm.view), _p(gs.view), ts, _p(gt.view), gt.bs, ld, _p(gts.view), _p(gl.view), M, C, L, H,
                                          W, _p(go.view), _p(gn.view), Lt, 1, _p(gw.view), nb, stream)
        torch.cuda.synchronize()
        return st

    assert call(nbytes - 1) == -1 and _unwritten(go.payload()) and _unwritten(gn.payload())  # LDC_ERR_ARG, nothing written
    assert call(nbytes) == 0
    for k, g in dict(forecast=gf, truth=gt, row_weight=gl, truth_slot=gts, mean=gm, std=gs, workspace=gw, out=go, n_invalid=gn).items():
        assert_untouched(g, k)
    out, ninv = go.payload()[0].reshape(3, C, Lt, K), gn.payload()[0].reshape(C, Lt)
    for col in (0, L + 1):  # the columns outside l_off .. l_off + L - 1 keep their first bits
        assert _unwritten(out[:, :, col]) and _unwritten(ninv[:, col])
    xp = R.inv_norm_f32(c["x"], mean, std, ts)
    got = dict(n_invalid=ninv[:, 1:L + 1].numpy(), **{k: out[i, :, 1:L + 1].numpy() for i, k in enumerate(R.NAMES)})
    r = R.check(got, R.spectrum_ref(xp, c["t"], w), f"{shape} {layout}")
    print(f"guard bands {shape} {layout}: worst err / bound {r:.4f}")


# ---- g. arguments ------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_launch_nothing(E):
    from ladcast_amd import hip

    C, L, H = 1, 1, 4
    big = torch.zeros(1025 * C * L * H * 514, device="cuda")
    t, w, slot = torch.zeros(C * L * H * 514, device="cuda"), torch.ones(H, device="cuda"), torch.zeros(L, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gw = guarded(1, 1 << 16, unwritten=False)
    ARG, UNSUPPORTED = -1, -3

    def call(M=5, W=8, nbytes=1 << 18, L_total=L, l_off=0, null=None, C_=C, L_=L):
        K = W // 2 + 1 if W > 0 else 1
        go, gn = guarded(3 * C * L, K), guarded(C, L, dtype=torch.int32)
        ptr = dict(forecast=_p(big), truth=_p(t), slot=_p(slot), w=_p(w), out=_p(go.view), n=_p(gn.view), ws=_p(gw.view))
        if null:
            ptr[null] = None
        st = hip.lib.ldc_rollout_spectrum(ptr["forecast"], C * L * H * max(W, 1), H * max(W, 1), L * H * max(W, 1), None, None, 1.0, ptr["truth"], H * max(W, 1),
                                          L * H * max(W, 1), ptr["slot"], ptr["w"], M, C_, L_, H, W, ptr["out"], ptr["n"], L_total, l_off, ptr["ws"], nbytes,
                                          stream)
        torch.cuda.synchronize()
        untouched = _unwritten(go.payload()) and _unwritten(gn.payload())
        for g in (go, gn, gw):
            assert_untouched(g)
        return st, untouched

    q = hip.lib.ldc_rollout_spectrum_workspace_bytes
    need = int(q(5, C, L, H, 8))
    assert need == R.workspace_bytes(5, C, L, H, 8)
    for M, W in ((0, 8), (1025, 8), (5, 7), (5, 2), (5, 514), (5, 0)):
        assert q(M, C, L, H, W) == 0
    assert q(5, 65536, L, H, 8) == 0 and q(5, C, 65536, H, 8) == 0
    for kw in (dict(M=0), dict(M=-3), dict(W=0), dict(L_total=0), dict(l_off=-1), dict(l_off=1), dict(nbytes=need - 1), dict(null="forecast"),
               dict(null="truth"), dict(null="slot"), dict(null="w"), dict(null="out"), dict(null="n"), dict(null="ws")):
        assert call(**kw) == (ARG, True), kw
    for kw in (dict(M=1025), dict(W=7), dict(W=2), dict(W=514), dict(C_=65536), dict(L_=65536, L_total=65536)):
        assert call(**kw) == (UNSUPPORTED, True), kw
    assert call(nbytes=need) == (0, False) and call(M=1024, W=512) == (0, False)
    x5 = big[: 5 * C * L * H * 8].view(5, C, L, H, 8)
    with pytest.raises(RuntimeError, match="ldc_rollout_spectrum"):
        out = E.empty_spectrum(C, L, 8, "cuda")
        hip.rollout_spectrum(x5, t, slot, w, *out._buffers, M=1025, C=C, L=L, H=H, W=8, member_stride=x5.stride(0), lead_stride=x5.stride(2),
                             channel_stride=x5.stride(1), truth_slot_stride=H * 8, truth_channel_stride=L * H * 8, L_total=L)
    with pytest.raises(ValueError, match="non-negative"):  # a host weight is checked; a device weight is the caller's
        E.rollout_spectrum(x5, t[: C * L * H * 8].view(C, L, H, 8), torch.tensor([1.0, -1.0, 1.0, 1.0]))
    with pytest.raises(RuntimeError):
        E.rollout_spectrum(x5.cpu(), t[: C * L * H * 8].view(C, L, H, 8), w)  # device tensors only


# ---- h. the driver -------------------------------------------------------------------------------------------------------------------------
NEW = ("spec_members", "spec_mean", "spec_truth", "spec_n_invalid")


def test_driver_spectrum_flag(tmp_path):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate import rollout_spectrum
    from ladcast_amd.models import AutoencoderDC
    from ladcast_amd.pipelines.io import save_latent_npy
    from ladcast_amd.pipelines.utils import inverse_normalize_transform_3D
    from tests.synth import tiny_dcae_config

    ENS, C_LAT, T, h, w_, C, H, W, SST = 5, 8, 3, 6, 8, 8, 48, 64, 3
    K = W // 2 + 1
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
    truth[:, SST][:, torch.rand(H, W, generator=gen) < 0.02] = float("nan")  # land: some rows of the SST channel are left out
    np.save(tmp_path / "truth.npy", truth.numpy())
    clim = np.lib.format.open_memmap(tmp_path / "clim.npy", mode="w+", dtype=np.float32, shape=(366, 4, C, H, W))  # sparse: zeros
    clim.flush()
    del clim
    BAND = (-30.0, 45.0)

    def run_cli(flag, name):
        argv = ["--normalization_json", str(tmp_path / "norm.json"), "--encdec_model", str(tmp_path / "config.json"), "--data_path", str(tmp_path / "truth.npy"),
                "--result_path", str(tmp_path / "rollout"), "--climatology_path", str(tmp_path / "clim.npy"), "--start_date", "2020-02-27",
                "--end_date", "2020-02-29T12", "--output", str(tmp_path / name), "--total_lead_time_hour", "18", "--crop_init",
                "--sst_channel_idx", str(SST), "--variable_names", *names] + (["--spectrum", "--spectrum_lat_band", str(BAND[0]), str(BAND[1])] if flag else [])
        torch.manual_seed(1234)  # the weights the command line's from_config draws
        with pytest.warns(UserWarning):
            EG.main(argv)
        return tmp_path / name

    plain, spec = run_cli(False, "plain"), run_cli(True, "spec")
    assert sorted(p.name for p in spec.iterdir()) == sorted([p.name for p in plain.iterdir()] + [f"{k}.npy" for k in NEW])
    for p in plain.iterdir():  # the five scores (and the time stamps) bit for bit
        assert (spec / p.name).read_bytes() == p.read_bytes(), p.name
    a = {k: np.load(spec / f"{k}.npy") for k in NEW}
    assert all(a[k].shape == (2, C, T, K) and a[k].dtype == np.float32 for k in NEW[:3]) and a["spec_n_invalid"].shape == (2, C, T) and a["spec_n_invalid"].dtype == np.int32
    # the oracle, and rollout_spectrum itself, on the fields the product decoder returns for the same frame batches, de-normalised first
    torch.manual_seed(1234)
    model = AutoencoderDC.from_config(tiny_dcae_config()).cuda().eval()
    mean32, std32 = torch.tensor([float(v) for v in mean]), torch.tensor([float(v) for v in std])
    lat_w = EG.lat_weights_for(H)
    band_w = EG.spectrum_band_weights(lat_w, EG.row_latitudes(H), BAND)
    assert 0 < int((band_w > 0).sum()) < H
    for n in range(2):
        phys = torch.stack([inverse_normalize_transform_3D(model.decode(latents[n, :, :, 1 + l].contiguous().cuda()).sample.reshape(ENS, C, 1, H, W),
                                                           mean32, std32).reshape(ENS, C, H, W) for l in range(T)], dim=2)  # (ENS, C, T, H, W)
        tr = truth[6 + n + 1:6 + n + 1 + T].permute(1, 0, 2, 3).contiguous()  # (C, T, H, W)
        ref = R.spectrum_ref(phys.cpu().numpy(), tr.numpy(), band_w.numpy())
        cli = dict(n_invalid=a["spec_n_invalid"][n], **{k: a[k][n] for k in R.NAMES})
        r = R.check(cli, ref, f"init {n}: the command line")
        direct = host(rollout_spectrum(phys, tr.cuda(), band_w.cuda()))
        R.check(direct, ref, f"init {n}: rollout_spectrum on the de-normalised fields")
        print(f"init {n}: worst err / bound {r:.4f}; bit-equal to rollout_spectrum on the de-normalised fields: {same(cli, direct)}")
        assert int(ref["n_invalid"][SST].sum()) > 0 and int(np.delete(ref["n_invalid"], SST, axis=0).sum()) == 0
    # score_latent_rollout: the five scores bit for bit, the default row weight is lat_weight
    kw = dict(sst_channel=SST, crop_init=True)
    tabs = (truth.cuda(), [7, 8, 9], torch.zeros(3, C, H, W, device="cuda"), [0, 1, 2], lat_w)
    off = EG.score_latent_rollout(latents[0], model, mean32, std32, *tabs, **kw)
    on = EG.score_latent_rollout(latents[0], model, mean32, std32, *tabs, spectrum=True, reliability=True, **kw)
    rel = EG.score_latent_rollout(latents[0], model, mean32, std32, *tabs, reliability=True, **kw)
    assert set(on) == set(rel) | set(NEW) and not set(off) & set(NEW)
    for k in off:
        assert torch.equal(off[k].view(torch.int32), on[k].view(torch.int32)), k
    for k in rel:
        assert torch.equal(rel[k].view(torch.int32) if rel[k].dtype == torch.float32 else rel[k], on[k].view(torch.int32) if on[k].dtype == torch.float32 else on[k]), k
    phys = torch.stack([inverse_normalize_transform_3D(model.decode(latents[0, :, :, 1 + l].contiguous().cuda()).sample.reshape(ENS, C, 1, H, W),
                                                       mean32, std32).reshape(ENS, C, H, W) for l in range(T)], dim=2)
    ref = R.spectrum_ref(phys.cpu().numpy(), truth[7:10].permute(1, 0, 2, 3).numpy(), lat_w.numpy())
    R.check(dict(n_invalid=on["spec_n_invalid"].numpy(), **{k: on[k].numpy() for k in R.NAMES}), ref, "score_latent_rollout(spectrum=True)")
