"""Sphere fields on the device: `ldc_derive_sphere` through `derive_forecast` / `derive_table` against the host reference
(tests/sphere_refs.py), and the two drivers (`score_latent_rollout`, `products_of_latent_rollout`) with `derived=` on the tiny DC-AE of
tests/test_gpu_evaluate_ens.py.

Bounds.  A non-pole row is the same IEEE double operations in the same order as the reference, from inputs that hold the reference's
bits, rounded once to fp32: bit-equal (+0 and -0 compare equal, NaN equals NaN).  A pole row is a sum of W doubles in the wave's
fixed order against `math.fsum`: a recursive or tree sum of W terms errs at most (W - 1) 2^-53 sum|a_i|; divided by W, times |pc|,
plus the one rounding to fp32 (which can move the result to the neighbouring fp32 value): 1 fp32 ulp + (W - 1) 2^-53 sum|a_i| |pc| / W.
The tests print how many elements differ at all.

Grids: (2, 3) the smallest; (3, 5) odd, scalar path; (4, 8) the 16-byte path within one workgroup of four rows; (5, 64) one 16-byte
step per lane for a quarter of a wave, W one wave for the pole sum, H above the four rows of a workgroup; (6, 70) W % 4 != 0 above one
wave with a ragged tail of 6; (37, 12) many workgroups, a last one of one row; (3, 260) W above the 256 longitudes a wave covers in one
16-byte step, so the 16-byte loop runs twice for lane 0."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import derived_refs as R
from tests import sphere_refs as SR
from tests.redzone import assert_untouched, guarded
from tests.test_gpu_derived import NO_CHANNEL, _decode, _rows
from tests.test_gpu_evaluate_ens import C, ENS, H, KEYS, SST, T, TRUTH_SLOTS, W, _same_bits, setup  # noqa: F401

pytestmark = pytest.mark.gpu

GRIDS = [(2, 3), (3, 5), (4, 8), (5, 64), (6, 70), (37, 12), (3, 260)]
Z, DV, DV2 = ("z", "vorticity", (0, 1)), ("dv", "divergence", (3, 1)), ("dv", "divergence", (0, 1))


def _lats(Hh):
    """with both poles, with the north pole only (the drivers' rows), with none, descending (the pole first)"""
    return dict(both=np.linspace(-90.0, 90.0, Hh), north=np.linspace(-90.0, 90.0, Hh + 1)[1:], none=np.linspace(-80.0, 77.0, Hh),
                descending=np.linspace(-90.0, 90.0, Hh + 1)[1:][::-1].copy())


def _check(got, x, fields, axis, lat, mean=None, std=None, target_std=1.0, what=""):
    """got: the device result with the fields on `axis`; x: the fp32 source on the host with the channels on `axis`, (H, W) last"""
    from ladcast_amd.evaluate import sphere_row_tables

    got, x = got.detach().cpu().numpy(), np.asarray(x, dtype=np.float32)
    assert got.dtype == np.float32
    tab, k = sphere_row_tables(lat, x.shape[-1])
    poles = SR.pole_rows(tab)
    rows = [j for j in range(x.shape[-2]) if j not in poles]
    n_diff = n_pole = 0
    for n, f in enumerate(fields):
        u, v = (R.denorm(np.take(x, c, axis=axis), None if mean is None else float(mean[c]), None if std is None else float(std[c]), target_std) for c in f[2])
        want, g = SR.field(f[1], u, v, tab, k), np.take(got, n, axis=axis)
        assert g.shape == want.shape, (what, g.shape, want.shape)
        d = R.ulp_distance(g[..., rows, :], want[..., rows, :])
        assert int(d.max(initial=0)) == 0, (what, f, "a non-pole row differs", int(d.max()), int((d != 0).sum()))
        for j in poles:
            jp = 1 if j == 0 else x.shape[-2] - 2
            a = u if f[1] == "vorticity" else v
            bound = SR.pole_bound(a[..., jp, :], tab[3][j], want[..., j, 0])[..., None]
            gj, wj = g[..., j, :].astype(np.float64), want[..., j, :].astype(np.float64)
            fin = np.isfinite(wj)
            assert np.array_equal(np.isnan(gj), np.isnan(wj)) and np.array_equal(gj[~fin & ~np.isnan(wj)], wj[~fin & ~np.isnan(wj)]), (what, f, j)
            with np.errstate(invalid="ignore"):  # inf - inf where the reference is not finite: masked out
                err = np.abs(gj - wj)
            assert bool((err[fin] <= np.broadcast_to(bound, wj.shape)[fin]).all()), (what, f, j, float(err[fin].max()))
            assert bool((R.ulp_distance(g[..., j, :], g[..., j, :1]) == 0).all()), (what, f, j, "a pole row is one value")
            n_diff += int((R.ulp_distance(g[..., j, :], want[..., j, :]) != 0).sum())
            n_pole += gj.size
    if n_diff:
        print(f"{what}: {n_diff} of {n_pole} pole-row elements differ from the fsum reference (every non-pole element is bit-equal)")


# ---- 1. shapes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead_dim", [0, 2])
@pytest.mark.parametrize("hw", GRIDS)
def test_derive_forecast_grids_latitudes_and_strides(hw, lead_dim):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), Cc = hw, 5
    fields = [Z, DV, ("again", "vorticity", (4, 4))]
    for M, L in ((1, 1), (3, 1), (1, 3), (3, 3)):
        g = torch.Generator().manual_seed(3 + 7 * M + L)
        # a slice of a larger tensor: member, lead and channel strides all differ from the dense ones
        big = (torch.randn((M + 1, Cc + 2, L + 1, Hh, Ww) if lead_dim == 2 else (L + 1, M + 1, Cc + 2, Hh, Ww), generator=g) * 20.0).cuda()
        view = big[1:, 1 : 1 + Cc, :L] if lead_dim == 2 else big[:L, 1:, 1 : 1 + Cc]
        mean, std = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
        ax = 1 if lead_dim == 2 else 2
        for name, lat in _lats(Hh).items():
            for target_std in (1.0, 0.5):
                got = derive_forecast(view, fields, lead_dim=lead_dim, mean=mean.cuda(), std=std.cuda(), target_std=target_std, lat_deg=lat)
                assert got.shape == ((M, 3, L, Hh, Ww) if lead_dim == 2 else (L, M, 3, Hh, Ww)) and got.is_contiguous()
                _check(got, view.cpu().numpy(), fields, ax, lat, mean.numpy(), std.numpy(), target_std, f"{hw} M={M} L={L} {name} target_std={target_std}")
            phys = derive_forecast(view, fields[:2], lead_dim=lead_dim, lat_deg=torch.from_numpy(lat))  # no mean: physical, its bits are taken as they are
            _check(phys, view.cpu().numpy(), fields[:2], ax, lat, what=f"{hw} M={M} L={L} {name} physical")
    if Hh == 5:  # lat_deg None: the rows the drivers score on
        from ladcast_amd.evaluate.rollout_metrics import row_latitudes

        _check(derive_forecast(view, fields, lead_dim=lead_dim), view.cpu().numpy(), fields, ax, row_latitudes(Hh), what="default latitudes")


@pytest.mark.parametrize("hw", [(4, 8), (5, 64)])
@pytest.mark.parametrize("offset", [0, 1, 3])  # elements: 1 and 3 leave every plane base off the 16-byte grid while W % 4 == 0
def test_odd_storage_offsets(offset, hw):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), M, Cc, L = hw, 2, 6, 2
    g = torch.Generator().manual_seed(17 + offset)
    flat = torch.randn(offset + M * Cc * L * Hh * Ww, generator=g).cuda()
    view = flat[offset:].view(M, Cc, L, Hh, Ww)
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    fields = [(f"f{n}", ("vorticity", "divergence")[n % 2], (n % Cc, (2 * n + 1) % Cc)) for n in range(16)]  # D = 16, channels shared
    for name, lat in _lats(Hh).items():
        got = derive_forecast(view, fields, lat_deg=lat)
        _check(got, view.cpu().numpy(), fields, 1, lat, what=f"{hw} offset {offset} {name}")
    oflat = torch.zeros(offset + M * 16 * L * Hh * Ww).cuda()  # an aligned source with an out off the 16-byte grid
    out = oflat[offset:].view(M, 16, L, Hh, Ww)
    src = view.clone()
    assert derive_forecast(src, fields, lat_deg=lat, out=out).data_ptr() == out.data_ptr()
    _check(out, src.cpu().numpy(), fields, 1, lat, what=f"{hw} out offset {offset}")


# ---- 2. values -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 64), (6, 70), (3, 5)])
def test_divergence_is_vorticity_of_minus_v_u(hw):
    from ladcast_amd.evaluate import derive_forecast

    Hh, Ww = hw
    g = torch.Generator().manual_seed(31)
    uv = torch.randn(3, 2, 2, Hh, Ww, generator=g) * 15.0
    x = torch.cat([uv, -uv[:, 1:2]], dim=1).cuda()  # channels u, v, -v
    for name, lat in _lats(Hh).items():
        got = derive_forecast(x, [("d", "divergence", (0, 1)), ("z", "vorticity", (2, 0))], lat_deg=lat).cpu()
        assert torch.equal(got[:, 0].view(torch.int32), got[:, 1].view(torch.int32)), (hw, name)


@pytest.mark.parametrize("offset", [0, 1])  # the 16-byte path and the scalar path
def test_special_values(offset):
    from ladcast_amd.evaluate import derive_forecast

    Hh, Ww = 6, 8
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(37)
    base = torch.randn(1, 2, 1, Hh, Ww, generator=g) * 10.0
    lats = _lats(Hh)

    def run(x, lat, fields=(Z,)):
        flat = torch.empty(offset + x.numel()).cuda()
        view = flat[offset:].view(x.shape)
        view.copy_(x)
        got = derive_forecast(view, list(fields), lat_deg=lat)
        _check(got, x.numpy(), list(fields), 1, lat, what=f"special values, offset {offset}")
        return got[0, :, 0].cpu()

    clean = run(base, lats["none"])[0]
    # u is a (read at j +- 1, same column), v is b (read at i +- 1, same row, wrapped); an edge row's one-sided form reads its own row
    cases = [((0, 3, 2), [(2, 2), (4, 2)]), ((1, 3, 2), [(3, 1), (3, 3)]), ((1, 2, 0), [(2, 1), (2, Ww - 1)]), ((1, 2, Ww - 1), [(2, Ww - 2), (2, 0)]),
             ((0, 0, 5), [(0, 5), (1, 5)]), ((0, Hh - 1, 5), [(Hh - 1, 5), (Hh - 2, 5)]), ((1, 0, 0), [(0, 1), (0, Ww - 1)]), ((0, 2, Ww - 1), [(1, Ww - 1), (3, Ww - 1)])]
    for (ch, j, i), hit in cases:
        x = base.clone()
        x[0, ch, 0, j, i] = nan
        z = run(x, lats["none"])[0]
        want = torch.zeros(Hh, Ww, dtype=torch.bool)
        for p in hit:
            want[p] = True
        assert torch.equal(torch.isnan(z), want), (ch, j, i)
        assert torch.equal(z[~want].view(torch.int32), clean[~want].view(torch.int32)), (ch, j, i)
    # pole rows: a NaN anywhere in row jp poisons the whole pole row; the pole row's own values are read by its neighbour only
    x = base.clone()
    x[0, 0, 0, Hh - 2, 3] = nan
    z = run(x, lats["both"])[0]
    want = torch.zeros(Hh, Ww, dtype=torch.bool)
    want[Hh - 1, :] = True
    want[Hh - 3, 3] = True
    assert torch.equal(torch.isnan(z), want)
    x = base.clone()
    x[0, 1, 0, 1, 6] = nan  # v is not summed for the vorticity's pole row, but it is for the divergence's
    zd = run(x, lats["both"], (Z, DV2))
    assert not bool(torch.isnan(zd[0][0]).any()) and bool(torch.isnan(zd[1][0]).all()) and not bool(torch.isnan(zd[1][Hh - 1]).any())
    # +-inf follows IEEE: inf - inf is NaN, inf alone stays inf with the sign the formula gives (the reference does the same operations)
    x = base.clone()
    x[0, 0, 0, 2, 1], x[0, 0, 0, 4, 1], x[0, 1, 0, 3, 4], x[0, 0, 0, 1, 7], x[0, 1, 0, 0, 0] = inf, inf, -inf, -inf, 3.0e38
    z = run(x, lats["none"])[0]
    assert math.isnan(float(z[3, 1])) and bool(torch.isinf(z[3, 3])) and bool(torch.isinf(z[3, 5])) and float(z[3, 3]) == -float(z[3, 5])
    x = base.clone()
    x[0, 0, 0, 1, 2], x[0, 0, 0, Hh - 2, 0], x[0, 0, 0, Hh - 2, 4] = inf, inf, -inf
    z = run(x, lats["both"])[0]
    assert bool(torch.isinf(z[0]).all()) and bool(torch.isnan(z[Hh - 1]).all())


# ---- 3. tables -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(3, 5), (4, 8), (6, 70)])
def test_derive_table(hw):
    from ladcast_amd.evaluate import derive_table

    (Hh, Ww), N, Cc = hw, 5, 7
    g = torch.Generator().manual_seed(23)
    table = (torch.randn(N, Cc, Hh, Ww, generator=g) * 30.0).cuda()
    fields = [Z, ("dv", "divergence", (5, 6))]
    slots = [3, 0, 3, 1]  # out of order and repeated
    lat = _lats(Hh)["north"]
    host = table.cpu().numpy()
    got = derive_table(table, slots, fields)  # the default latitudes are these
    assert got.shape == (4, 2, Hh, Ww)
    _check(got, host[slots], fields, 1, lat, what="slots")
    _check(derive_table(table, torch.tensor(slots), fields, lat_deg=_lats(Hh)["descending"]), host[slots], fields, 1, _lats(Hh)["descending"], what="tensor slots")
    for bad in ([0, 5], [-1], []):
        with pytest.raises(ValueError):
            derive_table(table, bad, fields)
    clt = table.permute(1, 0, 2, 3).contiguous()  # (C, L, H, W), no slots
    _check(derive_table(clt, None, fields, lat_deg=lat), host, fields, 1, lat, what="no slots")
    _check(derive_table(table.permute(1, 0, 2, 3), None, fields, lat_deg=_lats(Hh)["both"]), host, fields, 1, _lats(Hh)["both"], what="no slots, a permuted view")


# ---- 4. writes stay where they belong; mixed lists -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("hw", [(3, 5), (4, 8), (6, 70)])
def test_out_as_tail_channels_keeps_head_and_guards(hw, offset):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), L, M, Cc = hw, 2, 3, 6
    fields = [Z, ("dv", "divergence", (5, 3)), ("z2", "vorticity", (2, 4))]
    n = L * M * (Cc + 3) * Hh * Ww
    buf = guarded(1, offset + n)
    flat = buf.view[0, 0]
    flat[:offset] = 123.0
    ext = flat[offset:].view(L, M, Cc + 3, Hh, Ww)  # lead-major, as the drivers' buffer
    g = torch.Generator().manual_seed(29)
    head = torch.randn(L, M, Cc, Hh, Ww, generator=g)
    ext[:, :, :Cc] = head.cuda()
    mean, std = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    lat = _lats(Hh)["both"]
    out = derive_forecast(ext[:, :, :Cc], fields, lead_dim=0, mean=mean.cuda(), std=std.cuda(), out=ext[:, :, Cc:], lat_deg=lat)
    assert out.data_ptr() == ext[:, :, Cc:].data_ptr()
    assert_untouched(buf, f"derive_forecast {hw} offset {offset}")
    assert torch.equal(ext[:, :, :Cc].cpu(), head) and bool((flat[:offset].cpu() == 123.0).all())
    _check(ext[:, :, Cc:], head.numpy(), fields, 2, lat, mean.numpy(), std.numpy(), what="tail")


@pytest.mark.parametrize("hw", [(3, 5), (5, 64)])
def test_mixed_list_keeps_each_fields_bits(hw):
    from ladcast_amd.evaluate import derive_forecast

    (Hh, Ww), L, M, Cc = hw, 2, 3, 6
    g = torch.Generator().manual_seed(43)
    x = (torch.randn(L, M, Cc, Hh, Ww, generator=g) * 8.0).cuda()
    mean, std = torch.randn(Cc, generator=g).cuda(), (torch.rand(Cc, generator=g) + 0.5).cuda()
    fields = [("s", "speed", (0, 1)), Z, ("d", "diff", (2, 4)), ("dv", "divergence", (0, 1))]
    kw = dict(lead_dim=0, mean=mean, std=std, lat_deg=_lats(Hh)["north"])
    buf = guarded(1, L * M * 4 * Hh * Ww)
    out = buf.view[0, 0].view(L, M, 4, Hh, Ww)
    derive_forecast(x, fields, out=out, **kw)
    assert_untouched(buf, f"mixed list {hw}")
    for n, f in enumerate(fields):
        alone = derive_forecast(x, [f], **kw)
        assert torch.equal(out[:, :, n].view(torch.int32), alone[:, :, 0].view(torch.int32)), f
    swapped = derive_forecast(x, [fields[1], fields[3], fields[0], fields[2]], **kw)  # two runs of two
    for n, m in enumerate((1, 3, 0, 2)):
        assert torch.equal(swapped[:, :, n].view(torch.int32), out[:, :, m].view(torch.int32))


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from ladcast_amd import hip
    from ladcast_amd.evaluate import derive_forecast, derive_table, sphere_row_tables

    x = torch.randn(2, 4, 1, 4, 8)
    with pytest.raises(RuntimeError):
        derive_forecast(x, [Z])  # host tensors
    with pytest.raises(RuntimeError):
        derive_table(x[0], None, [Z])
    with pytest.raises(RuntimeError):
        derive_forecast(x.cuda(), [Z], mean=torch.zeros(4), std=torch.ones(4))
    with pytest.raises(NotImplementedError):
        derive_forecast(x.cuda().half(), [Z])
    with pytest.raises(NotImplementedError):
        derive_table(x[0].cuda().half(), None, [Z])
    for bad in ([Z] * 17, [("z", "vorticity", (0, 4))], [("z", "divergence", (-1, 0))], [("z", "curl", (0, 1))], [("z", "vorticity", (0, 1, 2, 3))], []):
        with pytest.raises(ValueError):
            derive_forecast(x.cuda(), bad)
    for lat in ([0.0, 10.0, 20.0], [0.0, 10.0, 10.0, 20.0], [0.0, 30.0, 60.0, 91.0], [-90.0, 90.0, 0.0, 10.0], [0.0, 80.0, 90.0 - 5e-7, 90.0]):
        with pytest.raises(ValueError):  # the wrong count, not monotonic, out of range, a pole in the middle - on a host tensor too: before any device check
            derive_forecast(x, [Z], lat_deg=lat)
    with pytest.raises(ValueError):
        derive_forecast(torch.randn(2, 4, 1, 1, 8).cuda(), [Z], lat_deg=[0.0])  # H = 1
    with pytest.raises(ValueError):
        derive_forecast(torch.randn(2, 4, 1, 4, 2).cuda(), [Z])  # W = 2
    for bad_out in (torch.empty(2, 1, 1, 4, 8), torch.empty(2, 2, 1, 4, 8).cuda(), torch.empty(2, 1, 1, 8, 4).cuda().transpose(3, 4)):
        with pytest.raises((ValueError, RuntimeError)):
            derive_forecast(x.cuda(), [Z], out=bad_out)
    with pytest.raises(ValueError):
        derive_forecast(x.cuda(), [Z], lead_dim=1)
    # the C ABI itself: a wrong kind, a channel out of range, D outside 1 .. 16, H = 1, W = 2, a missing table
    lat = np.linspace(-90.0, 90.0, 5)[1:]
    tab, k = sphere_row_tables(lat, 8)
    tabd = torch.from_numpy(tab).cuda()
    xd, out = x.cuda(), torch.empty(2, 1, 1, 4, 8).cuda()
    out.fill_(7.0)
    keep = out.clone()

    def call(desc, n, Hh=4, Ww=8, table=tabd.data_ptr()):
        return hip.lib.ldc_derive_sphere(xd.data_ptr(), 128, 32, 32, None, None, None, 1.0, 2, 1, 4, Hh, Ww, table, k, desc, n, out.data_ptr(), 32, 32, 32, None)

    one = (hip.SphereDesc * 1)()
    one[0].kind, one[0].ch[0], one[0].ch[1] = 2, 0, 1
    assert call(one, 1) == -1  # LDC_ERR_ARG
    one[0].kind, one[0].ch[1] = hip.SPHERE_DIVERGENCE, 4
    assert call(one, 1) == -1
    one[0].ch[0], one[0].ch[1] = -1, 1
    assert call(one, 1) == -1
    many = (hip.SphereDesc * 17)()
    assert call(many, 17) == -1 and call(many, 0) == -1
    one[0].kind, one[0].ch[0], one[0].ch[1] = hip.SPHERE_VORTICITY, 0, 3
    assert call(one, 1, Hh=1) == -1 and call(one, 1, Ww=2) == -1 and call(one, 1, table=None) == -1
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), keep.view(torch.int32))  # nothing was launched
    assert call(one, 1) == 0
    torch.cuda.synchronize()
    _check(out, x.numpy(), [("z", "vorticity", (0, 3))], 1, lat, what="the C ABI")
    assert ctypes.sizeof(hip.SphereDesc) == hip.lib.ldc_sizeof_sphere_desc() == 12


# ---- 6. the drivers --------------------------------------------------------------------------------------------------------------------------
FIELDS = [("vort", "vorticity", (0, 1)), ("div", "divergence", (5, 6)), ("speed", "speed", (0, 1))]
D = len(FIELDS)


def _extended(s, y, t_slots, c_slots):
    """the extended batch by hand, from the public derive_* functions: forecast, truth, clim with the derived fields as tail channels"""
    from ladcast_amd.evaluate import derive_forecast, derive_table

    md, sd, td, cd = s["mean"].cuda(), s["std"].cuda(), s["truth"].cuda(), s["clim"].cuda()
    ext = torch.cat([y, derive_forecast(y, FIELDS, lead_dim=0, mean=md, std=sd)], dim=2)
    truth = torch.cat([td[t_slots], derive_table(td, t_slots, FIELDS)], dim=1)
    clim = torch.cat([cd[c_slots], derive_table(cd, c_slots, FIELDS)], dim=1)
    clim[:, C + 2] = float("nan")  # the speed: no climatology
    return ext, truth, clim


def _scales(s):
    st = [float(v) for v in s["std"]]
    return torch.tensor(st + [math.sqrt(st[0] ** 2 + st[1] ** 2) / 1.0e5, math.sqrt(st[5] ** 2 + st[6] ** 2) / 1.0e5, math.sqrt(st[0] ** 2 + st[1] ** 2)],
                        dtype=torch.float64)


def _options():
    from ladcast_amd.evaluate.energy import EnergyGroup
    from ladcast_amd.evaluate.regional import Region
    from ladcast_amd.evaluate.utils import Event

    events = [Event(0, "gt", 0.0), Event(C, "gt", 0.0, True), Event(C + 1, "lt", 0.0)]  # decoded; the vorticity's anomaly; the divergence
    return dict(reliability=True, spectrum=True, events=events, fss_radii=(0, 2), regions=[Region("box", -20.0, 20.0, 30.0, 120.0)], energy=True,
                energy_groups=[EnergyGroup("mixed", (2, C, C + 1)), EnergyGroup("decoded", (0, 1))])


@pytest.mark.parametrize("dbf", [3, 6])
def test_score_latent_rollout_with_sphere_fields(setup, dbf):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG
    from ladcast_amd.evaluate.rollout_metrics import METRICS, Batch
    from ladcast_amd.evaluate.utils import rollout_scores

    s = setup
    args = (s["latents"], s["g"], s["mean"], s["std"], s["truth"].cuda(), TRUTH_SLOTS, s["clim"].cuda(), s["clim_slots"], s["lat_w"])
    kw = dict(sst_channel=SST, crop_init=True, decode_batch_frames=dbf)
    opts = _options()
    got = EG.score_latent_rollout(*args, derived=FIELDS, **opts, **kw)
    plain = EG.score_latent_rollout(*args, **dict(opts, events=opts["events"][:1], energy_groups=opts["energy_groups"][1:]), **kw)
    assert all(got[k].shape == (C + D, T) for k in KEYS)
    # a. rows 0 .. C - 1: the bits of the call without derived fields, for the five scores and every optional metric
    for k, v in plain.items():
        if k in NO_CHANNEL or k.startswith("energy_group"):
            continue
        assert _same_bits(_rows(k, got[k], 0, C).double(), v.double()) and got[k].dtype == v.dtype, k
    for k in ("event_hist", "event_hist_weighted", "event_n_invalid", "event_fss_sums", "event_fss_n_invalid"):
        assert _same_bits(got[k][:1].double(), plain[k].double()), k
    for k in got:
        if k.startswith("energy_group"):
            assert _same_bits(got[k][1:].double(), plain[k].double()), k
    # b. every row: the bits of the scorers run on an extended batch built by hand
    per = max(1, dbf // ENS)
    scores = torch.full((5, C + D, T), float("nan"), device="cuda")
    o = dict(opts, spectrum_row_weight=None, region_mask=None, energy_scales=_scales(s), clim=s["clim"], std_tensor=None)
    metrics = [m for m in (cls.for_rollout(o) for cls in METRICS) if m is not None]
    lat_w = s["lat_w"].cuda()
    for m in metrics:
        m.start(lat_w)
    mean_e, std_e = torch.cat([s["mean"], torch.zeros(D)]).cuda(), torch.cat([s["std"], torch.ones(D)]).cuda()
    for s0 in range(0, T, per):
        nl = min(per, T - s0)
        ext, truth, clim = _extended(s, _decode(s, s0, nl), TRUTH_SLOTS[s0 : s0 + nl], s["clim_slots"][s0 : s0 + nl])
        b = Batch(ext, truth, lat_w, SST, T, dict(lead_dim=0, mean=mean_e, std=std_e, truth_slot=list(range(nl)), l_off=s0),
                  dict(clim=clim, clim_slots=list(range(nl))))
        rollout_scores(ext, truth, clim, lat_w, SST, lead_dim=0, mean=mean_e, std=std_e, truth_slots=list(range(nl)), clim_slots=list(range(nl)),
                       out=scores, lead_offset=s0)
        for m in metrics:
            m.run(b)
    hand = {k: scores[i].cpu() for i, k in enumerate(KEYS)}
    for m in metrics:
        hand.update(m.result())
    assert set(hand) == set(got)
    for k, v in hand.items():
        assert _same_bits(got[k].double(), v.double()) and got[k].dtype == v.dtype, k
    # c. the two sphere fields are linear in the wind: they have a climatology, their ACC is a number; the speed's is NaN
    acc = got["ens_acc"][C:]
    assert bool(torch.isfinite(acc[:2]).all()) and bool(torch.isnan(acc[2]).all())
    assert all(bool(torch.isfinite(got[k][C:]).all()) for k in KEYS[1:])


@pytest.mark.parametrize("dbf", [3, 6])
def test_products_with_sphere_fields(setup, dbf):
    from ladcast_amd.evaluate import products_of_latent_rollout, rollout_products, sphere_row_tables
    from ladcast_amd.evaluate.rollout_metrics import row_latitudes

    s = setup
    ys = torch.cat([_decode(s, l, 1) for l in range(T)])  # one decoder call per lead time, always ENS frames, as the driver decodes
    tab, k = sphere_row_tables(row_latitudes(H), W)
    ref = SR.derive(ys.cpu().numpy(), FIELDS[:1], 2, tab, k, s["mean"].numpy(), s["std"].numpy())[:, :, 0]  # the reference vorticity, (T, ens, H, W)
    thr = float(np.float32(np.median(ref[..., : H - 1, :]) + 1e-3 * np.std(ref[..., : H - 1, :])))  # about half the members above it
    table = torch.full((1, C + D), float("nan"))
    table[0, C] = thr
    args = (s["latents"], s["g"], s["mean"], s["std"])
    kw = dict(crop_init=True, decode_batch_frames=dbf)
    got = products_of_latent_rollout(*args, thresholds=table, derived=FIELDS, **kw)
    plain = products_of_latent_rollout(*args, **kw)
    for name in ("mean", "std", "min", "max"):
        assert got[name].shape == (C + D, T, H, W) and _same_bits(got[name][:C], plain[name]), name  # the decoded channels keep their bits
    assert got["exceed"].shape == (1, C + D, T, H, W) and bool(torch.isnan(got["exceed"][0, :C]).all())
    mean_e, std_e = torch.cat([s["mean"], torch.zeros(D)]).cuda(), torch.cat([s["std"], torch.ones(D)]).cuda()
    ext, _, _ = _extended(s, ys, TRUTH_SLOTS, s["clim_slots"])
    hand = rollout_products(ext, thresholds=table, lead_dim=0, mean=mean_e, std=std_e)
    for name in ("mean", "std", "min", "max", "exceed"):
        assert _same_bits(got[name].narrow(-4, C, D), hand[name].cpu().narrow(-4, C, D)), name
    # the exceedance plane against the reference field on the non-pole rows, which are bit-equal to it: the member count above thr over M
    want = (ref > np.float32(thr)).sum(axis=1).astype(np.float32) / np.float32(ENS)
    ex = got["exceed"][0, C].numpy()
    assert 0.05 < want.mean() < 0.95 and np.array_equal(ex[:, : H - 1], want[:, : H - 1])
