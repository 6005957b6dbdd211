"""Guard-band and per-element edge tests of the row, layout, sampler and DC-AE element-wise kernels (csrc/rowops.hip, layout.hip,
sampler.hip and the non-GEMM kernels of dcae.hip), all through ladcast_amd.hip.

Every case: guarded outputs (tests/redzone.py), poisoned guarded inputs with strided rows and a batch stride above rows * ld where the
ABI has them, a finite-ness check of the whole payload (a read of a pad column or of the row after the last one pulls a NaN in; an
element that was not written still holds one), the per-element DERIVED bound of tests/row_edge_refs.py against float64 - or
torch.equal where the suite holds the kernel bit-exact -, and `assert_untouched` on every buffer, inputs included.  Inputs are not
iid (rows scaled by 10 ** U(-3, 3), one column in 64 by 100) except one plain-Gaussian case per kernel.  Shapes an entry refuses are
kept, with the error code asserted ("refused").  tests/test_row_edge_bounds_cpu.py judges the bounds themselves."""
import pytest
import torch
import torch.nn.functional as F

from tests import redzone as rz
from tests import row_edge_refs as R
from tests.redzone import FMT_BF16, FMT_F32, FMT_SPLIT, assert_elementwise, assert_untouched, guarded, operand_rows, operand_width

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -3
FMTS = (FMT_F32, FMT_SPLIT, FMT_BF16)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ladcast_amd.hip as h

    return h


def refused(code):
    return pytest.raises(RuntimeError, match=f"failed with status {code}$")


def gin(t, pad=4, gap=8, align=16):
    """poisoned guarded input holding t [B][rows][width] (or [rows][width]) with row stride width + pad, batch stride rows * ld + gap"""
    t = t if t.dim() == 3 else t[None]
    B, rows, w = t.shape
    return guarded(rows, w, w + pad, dtype=t.dtype, align_bytes=align, batch=B, batch_stride=rows * (w + pad) + gap).fill(t)


def gout(B, rows, w, pad=4, gap=8, align=16, dtype=torch.float32):
    return guarded(rows, w, w + pad, dtype=dtype, align_bytes=align, batch=B, batch_stride=rows * (w + pad) + gap)


def gvec(v):
    """contiguous guarded copy of a tensor ([n] or [rows][n]): guards only"""
    return gin(v.reshape(-1, v.shape[-1]) if v.dim() > 1 else v[None], pad=0, gap=0)


def fmt_out(B, rows, C, fmt):
    """guarded output for rows of C values in format fmt (operand rows: 32-byte aligned, strides multiples of 8)"""
    if fmt == FMT_F32:
        return gout(B, rows, C, pad=4)
    w = operand_width(C, fmt)  # the row stride stays that of the fp32 row rounded up to 8, plus 8: above the rounded width
    return gout(B, rows, w, pad=(C + 7) // 8 * 8 + 8 - w, gap=8, align=32)


def finite(g, what):
    p = g.payload()
    assert torch.isfinite(p).all(), f"{what}: {int((~torch.isfinite(p)).sum())} non-finite payload values (a poisoned read or a missing write), first at {tuple((~torch.isfinite(p)).nonzero()[0].tolist())}"
    return p


def untouched(*bufs):
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        if b is not None:
            assert_untouched(b, f"buffer {i}")


def same_bits(got, want, what):
    got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} words differ, first at {tuple(bad[0].tolist())}")


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
def _run_ln(hip, kw, fmt, split_row=None, s2=None, h2=None):
    x = kw["x"]
    B, rows, D = x.shape
    gx, gy = gin(x), fmt_out(B, rows, D, fmt)
    vs = [None if v is None else gin(v[:, None], gap=0) for v in (kw["scale"], kw["shift"], s2, h2)]  # [nb][1][D], batch stride D + 4
    pv = [None if g is None else g.view for g in vs]
    hip.layernorm_mod(gx.view, gy.view, B=B, rows=rows, D=D, ldx=gx.ld, x_bs=gx.bs, ldy=gy.ld, y_bs=gy.bs, scale=pv[0], shift=pv[1], mod_bs=D + 4,
                      mode=kw["mode"], eps=kw["eps"], out_split=fmt, split_row=split_row, scale2=pv[2], shift2=pv[3])
    untouched(gx, gy, *vs)
    return finite(gy, "layernorm") if fmt == FMT_F32 else gy.payload()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layernorm_mod(hip, case, fmt):
    kw = R.ln_inputs(*case)
    D = case[2]
    if fmt != FMT_F32 and D % 8:  # refused: LDC_ERR_ALIGN (operand rows need whole 8-column groups)
        with refused(ERR_ALIGN):
            _run_ln(hip, kw, fmt)
        return
    y32 = _run_ln(hip, kw, FMT_F32)
    want, bound = R.layernorm_ref(**kw)
    print(f"layernorm{case}: worst ratio {assert_elementwise(y32, want, bound, f'layernorm{case}'):.3f}")
    if fmt != FMT_F32:  # operand rows = the split of the fp32 rows, bit for bit
        same_bits(_run_ln(hip, kw, fmt), operand_rows(y32, fmt), f"layernorm{case} fmt {fmt}")


@pytest.mark.parametrize("D,code", [(6, ERR_UNSUPPORTED), (2052, ERR_UNSUPPORTED)])
def test_layernorm_refused_widths(hip, D, code):
    kw = dict(x=R.rows_input(1, 3, D, 1), scale=None, shift=None, mode=1, eps=1e-6)
    with refused(code):
        _run_ln(hip, kw, FMT_F32)


@pytest.mark.parametrize("fmt", (FMT_F32, FMT_SPLIT))
@pytest.mark.parametrize("rows,split_row", [(5, 0), (5, 1), (5, 4), (5, 5), (1, 0), (1, 1)])
def test_layernorm_two_row_segments(hip, rows, split_row, fmt):
    kw = R.ln_inputs(3, rows, 264, 0, True, True, "scaled")
    s2, h2 = R.vec(264, 5, rows=3), R.vec(264, 6, rows=3)
    y32 = _run_ln(hip, kw, FMT_F32, split_row, s2, h2)
    want, bound = R.layernorm_ref(**kw, split_row=split_row, scale2=s2, shift2=h2)
    assert_elementwise(y32, want, bound, f"layernorm split_row {split_row}")
    if fmt != FMT_F32:
        same_bits(_run_ln(hip, kw, fmt, split_row, s2, h2), operand_rows(y32, fmt), "layernorm_mod2 operand rows")


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,rows,D", [(1, 1, 8), (3, 3, 264), (3, 5, 2048), (1, 4, 260)])
def test_gate_residual_layernorm(hip, B, rows, D, fmt):
    d = R.gate_inputs(B, rows, D, True, False)
    w, b = R.vec(D, 3)[0], R.vec(D, 4)[0]
    gr, gyv, gg, gw, gb = gin(d["resid"]), gin(d["y"], pad=8), gin(d["gate"][:, None], gap=0), gvec(w), gvec(b)
    go = fmt_out(B, rows, D, fmt)
    call = lambda: hip.gate_residual_layernorm(gr.view, gyv.view, gg.view, go.view, B=B, rows=rows, D=D, ld_res=gr.ld, res_bs=gr.bs, ld_y=gyv.ld, y_bs=gyv.bs,  # noqa: E731
                                               gate_bs=D + 4, ld_out=go.ld, out_bs=go.bs, weight=gw.t[0], bias=gb.t[0], eps=1e-6, out_split=fmt)
    if fmt != FMT_F32 and D % 8:  # refused: LDC_ERR_ALIGN
        with refused(ERR_ALIGN):
            call()
        return
    call()
    untouched(gr, gyv, gg, gw, gb, go)
    r2 = finite(gr, "resid")
    want, bound = R.gate_residual_ref(**d)
    assert_elementwise(r2, want, bound, "resid += gate * y")
    g2 = gin(d["resid"])  # the same update by ldc_gate_residual: bit-identical
    hip.gate_residual(g2.view, gyv.view, gg.view, g2.view, B=B, rows=rows, D=D, ld_res=g2.ld, res_bs=g2.bs, ld_y=gyv.ld, y_bs=gyv.bs, gate_bs=D + 4)
    same_bits(g2.payload(), r2, "gate_residual_layernorm's residual vs ldc_gate_residual")
    kw = dict(x=r2, scale=w[None], shift=b[None], mode=1, eps=1e-6)
    y32 = _run_ln(hip, kw, FMT_F32)  # bit-identical to ldc_layernorm_mod(mode 1) on the updated residual
    want, bound = R.layernorm_ref(**kw)
    assert_elementwise(y32, want, bound, "LayerNorm of the updated residual")
    same_bits(go.payload(), operand_rows(y32, fmt), "gate_residual_layernorm out")


# ---- q / k RMSNorm + RoPE ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.QK_CASES, ids=str)
def test_qk_rmsnorm_rope(hip, case):
    rows, H, row0, rope, _ = case
    d = R.qk_inputs(*case)
    qkv = d["qkv"]
    B, tot, w = qkv.shape
    g = gin(qkv, pad=2, gap=6)  # ld > 3 * H * 128; the entry asks for even strides only
    gq, gk, gc, gs = gvec(d["wq"]), gvec(d["wk"]), None, None
    if rope:
        gc, gs = gvec(d["cos"]), gvec(d["sin"])
    D = H * 128
    hip.qk_rmsnorm_rope(g.view, g.view[:, :, D:], B=B, row0=row0, rows=rows, H=H, ld=g.ld, bs=g.bs, wq=gq.t[0], wk=gk.t[0], eps=d["eps"],
                        cos=gc.t if rope else None, sin=gs.t if rope else None)
    untouched(g, gq, gk, gc, gs)
    got = finite(g, "qkv")
    keep = torch.ones(tot, dtype=torch.bool)
    keep[row0:row0 + rows] = False
    same_bits(got[:, keep], qkv[:, keep], "rows outside [row0, row0 + rows)")
    same_bits(got[:, :, 2 * D:], qkv[:, :, 2 * D:], "v")
    for i, wv in enumerate((d["wq"], d["wk"])):
        x = qkv[:, row0:row0 + rows, i * D:(i + 1) * D].reshape(B, rows, H, 128)
        want, bound = R.qk_rmsnorm_rope_ref(x, wv, d["eps"], d["cos"], d["sin"])
        assert_elementwise(got[:, row0:row0 + rows, i * D:(i + 1) * D].reshape(B, rows, H, 128), want, bound, f"{'qk'[i]}{case}")


# ---- mean over rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.MEAN_CASES, ids=str)
def test_mean_rows(hip, case):
    B, rows, D, _ = case
    x = R.mean_inputs(*case)
    gx, gy = gin(x), gout(1, B, D, pad=0, gap=0)
    hip.mean_rows(gx.view, gy.view, B=B, rows=rows, D=D, ldx=gx.ld, x_bs=gx.bs)
    untouched(gx, gy)
    y = finite(gy, "mean")[0]
    want, bound = R.mean_rows_ref(x)
    print(f"mean_rows{case}: worst ratio {assert_elementwise(y, want, bound, f'mean_rows{case}'):.3f}")
    for fmt in (FMT_SPLIT, FMT_BF16):
        gy2, gs = gout(1, B, D, pad=0, gap=0), fmt_out(B, rows, D, fmt)
        call = lambda: hip.mean_rows(gx.view, gy2.view, B=B, rows=rows, D=D, ldx=gx.ld, x_bs=gx.bs, x_split=gs.view, lds=gs.ld, s_bs=gs.bs, fmt=fmt)  # noqa: E731
        if D % 8:  # refused: LDC_ERR_ALIGN (D = 4 is served by the plain form only)
            with refused(ERR_ALIGN):
                call()
            continue
        call()
        untouched(gx, gy2, gs)
        same_bits(gy2.payload()[0], y, "mean of the split form vs the plain form")
        same_bits(gs.payload(), operand_rows(x, fmt), f"x_split fmt {fmt}")


# ---- gated residual -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GATE_CASES, ids=str)
def test_gate_residual(hip, case):
    B, rows, D, inplace, _ = case
    d = R.gate_inputs(*case)
    gr, gyv, gg = gin(d["resid"]), gin(d["y"], pad=8, gap=16), gin(d["gate"][:, None], gap=0)
    go = gr if inplace else guarded(rows, D, gr.ld, batch=B, batch_stride=gr.bs)  # out shares the residual's strides
    hip.gate_residual(gr.view, gyv.view, gg.view, go.view, B=B, rows=rows, D=D, ld_res=gr.ld, res_bs=gr.bs, ld_y=gyv.ld, y_bs=gyv.bs, gate_bs=D + 4)
    untouched(gr, gyv, gg, go)
    if not inplace:
        same_bits(gr.payload(), d["resid"], "resid of the out-of-place form")
    want, bound = R.gate_residual_ref(**d)
    assert_elementwise(finite(go, "out"), want, bound, f"gate_residual{case}")


def test_gate_residual_more_rows_than_a_grid_dimension(hip):
    """rows = 65537, D = 4: rows ride on gridDim.y (<= 65535) - the entry refuses (LDC_ERR_UNSUPPORTED) rather than return garbage"""
    rows = 65537
    gr, gyv, gg, go = gin(torch.ones(1, rows, 4), pad=0), gin(torch.ones(1, rows, 4), pad=0), gvec(torch.ones(4)), gout(1, rows, 4, pad=0)
    try:
        hip.gate_residual(gr.view, gyv.view, gg.view, go.view, B=1, rows=rows, D=4, ld_res=4, res_bs=gr.bs, ld_y=4, y_bs=gyv.bs, gate_bs=4)
    except RuntimeError as e:
        assert str(e).endswith(f"status {ERR_UNSUPPORTED}"), e
        untouched(gr, gyv, gg, go)
        assert not torch.isfinite(go.payload()).any()  # nothing was launched
        return
    untouched(gr, gyv, gg, go)
    assert torch.equal(finite(go, "out"), torch.full((1, rows, 4), 2.0))


# ---- small-M linear ---------------------------------------------------------------------------------------------------------------------------
def _ls_bufs(kw):
    x = kw["x"]
    gx = gvec(x if x.dim() == 2 else x)
    return gx, gvec(kw["W"]), *[None if kw[k] is None else gvec(kw[k]) for k in ("bias", "add", "mod")]


def _ls_args(case, kw, bufs):
    rows, x_rows, add_rows, N, K, act_in, act_out, _, mod_rows = case
    gx, gW, gb, ga, gm = bufs
    return dict(rows=rows, N=N, K=K, x_rows=x_rows, bias=None if gb is None else gb.t[0], add=None if ga is None else ga.t, add_rows=max(add_rows, 1),
                act_in=act_in, act_out=act_out)


@pytest.mark.parametrize("case", R.LS_CASES, ids=str)
def test_linear_small(hip, case):
    rows, x_rows, add_rows, N, K, act_in, act_out, _, mod_rows = case
    kw = R.ls_inputs(*case)
    bufs = _ls_bufs(kw)
    gx, gW, gb, ga, gm = bufs
    gy = gout(1, rows, N, pad=0)
    a = _ls_args(case, kw, bufs)
    xin = gx.t[0] if act_in == R.ACT_IN_TIMESTEP_SINCOS else gx.t
    hip.linear_small(xin, gW.t, gy.t, **a, mod=None if gm is None else gm.t, mod_rows=max(mod_rows, 1))
    untouched(*bufs, gy)
    y = finite(gy, "y")[0]
    want, bound = R.linear_small_ref(**kw)
    print(f"linear_small{case}: worst ratio {assert_elementwise(y, want, bound, f'linear_small{case}'):.3f}")
    if gm is None:  # the grouped launch: bit-identical to the single one (VALU kernel)
        g2, g3 = gout(1, rows, N, pad=0), gout(1, rows, N, pad=0)
        hip.linear_small_grouped([hip.linear_small_problem(xin, gW.t, g2.t, **a), hip.linear_small_problem(xin, gW.t, g3.t, **a)])
        untouched(*bufs, g2, g3)
        same_bits(g2.payload()[0], y, "grouped problem 0 vs single launch")
        same_bits(g3.payload()[0], y, "grouped problem 1 vs single launch")
    else:  # the modulation epilogue = ldc_linear_small + ldc_temb_modulate, bit for bit
        g2 = gout(1, rows, N, pad=0)
        hip.linear_small(xin, gW.t, g2.t, **a)
        hip.temb_modulate(g2.t, gm.t, B=rows, D=N, te_rows=mod_rows)
        same_bits(g2.payload()[0], y, "linear_small_mod vs linear_small + temb_modulate")
    if act_in == R.ACT_IN_TIMESTEP_SINCOS:  # the sinusoid input is ldc_timestep_embedding's, bit for bit
        ge, g2 = gout(1, x_rows, 256, pad=0), gout(1, rows, N, pad=0)
        hip.timestep_embedding(gx.t[0], ge.t, x_rows)
        hip.linear_small(ge.t, gW.t, g2.t, **dict(a, act_in=0))
        untouched(ge, g2)
        same_bits(g2.payload()[0], y, "timestep sinusoid inside the linear vs ldc_timestep_embedding + linear")


@pytest.mark.parametrize("K,act_in,code", [(6, 0, ERR_ALIGN), (260, R.ACT_IN_TIMESTEP_SINCOS, ERR_ARG)])
def test_linear_small_refused(hip, K, act_in, code):
    x, W, y = gvec(torch.ones(1, K)), gvec(torch.ones(3, K)), gout(1, 1, 3, pad=0)
    with refused(code):
        hip.linear_small(x.t, W.t, y.t, rows=1, N=3, K=K, act_in=act_in)
    untouched(x, W, y)


# ---- timestep embedding, temb modulation, channel affine --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5])
def test_timestep_embedding(hip, n):
    from oracle.layers import get_timestep_embedding

    t = torch.tensor(R.TIMESTEPS).flip(0)[:n].clone() if n < 5 else torch.tensor(R.TIMESTEPS)
    gt, ge = gvec(t), gout(1, n, 256, pad=0)
    hip.timestep_embedding(gt.t[0], ge.t, n)
    untouched(gt, ge)
    want, bound = R.timestep_embedding_ref(t)
    print(f"timestep_embedding n={n}: worst ratio {assert_elementwise(finite(ge, 'emb')[0], want, bound, 'timestep_embedding'):.3f}")
    assert_elementwise(get_timestep_embedding(t, 256), want, bound, "oracle.layers.get_timestep_embedding")


@pytest.mark.parametrize("case", R.TEMB_CASES, ids=str)
def test_temb_modulate(hip, case):
    B, te_rows, D = case
    d = R.temb_inputs(*case)
    gt, ge = gvec(d["temb"]), gvec(d["te"])
    hip.temb_modulate(gt.t, ge.t, B=B, D=D, te_rows=te_rows)
    untouched(gt, ge)
    want, bound = R.temb_modulate_ref(**d)
    assert_elementwise(finite(gt, "temb")[0], want, bound, f"temb_modulate{case}")


@pytest.mark.parametrize("outer", [1, 3])
@pytest.mark.parametrize("C", [1, 84])
@pytest.mark.parametrize("inner", [1, 7, 450])
def test_chan_affine(hip, outer, C, inner):
    x = R.rows_input(outer, C, inner, 7 + C + inner)
    mu, sd = R.vec(C, 1)[0], R.vec(C, 2)[0].abs() + 0.3
    gx, gm, gs = gvec(x.reshape(1, -1)), gvec(mu), gvec(sd)
    gy, gz = gout(1, 1, x.numel(), pad=0), gout(1, 1, x.numel(), pad=0)
    hip.chan_affine(gx.t, gy.t, gm.t[0], gs.t[0], 0.5, outer=outer, C=C, inner=inner, inverse=False)
    hip.chan_affine(gy.t, gz.t, gm.t[0], gs.t[0], 0.5, outer=outer, C=C, inner=inner, inverse=True)
    untouched(gx, gm, gs, gy, gz)
    want = (x - mu[None, :, None]) / sd[None, :, None] * 0.5
    same_bits(gy.payload().reshape(x.shape), want, "chan_affine forward vs torch fp32")
    same_bits(gz.payload().reshape(x.shape), (want / 0.5) * sd[None, :, None] + mu[None, :, None], "chan_affine inverse vs torch fp32")


# ---- layout transposes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,C,N", [(1, 1, 1), (2, 31, 33), (1, 32, 32), (2, 33, 31), (1, 84, 65), (2, 1, 65), (1, 33, 1)])
def test_chan_to_token_and_back(hip, B, C, N, fmt):
    x = R.rows_input(B, C, N, 3 + C + N)
    fill = (C + 7) // 8 * 8 + 8  # C < fill_cols < ldo
    ldo = fill + 8
    wf = operand_width(fill, fmt)
    gx = gvec(x.reshape(1, -1))
    go = guarded(B * N, wf, ldo, align_bytes=32)  # batches are contiguous token rows: [B * N][ldo]
    hip.chan_to_token(gx.t, go.t, B=B, C=C, N=N, ldo=ldo, fill_cols=fill, out_split=fmt)
    untouched(gx, go)  # [fill_cols, ldo) is pad: untouched
    tok = F.pad(x.transpose(1, 2), (0, fill - C)).reshape(B * N, fill)  # columns [C, fill_cols) are zero
    same_bits(go.payload()[0], operand_rows(tok, fmt), f"chan_to_token fmt {fmt}")
    if fmt == FMT_F32:
        gb = gout(1, 1, x.numel(), pad=0)
        hip.token_to_chan(go.t, gb.t, B=B, C=C, N=N, ldi=ldo)
        untouched(go, gb)
        same_bits(gb.payload().reshape(x.shape), x, "token_to_chan")


# ---- sampler state updates: bit-equal to torch's elementwise arithmetic, guards on all operands ---------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_sampler_updates(hip, n):
    f32 = lambda s: R.vec(n, s + n)[0]  # noqa: E731
    g = lambda t: gvec(t)  # noqa: E731
    o32, o64 = (lambda: gout(1, 1, n, pad=0)), (lambda: gout(1, 1, n, pad=0, dtype=torch.float64))
    noise, Fm, smp, m1 = f32(1), f32(2), f32(3), f32(4)
    s0, s1, sd = torch.tensor(79.999985), torch.tensor(59.657501), 0.5
    gn, gF = g(noise), g(Fm)
    x = o64()
    hip.edm_init_state(gn.t[0], float(s0), x.t[0])
    x_ref = noise.double() * s0
    assert torch.equal(x.payload()[0, 0], x_ref)
    c_in = 1 / ((s0**2 + sd**2) ** 0.5)
    xin, x32 = o32(), o32()
    hip.edm_scale_f64_to_f32(x.t[0], float(c_in), xin.t[0])
    hip.f64_to_f32(x.t[0], x32.t[0])
    assert torch.equal(xin.payload()[0, 0], (x_ref * c_in).float()) and torch.equal(x32.payload()[0, 0], x_ref.float())
    nz64 = g(R.vec(n, 9 + n)[0].double())
    xh = o64()
    hip.edm_churn(x.t[0], nz64.t[0], 0.37, xh.t[0])
    assert torch.equal(xh.payload()[0, 0], x_ref + 0.37 * nz64.payload()[0, 0])
    c_skip, c_out = sd**2 / (s0**2 + sd**2), s0 * sd / (s0**2 + sd**2) ** 0.5
    xn, dc = o64(), o64()
    hip.edm_euler(x.t[0], gF.t[0], float(c_skip), float(c_out), float(s0), float(s1 - s0), xn.t[0], dc.t[0])
    d_ref = (x_ref - (c_skip * x_ref + c_out * Fm.double())) / s0
    xn_ref = x_ref + (s1 - s0) * d_ref
    assert torch.equal(dc.payload()[0, 0], d_ref) and torch.equal(xn.payload()[0, 0], xn_ref)
    c_skip1, c_out1 = sd**2 / (s1**2 + sd**2), s1 * sd / (s1**2 + sd**2) ** 0.5
    hip.edm_heun(x.t[0], xn.t[0], gF.t[0], dc.t[0], float(c_skip1), float(c_out1), float(s1), float(s1 - s0))  # x_next in place, as the sampler runs it
    dp = (xn_ref - (c_skip1 * xn_ref + c_out1 * Fm.double())) / s1
    assert torch.equal(xn.payload()[0, 0], x_ref + (s1 - s0) * (0.5 * d_ref + 0.5 * dp))
    untouched(gn, gF, x, xin, x32, nz64, xh, xn, dc)
    # DPM-Solver++ orders 1 and 2 (fp32)
    gs, gm1 = g(smp), g(m1)
    a, b, inv_r0 = torch.tensor(0.7457), torch.tensor(-0.2543), torch.tensor(1.25)
    m0 = c_skip * smp + c_out * Fm
    for order, want in ((1, a * smp - b * m0), (2, a * smp - b * m0 - (0.5 * b) * (inv_r0 * (m0 - m1)))):
        x0, prev = o32(), o32()
        hip.dpm_step(gs.t[0], gF.t[0], gm1.t[0] if order == 2 else None, x0.t[0], prev.t[0], float(c_skip), float(c_out), float(a), float(b), float(inv_r0), order)
        untouched(gs, gF, gm1, x0, prev)
        assert torch.equal(x0.payload()[0, 0], m0) and torch.equal(prev.payload()[0, 0], want), f"dpm_step order {order}"
    sp = g(smp)  # `prev` written over the sample, as the pipeline's loop does
    x0 = o32()
    hip.dpm_step(sp.t[0], gF.t[0], gm1.t[0], x0.t[0], sp.t[0], float(c_skip), float(c_out), float(a), float(b), float(inv_r0), 2)
    untouched(sp, x0)
    assert torch.equal(sp.payload()[0, 0], a * smp - b * m0 - (0.5 * b) * (inv_r0 * (m0 - m1)))
    # DDIM / DDPM (fp32), every prediction type, clamp on, noise on / off
    sa, sb, c0, c1, sdv, clip = (torch.tensor(v) for v in (0.83, 0.5577, 0.9, 0.31, 0.2, 1.5))
    for pred in (0, 1, 2):
        x0r = ((smp - sb * Fm) / sa, Fm, sa * smp - sb * Fm)[pred].clamp(-clip, clip)
        eps = (smp - sa * x0r) / sb  # use_clipped_model_output
        for ddpm, has_noise in ((0, True), (0, False), (1, True), (1, False)):
            want = c0 * x0r + c1 * (smp if ddpm else eps)
            if has_noise:
                want = want + sdv * noise
            x0, prev = o32(), o32()
            nz = gn.t[0] if has_noise else None
            if ddpm:
                hip.ddpm_step(gs.t[0], gF.t[0], nz, x0.t[0], prev.t[0], float(sa), float(sb), float(c0), float(c1), float(sdv), float(clip), pred)
            else:
                hip.ddim_step(gs.t[0], gF.t[0], nz, x0.t[0], prev.t[0], float(sa), float(sb), float(c0), float(c1), float(sdv), float(clip), pred, True)
            untouched(gs, gF, gn, x0, prev)
            assert torch.equal(x0.payload()[0, 0], x0r) and torch.equal(prev.payload()[0, 0], want), f"{'ddpm' if ddpm else 'ddim'} pred {pred} noise {has_noise}"
    y, z = o32(), o32()
    hip.scale_f32(gs.t[0], 0.37, y.t[0])
    hip.axpby_f32(gs.t[0], 0.3, gF.t[0], -1.7, z.t[0])
    untouched(gs, gF, y, z)
    assert torch.equal(y.payload()[0, 0], smp * torch.tensor(0.37)) and torch.equal(z.payload()[0, 0], torch.tensor(0.3) * smp + torch.tensor(-1.7) * Fm)
    hip.axpby_f32(gs.t[0], 0.3, gF.t[0], -1.7, gs.t[0])  # in place: scheduler.add_noise on the state
    untouched(gs)
    assert torch.equal(gs.payload()[0, 0], z.payload()[0, 0])


# ---- RMSNorm rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", R.RMS_CASES, ids=str)
def test_rmsnorm_rows(hip, case, fmt):
    rows, C, act, has_b, has_r, _ = case
    kw = R.rms_inputs(*case)
    gx, gw = gin(kw["x"]), gvec(kw["w"])
    gb = None if kw["b"] is None else gvec(kw["b"])
    gr = None if kw["resid"] is None else gin(kw["resid"], pad=8)
    gy = gout(1, rows, C, pad=12)
    a = dict(rows=rows, C=C, eps=kw["eps"], b=None if gb is None else gb.t[0], resid=None if gr is None else gr.t, ldx=gx.ld, ldr=None if gr is None else gr.ld, act=act)
    hip.rmsnorm_rows(gx.t, gw.t[0], gy.t, ldy=gy.ld, **a)
    untouched(gx, gw, gb, gr, gy)
    y = finite(gy, "y")[0]
    want, bound = R.rmsnorm_rows_ref(**kw)
    print(f"rmsnorm_rows{case}: worst ratio {assert_elementwise(y, want, bound, f'rmsnorm_rows{case}'):.3f}")
    if fmt != FMT_F32:  # operand rows (y = None), pad half-groups zero, lds above the rounded width
        gs = fmt_out(1, rows, C, fmt)
        hip.rmsnorm_rows(gx.t, gw.t[0], None, ys=gs.t, lds=gs.ld, fmt=fmt, **a)
        untouched(gx, gs)
        same_bits(gs.payload()[0], operand_rows(y, fmt), f"rmsnorm_rows{case} ys fmt {fmt}")
        gy2, gs2 = gout(1, rows, C, pad=4), fmt_out(1, rows, C, fmt)  # both outputs in one launch
        hip.rmsnorm_rows(gx.t, gw.t[0], gy2.t, ldy=gy2.ld, ys=gs2.t, lds=gs2.ld, fmt=fmt, **a)
        untouched(gy2, gs2)
        same_bits(gy2.payload()[0], y, "y next to ys")
        same_bits(gs2.payload()[0], gs.payload()[0], "ys next to y")


def test_rmsnorm_rows_refused_width(hip):
    x, w, y = gvec(torch.ones(1, 2052)), gvec(torch.ones(2052)), gout(1, 1, 2052, pad=0)
    with refused(ERR_UNSUPPORTED):  # C > 2048
        hip.rmsnorm_rows(x.t, w.t[0], y.t, rows=1, C=2052, eps=1e-5)
    untouched(x, w, y)


# ---- DC-AE shuffles, regroup, split copies ------------------------------------------------------------------------------------------------------------
def _both(hip_call, y_shape, C, fmt, what, want_bits=None):
    """run a producer with (y, ys) guarded; returns y's payload; ys must be the operand rows of y"""
    rows = 1
    for v in y_shape[:-1]:
        rows *= v
    gy, gs = gout(1, rows, C, pad=0), (fmt_out(1, rows, C, fmt) if fmt != FMT_F32 else None)
    hip_call(gy.t, None if gs is None else gs.t, None if gs is None else gs.ld)
    untouched(gy, gs)
    y = finite(gy, what)[0]
    if gs is not None:
        same_bits(gs.payload()[0], operand_rows(y, fmt), f"{what}: operand rows fmt {fmt}")
    return y.reshape(y_shape)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("case", R.UNSHUF_CASES, ids=str)
def test_pixel_unshuffle_shortcut(hip, case, fmt):
    B, H2, W2, cout, cin = case
    kw = R.unshuf_inputs(*case)
    gc, gx = gvec(kw["cv"].reshape(1, -1)), None if cin is None else gvec(kw["x"].reshape(1, -1))
    y = _both(lambda y, ys, lds: hip.pixel_unshuffle_shortcut(gc.t, None if gx is None else gx.t, y, B=B, H2=H2, W2=W2, cout=cout, cin=cin or 1, ys=ys, lds=lds, fmt=fmt),
              (B, H2, W2, cout), cout, fmt, f"pixel_unshuffle_shortcut{case}")
    untouched(gc, gx)
    want, bound = R.pixel_unshuffle_shortcut_ref(**kw)
    assert_elementwise(y, want, bound, f"pixel_unshuffle_shortcut{case}")  # (x = None: bound 0, the copy is exact)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,cout,cin,has_cv", [(1, 1, 1, 4, 16, True), (1, 1, 2, 12, 12, True), (2, 3, 5, 12, 16, True), (2, 3, 5, 20, 40, True), (1, 1, 2, 12, 24, False),
                                                    (2, 3, 5, 4, 4, False)])
def test_pixel_shuffle_shortcut(hip, B, H, W, cout, cin, has_cv, fmt):
    cv, x = R.rows_input(B, H * W, 4 * cout, 5 + cout).reshape(B, H, W, 4 * cout), R.rows_input(B, H * W, cin, 6 + cin).reshape(B, H, W, cin)
    gc, gx = gvec(cv.reshape(1, -1)) if has_cv else None, gvec(x.reshape(1, -1))
    y = _both(lambda y, ys, lds: hip.pixel_shuffle_shortcut(None if gc is None else gc.t, gx.t, y, B=B, H=H, W=W, cout=cout, cin=cin, ys=ys, lds=lds, fmt=fmt),
              (B, 2 * H, 2 * W, cout), cout, fmt, "pixel_shuffle_shortcut")
    untouched(gc, gx)
    sc = F.pixel_shuffle(x.repeat_interleave(4 * cout // cin, dim=-1).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    want = sc if not has_cv else F.pixel_shuffle(cv.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) + sc  # one fp32 add: bit-equal to torch's
    same_bits(y, want.contiguous(), "pixel_shuffle_shortcut vs torch fp32")


def test_pixel_shuffle_shortcut_refused(hip):
    x, y = gvec(torch.ones(1, 6)), gout(1, 4, 6, pad=0)
    with refused(ERR_UNSUPPORTED):  # cout % 4 != 0
        hip.pixel_shuffle_shortcut(None, x.t, y.t, B=1, H=1, W=1, cout=6, cin=6)
    untouched(x, y)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (1, 1, 2, 12), (2, 3, 5, 12), (2, 3, 5, 8)])
def test_upsample_nearest2x_rows(hip, B, H, W, C, fmt):
    x = R.rows_input(1, B * H * W, C, 8 + C)
    gx = gin(x)
    rows = B * 4 * H * W
    gy, gs = gout(1, rows, C, pad=8), (fmt_out(1, rows, C, fmt) if fmt != FMT_F32 else None)
    hip.upsample_nearest2x_rows(gx.t, gy.t, B=B, H=H, W=W, C=C, ldx=gx.ld, ldy=gy.ld, ys=None if gs is None else gs.t, lds=None if gs is None else gs.ld, fmt=fmt)
    untouched(gx, gy, gs)
    want = x.reshape(B, H, W, C).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(rows, C)
    same_bits(finite(gy, "y")[0], want, "upsample_nearest2x_rows")
    if gs is not None:
        same_bits(gs.payload()[0], operand_rows(want, fmt), f"upsample_nearest2x_rows ys fmt {fmt}")
        g2 = fmt_out(1, rows, C, fmt)  # y = None
        hip.upsample_nearest2x_rows(gx.t, None, B=B, H=H, W=W, C=C, ldx=gx.ld, ys=g2.t, lds=g2.ld, fmt=fmt)
        untouched(g2)
        same_bits(g2.payload()[0], gs.payload()[0], "ys alone")


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 1, 2), (2, 3, 5)])
@pytest.mark.parametrize("cout,keep", [(1, 1), (3, 2), (5, 4), (5, 5)])
def test_pixel_shuffle_to_chan(hip, B, H, W, cout, keep):
    cv = R.rows_input(B, H * W, 4 * cout, 9 + cout).reshape(B, H, W, 4 * cout)
    gc, go = gvec(cv.reshape(1, -1)), gout(1, 1, B * keep * 4 * H * W, pad=0)
    hip.pixel_shuffle_to_chan(gc.t, go.t, B=B, H=H, W=W, cout=cout, keep=keep)
    untouched(gc, go)
    same_bits(finite(go, "out").reshape(B, keep, 2 * H, 2 * W), F.pixel_shuffle(cv.permute(0, 3, 1, 2), 2)[:, :keep].contiguous(), "pixel_shuffle_to_chan")


@pytest.mark.parametrize("M,cin,cout", R.REGROUP_DOWN + [(1, 4, 8), (15, 4, 12), (3, 3, 12), (2, 1, 4)])
def test_chan_regroup(hip, M, cin, cout):
    x = R.rows_input(1, M, cin, 41 + M)[0]
    gx, gy = gvec(x.reshape(1, -1)), gout(1, 1, M * cout, pad=0)
    hip.chan_regroup(gx.t, gy.t, M=M, cin=cin, cout=cout)
    untouched(gx, gy)
    y = finite(gy, "y").reshape(M, cout)
    if cin < cout:
        same_bits(y, x.repeat_interleave(cout // cin, dim=1).contiguous(), "chan_regroup up")
    else:
        want, bound = R.chan_regroup_down_ref(x, cout)
        assert_elementwise(y, want, bound, "chan_regroup down")


def test_chan_regroup_refused(hip):
    x, y = gvec(torch.ones(1, 5)), gout(1, 1, 3, pad=0)
    with refused(ERR_UNSUPPORTED):  # 5 channels into 3
        hip.chan_regroup(x.t, y.t, M=1, cin=5, cout=3)
    untouched(x, y)


@pytest.mark.parametrize("fmt", (FMT_SPLIT, FMT_BF16))
@pytest.mark.parametrize("rows,C", [(1, 4), (3, 12), (65, 20), (5, 8), (257, 4)])
def test_split_rows(hip, rows, C, fmt):
    x = R.rows_input(1, rows, C, rows + C)
    gx, gs = gin(x), fmt_out(1, rows, C, fmt)
    hip.split_rows(gx.t, gs.t, rows=rows, C=C, ldx=gx.ld, lds=gs.ld, fmt=fmt)
    untouched(gx, gs)
    same_bits(gs.payload()[0], operand_rows(x[0], fmt), "split_rows")


# ---- grouped 1 x 1 conv ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GCONV_CASES, ids=str)
def test_grouped_conv1x1(hip, case):
    M, groups = case
    kw = R.gconv_inputs(*case)
    gx, gw, gy = gin(kw["x"]), gvec(kw["wt"]), gout(1, M, groups * 32, pad=8)
    hip.grouped_conv1x1_nhwc(gx.t, gw.t, gy.t, M=M, groups=groups, ldx=gx.ld, ldy=gy.ld)
    untouched(gx, gw, gy)
    want, bound = R.grouped_conv1x1_ref(**kw)
    assert_elementwise(finite(gy, "y")[0], want, bound, f"grouped_conv1x1{case}")


# ---- ReLU linear attention ---------------------------------------------------------------------------------------------------------------------------------
# below 1024 pixels `sliced` changes nothing (the one-launch kernel runs either way): those shapes take sliced=False once, in fp32
@pytest.mark.parametrize("case,fmt,sliced", [(c, f, s) for c in R.RLA_CASES for f in FMTS for s in (True, False) if s or c[1] >= 1024 or f == FMT_F32], ids=str)
def test_relu_linear_attn(hip, case, fmt, sliced):
    B, P, groups, kind = case
    qkv = R.rla_inputs(*case)
    gq = guarded(B * P, groups * 96, groups * 96 + 8)  # ldq wider than the groups, poison beside them; batches are contiguous pixel rows
    gq.fill(qkv.reshape(1, B * P, -1))
    gy = guarded(B * P, operand_width(groups * 32, fmt), groups * 32 + 8, align_bytes=32)
    hip.relu_linear_attn_nhwc(gq.t, gy.t, B=B, P=P, groups=groups, ldq=gq.ld, ldy=gy.ld, eps=1e-15, out_fmt=fmt, sliced=sliced)
    untouched(gq, gy)
    want, bound = R.relu_linear_attn_ref(qkv, groups, 1e-15)
    if fmt == FMT_F32:
        y = finite(gy, "y")[0].reshape(B, P, groups * 32)
        print(f"relu_linear_attn{case} sliced={sliced}: worst ratio {assert_elementwise(y, want, bound, f'relu_linear_attn{case}'):.3f}")
        if kind == "zero_q":
            assert (y[0, P // 2, :32] == 0).all()
        if kind == "zero_k":
            assert (y[..., :32] == 0).all()
    else:  # operand rows = the split of the fp32 rows of the same schedule
        g32 = guarded(B * P, groups * 32, groups * 32 + 8)
        hip.relu_linear_attn_nhwc(gq.t, g32.t, B=B, P=P, groups=groups, ldq=gq.ld, ldy=g32.ld, eps=1e-15, out_fmt=FMT_F32, sliced=sliced)
        same_bits(gy.payload()[0], operand_rows(g32.payload()[0], fmt), f"relu_linear_attn fmt {fmt}")


# ---- depthwise sphere conv -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.DW_CASES, ids=str)
def test_sphere_dwconv(hip, case):
    B, H, W, C, ks, glu, has_bias = case
    kw = R.dw_inputs(*case)
    cy = C // 2 if glu else C
    gx, gw = gin(kw["x"].reshape(1, B * H * W, C)), gvec(kw["wt"])
    gb = gvec(kw["bias"]) if has_bias else None
    gy = gout(1, B * H * W, cy, pad=4)
    a = dict(B=B, H=H, W=W, C=C, ldx=gx.ld, bias=None if gb is None else gb.t[0], ksize=ks, glu=glu)
    hip.sphere_dwconv_nhwc(gx.t, gw.t, gy.t, ldy=gy.ld, **a)
    untouched(gx, gw, gb, gy)
    y = finite(gy, "y")[0]
    want, bound = R.sphere_dwconv_ref(**kw)
    print(f"sphere_dwconv{case}: worst ratio {assert_elementwise(y.reshape(want.shape), want, bound, f'sphere_dwconv{case}'):.3f}")
    for fmt in (FMT_SPLIT, FMT_BF16):
        gs = fmt_out(1, B * H * W, cy, fmt)
        call = lambda: hip.sphere_dwconv_nhwc(gx.t, gw.t, gs.t, ldy=gs.ld, out_fmt=fmt, **a)  # noqa: E731
        if cy % 8:  # refused: LDC_ERR_ALIGN (operand rows need whole groups here)
            with refused(ERR_ALIGN):
                call()
            continue
        call()
        untouched(gx, gs)
        same_bits(gs.payload()[0], operand_rows(y, fmt), f"sphere_dwconv{case} fmt {fmt}")


@pytest.mark.parametrize("H,W,C,ks,glu,code", [(3, 5, 4, 3, False, ERR_UNSUPPORTED), (1, 4, 4, 3, False, ERR_UNSUPPORTED), (3, 4, 4, 7, False, ERR_UNSUPPORTED),
                                               (3, 4, 6, 3, False, ERR_ALIGN), (3, 4, 12, 3, True, ERR_ALIGN)])
def test_sphere_dwconv_refused(hip, H, W, C, ks, glu, code):
    x, w, y = gvec(torch.ones(H * W, C)), gvec(torch.ones(ks * ks, C)), gout(1, H * W, C, pad=0)
    with refused(code):
        hip.sphere_dwconv_nhwc(x.t, w.t, y.t, B=1, H=H, W=W, C=C, ksize=ks, glu=glu)
    untouched(x, w, y)
