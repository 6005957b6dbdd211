"""The bounds of tests/test_gpu_row_edges.py, judged on the CPU before any kernel is blamed.

For every bound of the GPU file, on the same seeded inputs (tests/row_edge_refs.py):
  * the same formula evaluated in plain fp32 torch lies within the bound (worst ratio printed, < 1): a correct fp32 implementation
    can meet it;
  * three planted defects, applied to that fp32 result, exceed it at least 4 x (ratios printed): one dropped term of the reduction,
    one element taken from the neighbouring row, one rounding of the result to bf16.
And tests/redzone.py is tested on itself: a one-word write into each kind of region is reported by that region's name.
Run with -s to see the ratios."""
import pytest
import torch

from tests import redzone as rz
from tests import row_edge_refs as R


def _judge(name, want, bound, got, got_drop=None):
    """fp32 restatement inside the bound; each applicable planted defect >= 4 x outside it"""
    ok = rz.assert_elementwise(got, want, bound, f"{name}: fp32 restatement")
    out = [f"fp32 {ok:.3f}"]
    ratios = {}
    if got_drop is not None:
        ratios["dropped term"] = rz.worst_ratio(got_drop, want, bound)[0]
    g2 = got.reshape(-1, got.shape[-1])
    if g2.shape[0] >= 2 and not torch.equal(g2[0], g2[1]):
        g = g2.clone()
        c = int((g2[0] - g2[1]).abs().argmax())  # (a column where the two rows differ at all)
        g[0, c] = g2[1, c]
        ratios["neighbour row"] = rz.worst_ratio(g.reshape(got.shape), want, bound)[0]
    ratios["bf16 rounding"] = rz.worst_ratio(got.bfloat16().float(), want, bound)[0]
    for k, v in ratios.items():
        out.append(f"{k} {v:.3g}")
    print(f"{name}: " + ", ".join(out))
    for k, v in ratios.items():
        assert v >= 4.0, f"{name}: the bound does not see the planted defect '{k}' (ratio {v:.3g} < 4)"


@pytest.mark.parametrize("case", R.LN_CASES, ids=str)
def test_layernorm_bound(case):
    kw = R.ln_inputs(*case)
    want, bound = R.layernorm_ref(**kw)
    _judge(f"layernorm{case}", want, bound, R.layernorm_f32(**kw), R.layernorm_f32(**kw, drop=True))


def test_layernorm_two_segments_bound():
    kw = R.ln_inputs(3, 5, 260, 0, True, True, "scaled")
    kw2 = dict(kw, split_row=2, scale2=R.vec(260, 5, rows=3), shift2=R.vec(260, 6, rows=3))
    want, bound = R.layernorm_ref(**kw2)
    _judge("layernorm split_row=2", want, bound, R.layernorm_f32(**kw2), R.layernorm_f32(**kw2, drop=True))


@pytest.mark.parametrize("case", R.QK_CASES, ids=str)
def test_qk_rmsnorm_rope_bound(case):
    rows, H, row0 = case[:3]
    d = R.qk_inputs(*case)
    x = d["qkv"][:, row0:row0 + rows, : H * 128].reshape(2, rows, H, 128)
    want, bound = R.qk_rmsnorm_rope_ref(x, d["wq"], d["eps"], d["cos"], d["sin"])
    _judge(f"qk_rmsnorm_rope{case}", want, bound, R.qk_rmsnorm_rope_f32(x, d["wq"], d["eps"], d["cos"], d["sin"]),
           R.qk_rmsnorm_rope_f32(x, d["wq"], d["eps"], d["cos"], d["sin"], drop=True))


@pytest.mark.parametrize("case", R.MEAN_CASES, ids=str)
def test_mean_rows_bound(case):
    x = R.mean_inputs(*case)
    want, bound = R.mean_rows_ref(x)
    _judge(f"mean_rows{case}", want, bound, R.mean_rows_f32(x), R.mean_rows_f32(x, drop=True))


@pytest.mark.parametrize("case", R.GATE_CASES, ids=str)
def test_gate_residual_bound(case):
    d = R.gate_inputs(*case)
    want, bound = R.gate_residual_ref(**d)
    _judge(f"gate_residual{case}", want, bound, R.gate_residual_f32(**d))


@pytest.mark.parametrize("case", R.LS_CASES, ids=str)
def test_linear_small_bound(case):
    kw = R.ls_inputs(*case)
    want, bound = R.linear_small_ref(**kw)
    K = kw["W"].shape[1]
    _judge(f"linear_small{case}", want, bound, R.linear_small_f32(**kw), R.linear_small_f32(**kw, drop=True) if K > 4 else None)


def test_timestep_embedding_bound():
    t = torch.tensor(R.TIMESTEPS)
    want, bound = R.timestep_embedding_ref(t)
    _judge("timestep_embedding", want, bound, R.timestep_embedding_f32(t))
    from oracle.layers import get_timestep_embedding

    print(f"timestep_embedding: oracle {rz.assert_elementwise(get_timestep_embedding(t, 256), want, bound, 'oracle.layers.get_timestep_embedding'):.3f}")


@pytest.mark.parametrize("case", R.TEMB_CASES, ids=str)
def test_temb_modulate_bound(case):
    d = R.temb_inputs(*case)
    want, bound = R.temb_modulate_ref(**d)
    _judge(f"temb_modulate{case}", want, bound, R.temb_modulate_f32(**d))


@pytest.mark.parametrize("case", R.RMS_CASES, ids=str)
def test_rmsnorm_rows_bound(case):
    kw = R.rms_inputs(*case)
    want, bound = R.rmsnorm_rows_ref(**kw)
    _judge(f"rmsnorm_rows{case}", want, bound, R.rmsnorm_rows_f32(**kw), R.rmsnorm_rows_f32(**kw, drop=True))


@pytest.mark.parametrize("case", [c for c in R.UNSHUF_CASES if c[4] is not None], ids=str)
def test_pixel_unshuffle_shortcut_bound(case):
    kw = R.unshuf_inputs(*case)
    want, bound = R.pixel_unshuffle_shortcut_ref(**kw)
    G = 4 * case[4] // case[3]
    _judge(f"pixel_unshuffle_shortcut{case}", want, bound, R.pixel_unshuffle_shortcut_f32(**kw), R.pixel_unshuffle_shortcut_f32(**kw, drop=True) if G > 1 else None)


@pytest.mark.parametrize("case", R.REGROUP_DOWN, ids=str)
def test_chan_regroup_down_bound(case):
    M, cin, cout = case
    x = R.rows_input(1, M, cin, 41 + M)[0]
    want, bound = R.chan_regroup_down_ref(x, cout)
    _judge(f"chan_regroup{case}", want, bound, R.chan_regroup_down_f32(x, cout), R.chan_regroup_down_f32(x, cout, drop=True) if cin > cout else None)


@pytest.mark.parametrize("case", R.GCONV_CASES, ids=str)
def test_grouped_conv1x1_bound(case):
    kw = R.gconv_inputs(*case)
    want, bound = R.grouped_conv1x1_ref(**kw)
    _judge(f"grouped_conv1x1{case}", want, bound, R.grouped_conv1x1_f32(**kw), R.grouped_conv1x1_f32(**kw, drop=True))


@pytest.mark.parametrize("case", R.RLA_CASES, ids=str)
def test_relu_linear_attn_bound(case):
    B, P, groups, kind = case
    qkv = R.rla_inputs(*case)
    want, bound = R.relu_linear_attn_ref(qkv, groups, 1e-15)
    if kind == "zero_k":
        assert (want[..., :32] == 0).all()
    if kind == "zero_q":
        assert (want[0, P // 2, :32] == 0).all()
    _judge(f"relu_linear_attn{case}", want, bound, R.relu_linear_attn_f32(qkv, groups, 1e-15), R.relu_linear_attn_f32(qkv, groups, 1e-15, drop=True) if P > 1 else None)


@pytest.mark.parametrize("case", R.DW_CASES, ids=str)
def test_sphere_dwconv_bound(case):
    kw = R.dw_inputs(*case)
    want, bound = R.sphere_dwconv_ref(**kw)
    _judge(f"sphere_dwconv{case}", want, bound, R.sphere_dwconv_f32(**kw), R.sphere_dwconv_f32(**kw, drop=True))


@pytest.mark.parametrize("act", [1, 2])
def test_activation_bounds_reach_the_tails(act):
    v = torch.cat([torch.linspace(-30, 30, 2401), torch.tensor([-30.0, 30.0, 0.0, 1e-6, -1e-6])]).float()
    want, bound = rz.act_ref(v.double(), torch.zeros_like(v, dtype=torch.float64), act)
    _judge(f"act {act} on [-30, 30]", want, bound, R._act_f32(v, act))


# ---- redzone on itself ----------------------------------------------------------------------------------------------------------
def test_redzone_names_every_region():
    mk = lambda: rz.guarded(3, 5, 8, batch=2, batch_stride=40, align_bytes=32, device="cpu")  # noqa: E731
    g = mk()
    assert g.view.data_ptr() % 32 == 0 and g.view.shape == (2, 3, 5) and g.front >= rz.GUARD
    assert not torch.isfinite(g.payload()).any()  # UNWRITTEN
    g.fill(torch.arange(30.0))
    rz.assert_untouched(g)
    assert torch.equal(g.payload().reshape(-1), torch.arange(30.0))
    for off, name in ((g.front - 1, "front guard"), (0, "front guard"), (g.front + 5, "pad of row 0 of batch 0"), (g.front + 8 + 7, "pad of row 1 of batch 0"),
                      (g.front + 24, "gap after batch 0"), (g.front + 39, "gap after batch 0"), (g.front + 40 + 8 + 6, "pad of row 1 of batch 1"),
                      (g.front + g.span, "back guard"), (g.flat.numel() - 1, "back guard")):
        h = mk()
        h.flat[off] = 1.0
        with pytest.raises(AssertionError, match=f"{name} overwritten: first offending word at flat offset {off} "):
            rz.assert_untouched(h, "self-test")
    h = mk()
    h.flat.view(torch.int32)[h.front + 6] = rz.UNWRITTEN32  # another NaN is still a write: the comparison is on the bits
    with pytest.raises(AssertionError, match="pad of row 0"):
        rz.assert_untouched(h)
    d = rz.guarded(1, 7, dtype=torch.float64, device="cpu")
    rz.assert_untouched(d)
    d.flat[d.front + 7] = 0.0
    with pytest.raises(AssertionError, match="back guard"):
        rz.assert_untouched(d)


def test_operand_row_images():
    x = R.rows_input(1, 3, 12, 3)[0]
    img = rz.operand_rows(x, rz.FMT_SPLIT)
    assert img.shape == (3, 16) and rz.operand_width(12, rz.FMT_SPLIT) == 16 and rz.operand_width(12, rz.FMT_BF16) == 8
    b = img.view(torch.bfloat16).reshape(3, 2, 2, 8).float()  # [row][group][hi | lo][8]
    back = (b[:, :, 0] + b[:, :, 1]).reshape(3, 16)
    assert (back[:, 12:] == 0).all() and ((back[:, :12] - x).abs() <= x.abs() * 2.0 ** -16).all()
    assert torch.equal(rz.operand_rows(x, rz.FMT_BF16).view(torch.bfloat16)[:, :12], x.bfloat16())
