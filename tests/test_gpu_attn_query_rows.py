"""Attention with fewer queries than keys (ldc_attn_fwd_qrows / ldc_attn_fwd_ws_qrows / ldc_attn_fwd_split_qrows): the queries are the
first Sq of the S token rows, keys and values are all S rows, rows >= Sq of O are not touched.  Kernel level, through the C ABI.

Inputs are built as the attention cases of tests/test_gpu_ops.py build theirs (seeded normal q / k / v, q x 2 for the exact-fp32 kernel,
q x 4 and `attn_qkv_prepare_split` for the split kernel); the oracle is fp64 softmax attention on the CPU over the same rows, computed
once per (shape, input recipe, bias) and shared by the modes.  Tolerances: the ones those cases use per mode.

Shapes (B, H, S, Sq) and what they hit:
  1  (1,  2,  330,  330)  Sq = S: bit for bit the old entry point
  2  (2,  2,  330,  200)  Sq and S both ragged
  3  (1,  1,  450,    8)  less than one fragment row of queries
  4  (1,  3,  450,  256)  whole query tiles, ragged keys
  5  (1, 12,  450,  200)  24 units (two wave groups per unit).  With 15 key tiles these are 360 (unit, key tile) items, below the 512 the
                          balanced rule of the exact-fp32 kernel asks for, so fp32 runs the plain 8-wave grid here - case 7 is the balanced one
  6  (2, 12, 1920, 1500)  288 units: the split kernel's persistent form with its key-sliced tail and merge; the exact-fp32 kernel's
                          balanced cut with partial units and a ragged last query tile (92 rows)
  7  (1, 12, 1100,  200)  24 units of 35 key tiles = 840 items: the balanced cut of the exact-fp32 kernel with 3.3-tile ranges (every
                          unit in pieces), a ragged last query tile (72 rows) and ragged keys
Bit equality between a restricted and a full launch is not asked for: the balanced cut and the unit count legitimately differ."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_ops import _prep, _unsplit, dev, hip, rel, rnd  # noqa: E402,F401  (`hip`: the module fixture of the op tests)

CASES = [(1, 2, 330, 330), (2, 2, 330, 200), (1, 1, 450, 8), (1, 3, 450, 256), (1, 12, 450, 200), (2, 12, 1920, 1500), (1, 12, 1100, 200)]
# per mode: (q gain of the input recipe, rel-L2 bound) - tests/test_gpu_ops.py::test_attention / test_attention_f32_balanced_schedule
# (2e-6), ::test_attention_split / test_attention_split_tail_schedule (2e-5 three-term, 1e-2 single-term)
MODES = {"fp32": (2.0, 2e-6), "split3": (4.0, 2e-5), "split1": (4.0, 1e-2)}
SENTINEL = -12345.678


@functools.lru_cache(maxsize=None)
def _inputs(B, H, S, gain, bias):
    D = H * 128
    qkv = rnd(B, S, 3 * D, seed=11)
    qkv[..., :D] *= gain
    kb = 0.5 * rnd(S, seed=32) if bias else None
    return qkv, kb


@functools.lru_cache(maxsize=None)
def _oracle(B, H, S, Sq, gain, bias):
    """fp64 softmax attention of queries [0, Sq) over all S keys -> [B, Sq, H * 128]"""
    qkv, kb = _inputs(B, H, S, gain, bias)
    D = H * 128
    q, k, v = [t.reshape(B, S, H, 128).transpose(1, 2).double() for t in qkv.split(D, dim=-1)]
    s = q[:, :, :Sq] @ k.transpose(-1, -2) / 128.0**0.5
    if kb is not None:
        s = s + kb.double().view(1, 1, 1, S)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Sq, D)


def _buffer(B, S, ld):
    """[B, S, ld] output filled with a sentinel, plus one guard row behind it (same allocation)"""
    flat = torch.full((B * S + 1, ld), SENTINEL, device="cuda")
    return flat, flat[: B * S].view(B, S, ld)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(flat, out, Sq, D):
    """rows >= Sq, the pad columns of every row and the guard row still hold the sentinel, bit for bit"""
    want = _bits(torch.full((1,), SENTINEL, device="cuda"))[0]
    return bool((_bits(out[:, Sq:]) == want).all() and (_bits(out[:, :, D:]) == want).all() and (_bits(flat[-1]) == want).all())


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B,H,S,Sq", CASES)
def test_attention_query_rows(hip, B, H, S, Sq, mode, bias):
    gain, tol = MODES[mode]
    D, ld = H * 128, H * 128 + 64
    qkv, kb = _inputs(B, H, S, gain, bias)
    want = _oracle(B, H, S, Sq, gain, bias)
    d_qkv = dev(qkv)
    q, k, v = d_qkv[:, :, :D], d_qkv[:, :, D : 2 * D], d_qkv[:, :, 2 * D :]
    kw = dict(B=B, S=S, H=H, ld_qkv=3 * D, qkv_bs=S * 3 * D, ldo=ld, o_bs=S * ld)
    if mode == "fp32":
        launch = lambda o, **extra: hip.attn_fwd(q, k, v, o, key_bias=None if kb is None else dev(kb), **dict(kw, **extra))  # noqa: E731
    else:
        _prep(hip, d_qkv, B, S, H, D, split_row=S)
        kbp = None if kb is None else hip.pad_key_bias(dev(kb))
        launch = lambda o, **extra: hip.attn_fwd_split(q, k, v, o, key_bias=kbp, one_term=mode == "split1", **dict(kw, **extra))  # noqa: E731

    # two launches in a row on the same workspace, nothing re-zeroed in between
    outs = []
    for _ in range(2):
        flat, o = _buffer(B, S, ld)
        launch(o, Sq=Sq)
        outs.append((flat, o))
    flat, out = outs[0]
    err = rel(out[:, :Sq, :D], want)
    print(f"\nattention, {Sq} of {S} query rows, B {B} H {H}, {mode}{' + key bias' if bias else ''}: rel-L2 vs fp64 {err:.3e} (bound {tol:g})")
    assert torch.isfinite(out[:, :Sq, :D]).all()
    assert err < tol
    assert _untouched(flat, out, Sq, D) and _untouched(outs[1][0], outs[1][1], Sq, D)
    assert torch.equal(_bits(out), _bits(outs[1][1]))
    if mode == "fp32":  # the ticket counters of the balanced schedule (the split kernel's workspace holds partial results only: no counters)
        ws = hip._attn_f32_workspace(d_qkv.device)
        torch.cuda.synchronize()
        assert int(ws[:65536].view(torch.int32).abs().sum().item()) == 0
    if Sq == S:  # the old entry point is this code with Sq = S
        flat0, o0 = _buffer(B, S, ld)
        launch(o0)
        assert torch.equal(_bits(o0), _bits(out))

    if mode != "fp32":  # the other output formats: exactly the split / the bf16 rounding of the fp32 rows, rows >= Sq untouched
        fmt = hip.FMT_BF16 if mode == "split1" else True
        flat2, o2 = _buffer(B, S, ld)
        launch(o2, Sq=Sq, out_split=fmt)
        w = out[:, :Sq, :D].cpu().reshape(B * Sq, D)
        if mode == "split1":
            got = (o2.view(torch.int16)[:, :Sq, :D].to(torch.int32) << 16).view(torch.float32)
            assert torch.equal(got.cpu().reshape(B * Sq, D), w.bfloat16().float())
            want_bits = _bits(torch.full((1,), SENTINEL, device="cuda"))[0]
            assert bool((_bits(o2[:, Sq:]) == want_bits).all() and (_bits(o2[:, :Sq, (D + 1) // 2 :]) == want_bits).all() and (_bits(flat2[-1]) == want_bits).all())
        else:
            hi, lo = _unsplit(o2[:, :Sq, :D].contiguous().reshape(B * Sq, D), B * Sq, D)
            assert torch.equal(hi, w.bfloat16().float()) and torch.equal(lo, (w - w.bfloat16().float()).bfloat16().float())
            assert _untouched(flat2, o2, Sq, D)


def test_attention_query_rows_schedules(hip):
    """the shapes above do take the schedules their rows name: units are counted from Sq, not from S"""
    wsb = hip.lib.ldc_attn_fwd_split_qrows_workspace_bytes
    assert wsb(2, 1920, 1500, 12) > 0  # 288 units: persistent form + tail
    assert wsb(1, 2250, 2250, 16) == hip.lib.ldc_attn_fwd_split_workspace_bytes(1, 2250, 16) > 0  # Sq = S is the old call
    assert wsb(1, 2250, 1800, 16) == 0  # 240 units fit one round
    assert wsb(1, 450, 0, 1) == 0 and wsb(1, 450, 451, 1) == 0


def test_attention_query_rows_rejects_bad_counts(hip):
    D = 128
    x = torch.zeros(1, 64, 3 * D, device="cuda")
    o = torch.zeros(1, 64, D, device="cuda")
    kw = dict(B=1, S=64, H=1, ld_qkv=3 * D, qkv_bs=64 * 3 * D, ldo=D, o_bs=64 * D)
    for fn in (hip.attn_fwd, hip.attn_fwd_split, functools.partial(hip.attn_fwd, use_workspace=False)):
        for bad in (0, -1, 65):
            with pytest.raises(RuntimeError):
                fn(x[:, :, :D], x[:, :, D : 2 * D], x[:, :, 2 * D :], o, Sq=bad, **kw)
