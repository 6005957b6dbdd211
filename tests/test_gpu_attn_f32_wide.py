"""The exact-fp32 attention after its two trims - staging loads addressed from a wave-uniform row base (rows past S clamped, on the last key
tile only) and the deferred rescale (O and l follow a query's maximum only when a tile exceeds the applied maximum by more than the
threshold) - kernel level, through the C ABI.  Every case runs with the library's threshold (8) and with threshold 0
(ldc_attn_fwd_ws_qrows_thr), with the workspace (balanced cut where the rule takes it) and, where named, without.

Inputs are built as the attention cases of tests/test_gpu_ops.py build theirs (seeded normal q / k / v, q x 2); the oracle is float64
softmax(Q K^T / sqrt(128) + bias) V on the CPU, computed once per input and shared.  Bound: the rel-L2 2e-6 of those cases
(tests/test_gpu_ops.py::test_attention / test_attention_f32_balanced_schedule, tests/test_gpu_attn_query_rows.py MODES["fp32"]).

Shapes (B, S, H, Sq) and what they hit:
  (1,  70, 1,  70)  one unit, ragged in rows and in the last key tile (the clamped staging arm with 6 live rows of 32)
  (1, 257, 2, 257)  the third unit of a head holds one row; the last key tile holds one key
  (1, 300, 2, 130)  queries fewer than keys
  (2, 700, 4, 700)  48 units of 22 key tiles = 1056 items: the balanced cut with 4-tile ranges, every unit merged from 5 or 6 pieces
  (1, 512, 2, 512)  with a key bias; S a multiple of the tile (the clamped arm never runs)
  (4, 512, 16, 512) 256 units: whole rounds, the one-unit-per-workgroup 4-wave grid
The rescale branch is rare on random data, so it has inputs of its own (rule: a rare data-dependent branch needs its own test): a spiked
key late in a unit's first piece and late in a later piece, a key that holds every query's maximum in tile 0, and threshold 0 against the
library's threshold.

(The file is named for the wide form - one wave per SIMD, 64 query rows per wave - that these trims were to go with; that form measured
slower on every launch class and is not in the tree: profiles/attn_f32_wide_rejected.log.)"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_ops import dev, hip, rel, rnd  # noqa: E402,F401  (`hip`: the module fixture of the op tests)

TOL = 2e-6
SENTINEL = -12345.678
THRS = {"thr8": None, "thr0": 0.0}  # None: the library's entry point and threshold


@functools.lru_cache(maxsize=None)
def _inputs(B, H, S, bias, spike=None):
    """spike = (query row, key row, nats): k[key] of (batch 0, head 0) is set along q[query] so that their score is `nats`"""
    D = H * 128
    qkv = rnd(B, S, 3 * D, seed=11)
    qkv[..., :D] *= 2.0
    if spike is not None:
        for qrow, key, nats in spike:
            q = qkv[0, qrow, :128]
            qkv[0, key, D : D + 128] = q * (nats * 128.0**0.5 / float(q.double().dot(q.double())))
    kb = None
    if bias == "random":
        kb = 0.5 * rnd(S, seed=32)
    elif bias == "key0":  # key 0 holds every query's maximum: nothing rescales after tile 0
        kb = torch.zeros(S)
        kb[0] = 60.0
    return qkv, kb


@functools.lru_cache(maxsize=None)
def _oracle(B, H, S, Sq, bias, spike=None):
    qkv, kb = _inputs(B, H, S, bias, spike)
    D = H * 128
    q, k, v = [t.reshape(B, S, H, 128).transpose(1, 2).double() for t in qkv.split(D, dim=-1)]
    s = q[:, :, :Sq] @ k.transpose(-1, -2) / 128.0**0.5
    if kb is not None:
        s = s + kb.double().view(1, 1, 1, S)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, Sq, D)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(hip, B, H, S, Sq, bias, thr, spike=None, use_workspace=True):
    """-> (flat buffer with one guard row, [B, S, ld] view of it): O rows [0, Sq), columns [0, D) written, the rest sentinel"""
    D, ld = H * 128, H * 128 + 64
    qkv, kb = _inputs(B, H, S, bias, spike)
    d_qkv = dev(qkv)
    flat = torch.full((B * S + 1, ld), SENTINEL, device="cuda")
    o = flat[: B * S].view(B, S, ld)
    hip.attn_fwd(d_qkv[:, :, :D], d_qkv[:, :, D : 2 * D], d_qkv[:, :, 2 * D :], o, B=B, S=S, H=H, ld_qkv=3 * D, qkv_bs=S * 3 * D, ldo=ld,
                 o_bs=S * ld, key_bias=None if kb is None else dev(kb), Sq=Sq, rescale_thr=thr, use_workspace=use_workspace)
    torch.cuda.synchronize()
    return flat, o


def _check(flat, o, want, Sq, D, what):
    err = rel(o[:, :Sq, :D], want)
    print(f"\n{what}: rel-L2 vs fp64 {err:.3e} (bound {TOL:g})")
    assert torch.isfinite(o[:, :Sq, :D]).all()
    assert err < TOL
    sent = _bits(torch.full((1,), SENTINEL, device="cuda"))[0]
    assert bool((_bits(o[:, Sq:]) == sent).all() and (_bits(o[:, :, D:]) == sent).all() and (_bits(flat[-1]) == sent).all())


def _counters_zero(hip):
    ws = hip._attn_f32_workspace(torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    return int(ws[:65536].view(torch.int32).abs().sum().item()) == 0


@pytest.mark.parametrize("use_workspace", [True, False])
@pytest.mark.parametrize("thr", list(THRS))
@pytest.mark.parametrize("B,S,H,Sq,bias", [(1, 70, 1, 70, None), (1, 257, 2, 257, None), (1, 300, 2, 130, None), (1, 512, 2, 512, "random")])
def test_trims_small_shapes(hip, B, S, H, Sq, bias, thr, use_workspace):
    flat, o = _run(hip, B, H, S, Sq, bias, THRS[thr], use_workspace=use_workspace)
    _check(flat, o, _oracle(B, H, S, Sq, bias), Sq, H * 128, f"{thr}, workspace {use_workspace}, B {B} S {S} H {H} Sq {Sq} bias {bias}")
    assert _counters_zero(hip)


@pytest.mark.parametrize("thr", list(THRS))
def test_trims_balanced_cut_repeatable(hip, thr):
    B, S, H = 2, 700, 4
    first = _run(hip, B, H, S, S, None, THRS[thr])
    again = _run(hip, B, H, S, S, None, THRS[thr])  # the same workspace, nothing re-zeroed in between
    _check(*first, _oracle(B, H, S, S, None), S, H * 128, f"{thr}, balanced cut, B {B} S {S} H {H}")
    assert torch.equal(_bits(first[1]), _bits(again[1]))
    assert _counters_zero(hip)


@pytest.mark.parametrize("thr", list(THRS))
def test_trims_whole_rounds_unbalanced(hip, thr):
    B, S, H = 4, 512, 16
    flat, o = _run(hip, B, H, S, S, None, THRS[thr])
    _check(flat, o, _oracle(B, H, S, S, None), S, H * 128, f"{thr}, 256 units, one per workgroup")
    assert _counters_zero(hip)


# (2, 700, 4) cut into 256 ranges: 1056 items, the first 32 ranges hold 5 tiles, so unit 0 (batch 0, head 0, rows 0..127) is the pieces
# [0-4] [5-9] [10-14] [15-19] [20-21]; a piece's tiles go half to each wave group (tiles 0-2 | 3-4, 10-12 | 13-14): key 69 (tile 2) is the last
# tile of group 0 in the first piece, key 135 (tile 4) the last of group 1 there, key 455 (tile 14) the last of group 1 in the third piece
SPIKES = {"first_piece": ((5, 69, 40.0), (70, 135, 40.0)), "later_piece": ((37, 455, 40.0),),
          "all": ((5, 69, 40.0), (70, 135, 40.0), (37, 455, 40.0), (100, 690, 55.0))}


@pytest.mark.parametrize("use_workspace", [True, False])
@pytest.mark.parametrize("thr", list(THRS))
@pytest.mark.parametrize("spike", list(SPIKES))
def test_trims_rescale_spike(hip, spike, thr, use_workspace):
    B, S, H = 2, 700, 4
    flat, o = _run(hip, B, H, S, S, None, THRS[thr], spike=SPIKES[spike], use_workspace=use_workspace)
    _check(flat, o, _oracle(B, H, S, S, None, SPIKES[spike]), S, H * 128, f"{thr}, workspace {use_workspace}, spiked keys {spike}")
    for qrow, key, _ in SPIKES[spike]:  # the spiked query really is one-hot on its key: the branch was taken for something
        v = _inputs(B, H, S, None, SPIKES[spike])[0][0, key, 2 * H * 128 : 2 * H * 128 + 128]
        assert rel(o[0, qrow, :128], v) < 1e-3
    assert _counters_zero(hip)


@pytest.mark.parametrize("use_workspace", [True, False])
def test_trims_maximum_fixed_after_first_tile(hip, use_workspace):
    B, S, H = 1, 512, 2
    for thr in (None, 0.0):
        flat, o = _run(hip, B, H, S, S, "key0", thr, use_workspace=use_workspace)
        _check(flat, o, _oracle(B, H, S, S, "key0"), S, H * 128, f"threshold {thr}, key 0 holds every maximum, workspace {use_workspace}")


@pytest.mark.parametrize("B,S,H,bias", [(2, 700, 4, None), (1, 512, 2, "random")])
def test_trims_threshold_zero_agrees(hip, B, S, H, bias):
    want = _oracle(B, H, S, S, bias)
    _, o8 = _run(hip, B, H, S, S, bias, None)
    _, o8b = _run(hip, B, H, S, S, bias, 8.0)
    _, o0 = _run(hip, B, H, S, S, bias, 0.0)
    assert torch.equal(_bits(o8), _bits(o8b))  # the library's threshold is 8
    e8, e0, d = rel(o8[:, :, : H * 128], want), rel(o0[:, :, : H * 128], want), rel(o8[:, :, : H * 128], o0[:, :, : H * 128])
    print(f"\nthreshold 8 vs fp64 {e8:.3e}, threshold 0 vs fp64 {e0:.3e}, 8 vs 0 {d:.3e} (bound {TOL:g})")
    assert e8 < TOL and e0 < TOL and d < TOL


def test_trims_rejects_bad_threshold(hip):
    x = torch.zeros(1, 64, 3 * 128, device="cuda")
    o = torch.zeros(1, 64, 128, device="cuda")
    for bad in (-1.0, 65.0, float("nan")):
        with pytest.raises(RuntimeError):
            hip.attn_fwd(x[:, :, :128], x[:, :, 128:256], x[:, :, 256:], o, B=1, S=64, H=1, ld_qkv=384, qkv_bs=64 * 384, ldo=128, o_bs=64 * 128, rescale_thr=bad)
