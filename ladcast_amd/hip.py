"""ctypes binding of the C ABI in ``include/ladcast_hip.h``, generated from that header.

``ladcast_amd.abi`` reads the header at import: its prototypes become ``SIGNATURES`` (restype and argtypes of every entry point) and
its ``ldc_*`` structs the ``ctypes.Structure`` classes named below.  That header's set of entry points is recorded and held by the ABI
tests, so a new entry point needs its prototype in ``include/ladcast_hip_ext.h`` (read into ``abi.EXT_SIGNATURES`` and bound here
alongside) and a wrapper here, nothing else.  The constants stay literals, since call sites read them by name; tests/test_abi_cpu.py
holds them to the header.

PyTorch is plumbing here: it owns device memory and the HIP stream.  Every wrapper takes
torch CUDA(=HIP) tensors, passes raw device pointers + sizes + the current stream to the
shared library and raises ``RuntimeError`` on a non-zero status.  Importing this module
without the built library raises immediately -- the product path never falls back to
PyTorch ops.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int, c_void_p

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# LDC_LIB_PATH: diagnostic builds only (e.g. the in-kernel stamp build made by `make stamps`)
LIB_PATH = os.environ.get("LDC_LIB_PATH") or os.path.join(_HERE, "libladcast_hip.so")

ACT_NONE, ACT_SILU, ACT_GELU_TANH, ACT_RELU = 0, 1, 2, 3
ACT_IN_TIMESTEP_SINCOS = 16  # act_in of the small linears: x = one timestep per row, the input row = its sinusoidal embedding
GEMM_A_SPLIT, GEMM_C_SPLIT, GEMM_BF16_1TERM = 1, 2, 4
GEMM_F32_REGSTAGE = 8  # exact-fp32 problems: stay on the register-staged stream-K kernel (include/ladcast_hip.h)
ATTN_OUT_SPLIT, ATTN_BF16_1TERM, ATTN_OUT_BF16 = 1, 2, 4
ERR_UNSUPPORTED = -3  # LDC_ERR_UNSUPPORTED
ABI_VERSION = 5  # LDC_ABI_VERSION of include/ladcast_hip.h this binding was written against
FMT_F32, FMT_SPLIT, FMT_BF16 = 0, 1, 2  # activation formats of the producers' `out_split` arguments (True == FMT_SPLIT)
MAX_GROUPED = 4
GEMM_KERNEL_RING, GEMM_KERNEL_REGSTAGE = 0, 1  # LDC_GEMM_KERNEL_*
PRODUCTS_MAX_QUANTILES, PRODUCTS_MAX_THRESHOLDS, PRODUCTS_MAX_MEMBERS, PRODUCTS_MAX_SORT_MEMBERS = 16, 8, 1024, 64  # LDC_PRODUCTS_MAX_*
EVENTS_MAX, EVENTS_MAX_MEMBERS = 32, 1024  # LDC_EVENTS_MAX, the largest ensemble of ldc_rollout_events
FSS_SCALES_MAX, FSS_SUMS = 16, 6  # LDC_FSS_SCALES_MAX, the sums per (event, radius, lead time) of ldc_rollout_fss
DERIVE_MAX_FIELDS = 16  # LDC_DERIVE_MAX_FIELDS
DERIVE_SPEED, DERIVE_DIFF, DERIVE_SHEAR = 0, 1, 2  # LDC_DERIVE_*
DERIVE_INPUTS = {DERIVE_SPEED: 2, DERIVE_DIFF: 2, DERIVE_SHEAR: 4}  # source channels per kind
SPHERE_VORTICITY, SPHERE_DIVERGENCE = 0, 1  # LDC_SPHERE_*: fields of a wind (u, v) that need horizontal derivatives

# the header's structs: field names, order and types are the header's (a pointer field is a c_void_p)
GemmDesc = abi.STRUCTS["ldc_gemm_desc"]
GemmProblem = abi.STRUCTS["ldc_gemm_problem"]
GemmPlan = abi.STRUCTS["ldc_gemm_plan"]  # what a grouped GEMM call would run (per launch: tile_rows .. units_rem; per problem: the rest)
QkvEpilogue = abi.STRUCTS["ldc_qkv_epilogue"]
LinearSmallProblem = abi.STRUCTS["ldc_linear_small_problem"]
ProductsDesc = abi.STRUCTS["ldc_products_desc"]
DeriveDesc = abi.STRUCTS["ldc_derive_desc"]
SphereDesc = abi.STRUCTS["ldc_sphere_desc"]
EventsDesc = abi.STRUCTS["ldc_events_desc"]


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C ladcast_amd/csrc`).  ladcast_amd has no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (*abi.SIGNATURES.items(), *abi.EXT_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.ldc_abi_version() != ABI_VERSION:
        raise RuntimeError("libladcast_hip.so ABI version mismatch")
    for name, cls in abi.STRUCTS.items():  # every struct whose size the library reports, as its compiler laid it out
        size_of = "ldc_sizeof_" + name[len("ldc_"):]
        if size_of in abi.SIGNATURES and getattr(lib, size_of)() != ctypes.sizeof(cls):
            raise RuntimeError(f"{name} layout mismatch between header and binding")
    return lib


lib, SIGNATURES = _load(), abi.SIGNATURES


def _check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"{what} failed with status {status}")


def upload_nonblocking(t, device):
    """host -> device without stalling the host: a pageable source makes the copy synchronous, i.e. the host would wait for everything
    queued on the stream - the previous sampler chunk - before it can prepare the next one.  Pinned source + non_blocking: the copy
    is only stream-ordered (torch's pinned-memory allocator does not hand the block out again before the copy has run)."""
    device = torch.device(device)
    if device.type != "cuda" or t.device.type != "cpu":
        return t.to(device)
    return (t if t.is_pinned() else t.pin_memory()).to(device, non_blocking=True)


def _p(t):
    return None if t is None else c_void_p(t.data_ptr())


def _stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("ladcast_amd kernels need device tensors (no CPU fallback)")


# ---------------------------------------------------------------------------
def gemm(A, W, C, *, M, N, K, batch=1, lda=None, ldw=None, ldc=None, a_bs=0, c_bs=0, bias=None, gate=None,
         gate_bs=0, R=None, ldr=0, r_bs=0, act=ACT_NONE):
    """C[b] = epilogue(A[b] . W^T); A/C/R may be views (data_ptr carries the offset)."""
    _dev(A, W, C, bias, gate, R)
    d = GemmDesc(M, N, K, batch, lda if lda is not None else K, ldw if ldw is not None else K,
                 ldc if ldc is not None else N, ldr, a_bs, c_bs, r_bs, gate_bs, act, 0, 0)
    _check(lib.ldc_gemm_bias_act(_p(A), _p(W), _p(bias), _p(gate), _p(R), _p(C), ctypes.byref(d), _stream()), "ldc_gemm_bias_act")


_workspaces = {}  # (name, device, stream) -> fp32 tensor: every per-stream workspace of the library
_outgrown = []  # replaced blocks of a growing workspace: a captured hipGraph may still point at the smaller one


def _workspace(name, device, nbytes, init=None, grow=False):
    """The workspace `name` of the current stream of `device`, created at the first call: at least `nbytes` bytes, initialised by `init`
    (None: nothing | "zero": zero-filled | "grouped": ldc_gemm_grouped_workspace_init).  One per (device, stream): two streams never
    share one.  A fixed workspace (grow=False) is allocated ONCE and never replaced: its pointer is baked into every hipGraph captured
    on that stream, and graphs of several shapes stay alive side by side.  A first call inside a capture would take the block from the
    graph's private pool and publish it to eager callers, and put its initialisation into the graph: refused - whoever captures warms
    up on the capture stream first (`graphs.capture`).  A growing one (the scoring scratch) is replaced by a larger block when a call
    asks for more; the smaller block stays alive."""
    key = (name, str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or (grow and ws.numel() * 4 < nbytes):
        if not grow and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{name}: the first call on a stream must be made outside a graph capture (run one warm-up forward)")
        if ws is not None:
            _outgrown.append(ws)
        ws = torch.empty((nbytes + 3) // 4, device=device, dtype=torch.float32)
        if init == "zero":
            ws.zero_()
        elif init == "grouped":
            _check(lib.ldc_gemm_grouped_workspace_init(c_void_p(ws.data_ptr()), ws.numel() * 4, _stream()), "ldc_gemm_grouped_workspace_init")
        _workspaces[key] = ws
    return ws


def _grouped_workspace(device):
    """stream-K tile counters (first MiB, zeroed once; every launch re-arms them) + partial-tile slabs of every grouped GEMM and conv"""
    return _workspace("gemm_grouped", device, lib.ldc_gemm_grouped_workspace_bytes(), init="grouped")


def gemm_problem(A, W, C, *, M, N, K, batch=1, lda=None, ldw=None, ldc=None, a_bs=0, c_bs=0, bias=None, gate=None, gate_bs=0, R=None,
                 ldr=0, r_bs=0, act=ACT_NONE, flags=0):
    """one entry of a grouped launch (same argument meaning as `gemm`); flags: GEMM_A_SPLIT | GEMM_C_SPLIT (bf16x3 only); GEMM_F32_REGSTAGE
    (exact fp32 only): the register-staged kernel instead of the ring kernel"""
    _dev(A, W, C, bias, gate, R)
    d = GemmDesc(M, N, K, batch, lda if lda is not None else K, ldw if ldw is not None else K, ldc if ldc is not None else N, ldr,
                 a_bs, c_bs, r_bs, gate_bs, act, flags, 0)
    pv = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return GemmProblem(pv(A), pv(W), pv(bias), pv(gate), pv(R), pv(C), d), (A, W, C, bias, gate, R)


def gemm_grouped(problems, split_bf16=False):
    """Up to MAX_GROUPED independent GEMMs in one persistent stream-K launch (split tiles are reduced inside the launch).
    split_bf16: every problem's W is a `pack_weight_bf16x2` buffer and the bf16x3 kernel is used."""
    n = len(problems)
    if not 1 <= n <= MAX_GROUPED:
        raise ValueError(f"gemm_grouped takes 1..{MAX_GROUPED} problems")
    arr = (GemmProblem * n)(*[p[0] for p in problems])
    ws = _grouped_workspace(problems[0][1][2].device)
    fn = lib.ldc_gemm_grouped_bf16x3 if split_bf16 else lib.ldc_gemm_grouped
    _check(fn(arr, n, c_void_p(ws.data_ptr()), ws.numel() * 4, _stream()), "ldc_gemm_grouped" + ("_bf16x3" if split_bf16 else ""))


def _gemm_plan(problems, epilogues, split_bf16):
    n = len(problems)
    if not 1 <= n <= MAX_GROUPED or (epilogues is not None and len(epilogues) != n):
        raise ValueError(f"gemm_plan takes 1..{MAX_GROUPED} problems and, with epilogues, one (or None) per problem")
    arr = (GemmProblem * n)(*[p[0] for p in problems])
    epi = None if epilogues is None else (QkvEpilogue * n)(*[(e[0] if e is not None else QkvEpilogue()) for e in epilogues])
    plan = GemmPlan()
    return lib.ldc_gemm_grouped_plan(arr, epi, n, int(bool(split_bf16)), lib.ldc_gemm_grouped_workspace_bytes(), ctypes.byref(plan)), plan


def gemm_plan(problems, epilogues=None, split_bf16=False):
    """What `gemm_grouped(problems, split_bf16)` - with `epilogues`: `gemm_grouped_qkv_f32` | `gemm_grouped_qkv` - would run with this
    binding's workspace, as a `GemmPlan` (ldc_gemm_grouped_plan): kernel, tile height, launches, each launch's cut.  Launches nothing and
    reads no buffer (CPU only: only the addresses' alignment matters); raises with the status the launch would fail with."""
    st, plan = _gemm_plan(problems, epilogues, split_bf16)
    _check(st, "ldc_gemm_grouped_plan")
    return plan


def gemm_kernel_name(problems, epilogues=None, split_bf16=False):
    """the kernel instance that serves the call, as a profiler prints it (of a group launched problem by problem: the first launch's).
    Where the fused-QKV launch is not served (LDC_ERR_UNSUPPORTED: nothing is launched, the callers run the plain grouped GEMM
    instead) the plain GEMM's."""
    st, plan = _gemm_plan(problems, epilogues, split_bf16)
    if st == ERR_UNSUPPORTED and epilogues is not None:
        st, plan = _gemm_plan(problems, None, split_bf16)
    _check(st, "ldc_gemm_grouped_plan")
    if plan.kernel == GEMM_KERNEL_RING:
        return f"gemm_bf16x3_v3_kernel<{plan.tile_rows[0]}, {plan.terms}, false>"
    return "gemm_streamk_bf16x3_kernel" if split_bf16 else "gemm_streamk_kernel"


def gemm_sk(A, W, C, split_bf16=False, **kw):
    """single GEMM through the stream-K scheduler"""
    gemm_grouped([gemm_problem(A, W, C, **kw)], split_bf16=split_bf16)


def pack_weight_bf16x2(W):
    """fp32 [N, K] (K % 8 == 0) -> packed split-bf16 weight buffer (int32 view, N*K elements = same bytes)"""
    _dev(W)
    W = W.contiguous()
    N, K = W.shape
    out = torch.empty(N * K, device=W.device, dtype=torch.int32)
    _check(lib.ldc_pack_weight_bf16x2(_p(W), _p(out), N, K, K, _stream()), "ldc_pack_weight_bf16x2")
    return out


def pack_weight_bf16(W):
    """fp32 [N, K] (K % 8 == 0) -> plain bf16 [N, K] weight buffer (the W operand of the single-term bf16 mode)"""
    _dev(W)
    W = W.contiguous()
    N, K = W.shape
    out = torch.empty(N * K, device=W.device, dtype=torch.bfloat16)
    _check(lib.ldc_pack_weight_bf16(_p(W), _p(out), N, K, K, _stream()), "ldc_pack_weight_bf16")
    return out


def linear_small(x, W, y, *, rows, N, K, x_rows=None, bias=None, add=None, add_rows=1, act_in=ACT_NONE, act_out=ACT_NONE, mod=None, mod_rows=1):
    """mod ([mod_rows][2 N]): y = y * (1 + mod[:, :N]) + mod[:, N:] as the epilogue (ldc_linear_small_mod)"""
    _dev(x, W, y, bias, add, mod)
    xr = x_rows if x_rows is not None else rows
    if mod is not None:
        _check(lib.ldc_linear_small_mod(_p(x), xr, _p(W), _p(bias), _p(add), add_rows, _p(mod), mod_rows, _p(y), rows, N, K, act_in, act_out, _stream()),
               "ldc_linear_small_mod")
        return
    _check(lib.ldc_linear_small(_p(x), xr, _p(W), _p(bias), _p(add), add_rows, _p(y), rows, N, K, act_in, act_out, _stream()), "ldc_linear_small")


def gate_residual_layernorm(resid, y, gate, out, *, B, rows, D, ld_res, res_bs, ld_y, y_bs, gate_bs, ld_out, out_bs, weight, bias, eps, out_split=False):
    """resid += gate * y in place, then out = LayerNorm(resid) * weight + bias (one launch)"""
    _dev(resid, y, gate, out, weight, bias)
    _check(lib.ldc_gate_residual_layernorm(_p(resid), _p(y), _p(gate), _p(out), B, rows, D, ld_res, res_bs, ld_y, y_bs, gate_bs, ld_out, out_bs,
                                           _p(weight), _p(bias), eps, int(out_split), _stream()), "ldc_gate_residual_layernorm")


LINEAR_SMALL_MAX_GROUPED = 4  # LDC_LINEAR_SMALL_MAX_GROUPED


def linear_small_problem(x, W, y, *, rows, N, K, x_rows=None, bias=None, add=None, add_rows=1, act_in=ACT_NONE, act_out=ACT_NONE):
    """one entry of linear_small_grouped (same arguments as linear_small)"""
    _dev(x, W, y, bias, add)
    q = LinearSmallProblem(_p(x), _p(W), _p(bias), _p(add), _p(y), x_rows if x_rows is not None else rows, add_rows, rows, N, K, act_in, act_out, 0)
    return q, (x, W, y, bias, add)


def linear_small_grouped(problems):
    """up to LINEAR_SMALL_MAX_GROUPED independent small linears in one launch"""
    n = len(problems)
    if not 1 <= n <= LINEAR_SMALL_MAX_GROUPED:
        raise ValueError(f"linear_small_grouped takes 1..{LINEAR_SMALL_MAX_GROUPED} problems")
    arr = (LinearSmallProblem * n)(*[p[0] for p in problems])
    _check(lib.ldc_linear_small_grouped(arr, n, _stream()), "ldc_linear_small_grouped")


def _attn_f32_workspace(device):
    """counters + slabs of the exact-fp32 attention's balanced schedule (ldc_attn_fwd_ws), zero-filled once (the launches leave the
    counters zero)"""
    return _workspace("attn_fwd", device, lib.ldc_attn_fwd_workspace_bytes(), init="zero")


def attn_fwd(Q, K, V, O, *, B, S, H, ld_qkv, qkv_bs, ldo, o_bs, key_bias=None, use_workspace=True, Sq=None, rescale_thr=None):
    """exact-fp32 attention on fp32 q / k / v views (ldc_attn_fwd_ws); key_bias: [S] additive score bias per key (or None).
    use_workspace=False: never the balanced schedule (ldc_attn_fwd; A/B, tests).  Sq: the queries are the first Sq token rows only
    (keys / values: all S; rows >= Sq of O untouched; ldc_attn_fwd_qrows / _ws_qrows).  rescale_thr (tests, measurements): the deferred-rescale
    threshold of ldc_attn_fwd_ws_qrows_thr in log2 units (0: rescale at every new maximum); None: the library's"""
    _dev(Q, K, V, O, key_bias)
    if key_bias is not None and key_bias.numel() < S:
        raise ValueError("key_bias must hold one value per key")
    if rescale_thr is not None:
        ws = _attn_f32_workspace(Q.device) if use_workspace else None
        st = lib.ldc_attn_fwd_ws_qrows_thr(_p(Q), _p(K), _p(V), _p(O), B, S, S if Sq is None else Sq, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias),
                                           _p(ws), 0 if ws is None else ws.numel() * 4, float(rescale_thr), _stream())
        if ws is not None and st != 0 and not torch.cuda.is_current_stream_capturing():
            ws.zero_()
        _check(st, "ldc_attn_fwd_ws_qrows_thr")
        return
    if not use_workspace:
        if Sq is None:
            _check(lib.ldc_attn_fwd(_p(Q), _p(K), _p(V), _p(O), B, S, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), _stream()), "ldc_attn_fwd")
        else:
            _check(lib.ldc_attn_fwd_qrows(_p(Q), _p(K), _p(V), _p(O), B, S, Sq, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), _stream()), "ldc_attn_fwd_qrows")
        return
    ws = _attn_f32_workspace(Q.device)
    if Sq is None:
        st = lib.ldc_attn_fwd_ws(_p(Q), _p(K), _p(V), _p(O), B, S, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), _p(ws), ws.numel() * 4, _stream())
    else:
        st = lib.ldc_attn_fwd_ws_qrows(_p(Q), _p(K), _p(V), _p(O), B, S, Sq, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), _p(ws), ws.numel() * 4, _stream())
    if st != 0 and not torch.cuda.is_current_stream_capturing():
        ws.zero_()  # a launch that did not complete may leave ticket counters non-zero: re-arm them before anyone launches again
    _check(st, "ldc_attn_fwd_ws" if Sq is None else "ldc_attn_fwd_ws_qrows")


def rearm_attention_workspaces(device=None):
    """Zero the ticket counters + slabs of the balanced exact-fp32 attention for every stream of `device` (all devices when None).  The launches
    leave their counters zero, so this is needed only after a faulted / aborted launch, and is what the models call before they (re)capture a
    hipGraph.  Must not be called while a graph that uses the workspace is running.  One workspace serves ONE stream: a graph captured on
    stream A and replayed on stream B shares A's counters - replay it on A, or give B its own capture."""
    want = None if device is None else torch.device(device).index
    for key, ws in _workspaces.items():
        if key[0] == "attn_fwd" and (want is None or ws.device.index == want):
            ws.zero_()


def ensemble_scores(forecast, truth, clim, lat_weight, out, *, M, C, H, W, member_stride, channel_stride, truth_channel_stride,
                    clim_channel_stride=0, nan_channel=-1, skill_map=None, spread_map=None):
    """out: [5][C] = acc, mse, crps_spread, crps_skill, crps (ladcast_hip.h: ldc_ensemble_scores)"""
    _dev(forecast, truth, clim, lat_weight, out, skill_map, spread_map)
    ws = _workspace("ensemble_scores", forecast.device, int(lib.ldc_ensemble_scores_workspace_bytes(C, H, W)), grow=True)
    _check(lib.ldc_ensemble_scores(_p(forecast), member_stride, channel_stride, _p(truth), truth_channel_stride, _p(clim),
                                   clim_channel_stride, _p(lat_weight), M, C, H, W, nan_channel, _p(out), _p(skill_map), _p(spread_map),
                                   _p(ws), ws.numel() * 4, _stream()), "ldc_ensemble_scores")


def _forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std):
    """the leading arguments of ldc_rollout_scores / _reliability / _spectrum / _products / _events / _regional / _energy and ldc_validation_scores"""
    return _p(forecast), member_stride, lead_stride, channel_stride, _p(mean), _p(std), float(target_std)


def _truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot):
    """the truth table that follows them in every one of these but ldc_rollout_products"""
    return _p(truth), truth_slot_stride, truth_channel_stride, _p(truth_slot)


def rollout_scores(forecast, truth, truth_slot, clim, clim_slot, lat_weight, out, *, M, C, L, H, W, member_stride, lead_stride, channel_stride,
                   truth_slot_stride, truth_channel_stride, clim_slot_stride=0, clim_channel_stride=0, mean=None, std=None, target_std=1.0,
                   nan_channel=-1, L_total, l_off=0):
    """out [5][C][L_total], columns l_off .. l_off + L - 1 = acc, mse, crps_spread, crps_skill, crps of L lead times in one launch
    (ladcast_hip.h: ldc_rollout_scores); truth_slot / clim_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, clim, clim_slot, lat_weight, out, mean, std)
    ws = _workspace("rollout_scores", forecast.device, int(lib.ldc_rollout_scores_workspace_bytes(C, L, H, W)), grow=True)
    _check(lib.ldc_rollout_scores(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                  *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(clim), clim_slot_stride,
                                  clim_channel_stride, _p(clim_slot), _p(lat_weight), M, C, L, H, W, nan_channel, _p(out), L_total, l_off, _p(ws),
                                  ws.numel() * 4, _stream()), "ldc_rollout_scores")


def validation_scores(forecast, truth, truth_slot, lat_weight, out, *, M, C, L, H, W, member_stride, lead_stride, channel_stride,
                      truth_slot_stride, truth_channel_stride, mean=None, std=None, target_std=1.0, L_total, l_off=0):
    """out [3][C][L_total], columns l_off .. l_off + L - 1 = ens_mse, single_mse, crps of L lead times in one launch
    (ladcast_hip.h: ldc_validation_scores); truth_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, lat_weight, out, mean, std)
    ws = _workspace("validation_scores", forecast.device, int(lib.ldc_validation_scores_workspace_bytes(C, L, H, W)), grow=True)
    _check(lib.ldc_validation_scores(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                     *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(lat_weight), M, C, L, H, W,
                                     _p(out), L_total, l_off, _p(ws), ws.numel() * 4, _stream()), "ldc_validation_scores")


def rollout_reliability(forecast, truth, truth_slot, lat_weight, out, hist_count, hist_weight, n_invalid, *, M, C, L, H, W, member_stride,
                        lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, mean=None, std=None, target_std=1.0,
                        nan_channel=-1, L_total, l_off=0):
    """out [3][C][L_total] = ens_mse, ens_var, ssr; hist_count (int32) / hist_weight [C][L_total][M + 1]; n_invalid (int32) [C][L_total]:
    columns l_off .. l_off + L - 1 of L lead times in one launch (ladcast_hip.h: ldc_rollout_reliability); truth_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, lat_weight, out, hist_count, hist_weight, n_invalid, mean, std)
    nbytes = int(lib.ldc_rollout_reliability_workspace_bytes(M, C, L, H, W))
    ws = _workspace("rollout_reliability", forecast.device, max(nbytes, 4), grow=True)
    _check(lib.ldc_rollout_reliability(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                       *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(lat_weight), M, C, L, H, W,
                                       nan_channel, _p(out), _p(hist_count), _p(hist_weight), _p(n_invalid), L_total, l_off, _p(ws),
                                       ws.numel() * 4, _stream()), "ldc_rollout_reliability")


def rollout_spectrum(forecast, truth, truth_slot, row_weight, out, n_invalid, *, M, C, L, H, W, member_stride, lead_stride, channel_stride,
                     truth_slot_stride, truth_channel_stride, mean=None, std=None, target_std=1.0, L_total, l_off=0):
    """out [3][C][L_total][W / 2 + 1] = spec_members, spec_mean, spec_truth; n_invalid (int32) [C][L_total]: columns l_off .. l_off + L - 1
    of L lead times in one launch (ladcast_hip.h: ldc_rollout_spectrum); truth_slot: device int32 [L]; row_weight: device fp32 [H], >= 0"""
    _dev(forecast, truth, truth_slot, row_weight, out, n_invalid, mean, std)
    nbytes = int(lib.ldc_rollout_spectrum_workspace_bytes(M, C, L, H, W))
    ws = _workspace("rollout_spectrum", forecast.device, max(nbytes, 4), grow=True)
    _check(lib.ldc_rollout_spectrum(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                    *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(row_weight), M, C, L, H, W,
                                    _p(out), _p(n_invalid), L_total, l_off, _p(ws), ws.numel() * 4, _stream()), "ldc_rollout_spectrum")


def products_desc(quantiles, M, threshold_dirs=()):
    """ldc_products_desc for quantiles q in [0, 1] of M members and one direction (+1: above, -1: below) per threshold.  In float64:
    pos = q (M - 1), lo = min(floor(pos), M - 1), t = float32(pos - lo) - numpy's method="linear".  Host arithmetic only."""
    import math

    qs, dirs = [float(q) for q in quantiles], [int(d) for d in threshold_dirs]
    if len(qs) > PRODUCTS_MAX_QUANTILES or len(dirs) > PRODUCTS_MAX_THRESHOLDS:
        raise ValueError(f"at most {PRODUCTS_MAX_QUANTILES} quantiles and {PRODUCTS_MAX_THRESHOLDS} thresholds per call")
    if any(not 0.0 <= q <= 1.0 for q in qs):  # NaN fails the comparison too
        raise ValueError(f"quantiles must lie in [0, 1], got {qs}")
    if any(d not in (1, -1) for d in dirs):
        raise ValueError(f"a threshold direction is +1 (above) or -1 (below), got {dirs}")
    if M < 1:
        raise ValueError("at least one member")
    d = ProductsDesc()
    d.n_quant, d.n_thr = len(qs), len(dirs)
    for k, q in enumerate(qs):
        pos = q * (M - 1)
        lo = min(int(math.floor(pos)), M - 1)
        d.q_lo[k], d.q_t[k] = lo, pos - lo  # the field rounds to fp32
    for k, v in enumerate(dirs):
        d.thr_dir[k] = v
    return d


def rollout_products(forecast, desc, *, M, C, L, H, W, member_stride, lead_stride, channel_stride, channels=None, Cs=None, thr=None, stats=None,
                     quant=None, exceed=None, mean=None, std=None, target_std=1.0, L_total, l_off=0):
    """stats [4][Cs][L_total][H][W] = mean, std, min, max; quant [Q][Cs][L_total][H][W]; exceed [P][Cs][L_total][H][W]: columns
    l_off .. l_off + L - 1 of L lead times in one launch, each output optional (ladcast_hip.h: ldc_rollout_products); desc:
    `products_desc`; channels: device int32 [Cs] or None (all); thr: device fp32 [P][Cs]"""
    _dev(forecast, channels, thr, stats, quant, exceed, mean, std)
    _check(lib.ldc_rollout_products(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                    _p(channels), M, C, C if Cs is None else Cs, L, H, W, ctypes.byref(desc), _p(thr), _p(stats), _p(quant),
                                    _p(exceed), L_total, l_off, _stream()), "ldc_rollout_products")


def events_desc(events):
    """ldc_events_desc for a sequence of (channel, dir, thr, anomaly): dir +1 (value > thr) or -1 (value < thr), thr in physical units,
    anomaly 1 (the value is x - climatology) or 0.  Host only; the channel range is checked by the caller, who knows C."""
    ev = [(int(c), int(d), float(t), int(a)) for c, d, t, a in events]
    if not 1 <= len(ev) <= EVENTS_MAX:
        raise ValueError(f"{len(ev)} events: ldc_rollout_events takes 1 .. {EVENTS_MAX} per call")
    if any(d not in (1, -1) for _, d, _, _ in ev):
        raise ValueError(f"an event's direction is +1 (above) or -1 (below), got {[d for _, d, _, _ in ev]}")
    if any(a not in (0, 1) for _, _, _, a in ev):
        raise ValueError("an event's anomaly flag is 0 or 1")
    if any(t != t for _, _, t, _ in ev):
        raise ValueError("an event's threshold must not be NaN")
    d = EventsDesc()
    d.n_events = len(ev)
    for k, (c, dr, t, a) in enumerate(ev):
        d.channel[k], d.dir[k], d.thr[k], d.anomaly[k] = c, dr, t, a  # the threshold rounds to fp32
    return d


def rollout_events(forecast, truth, truth_slot, clim, clim_slot, lat_weight, desc, hist_count, hist_weight, n_invalid, *, M, C, L, H, W,
                   member_stride, lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, clim_slot_stride=0,
                   clim_channel_stride=0, mean=None, std=None, target_std=1.0, L_total, l_off=0):
    """hist_count (int32) / hist_weight [E][L_total][M + 1][2]; n_invalid (int32) [E][L_total]: columns l_off .. l_off + L - 1 of L lead
    times in one launch (ladcast_hip.h: ldc_rollout_events); desc: `events_desc`; truth_slot / clim_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, clim, clim_slot, lat_weight, hist_count, hist_weight, n_invalid, mean, std)
    nbytes = int(lib.ldc_rollout_events_workspace_bytes(M, desc.n_events, L, H, W))
    ws = _workspace("rollout_events", forecast.device, max(nbytes, 4), grow=True)
    _check(lib.ldc_rollout_events(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                  *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(clim), clim_slot_stride,
                                  clim_channel_stride, _p(clim_slot), _p(lat_weight), M, C, L, H, W, ctypes.byref(desc), _p(hist_count),
                                  _p(hist_weight), _p(n_invalid), L_total, l_off, _p(ws), ws.numel() * 4, _stream()), "ldc_rollout_events")


def rollout_fss_workspace_bytes(M, E, S, L, H, W):
    """bytes of device scratch ldc_rollout_fss needs for M members, E events, S radii, L lead times on an H x W grid; 0 for sizes the call
    refuses"""
    return int(lib.ldc_rollout_fss_workspace_bytes(M, E, S, L, H, W))


def rollout_fss(forecast, truth, truth_slot, clim, clim_slot, lat_weight, desc, radii, fss_sums, n_invalid, *, M, C, L, H, W, member_stride,
                lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, clim_slot_stride=0, clim_channel_stride=0, mean=None,
                std=None, target_std=1.0, L_total, l_off=0):
    """fss_sums (fp64) [E][S][L_total][6]; n_invalid (int32) [E][L_total]: columns l_off .. l_off + L - 1 of L lead times in one call
    (ladcast_hip.h: ldc_rollout_fss); desc: `events_desc`; radii: S host integers (grid points); truth_slot / clim_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, clim, clim_slot, lat_weight, fss_sums, n_invalid, mean, std)
    rs = [int(r) for r in radii]
    if not 1 <= len(rs) <= FSS_SCALES_MAX:
        raise ValueError(f"{len(rs)} radii: ldc_rollout_fss takes 1 .. {FSS_SCALES_MAX} per call")
    nbytes = rollout_fss_workspace_bytes(M, desc.n_events, len(rs), L, H, W)
    ws = _workspace("rollout_fss", forecast.device, max(nbytes, 8), grow=True)
    _check(lib.ldc_rollout_fss(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                               *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(clim), clim_slot_stride,
                               clim_channel_stride, _p(clim_slot), _p(lat_weight), M, C, L, H, W, ctypes.byref(desc), (c_int * len(rs))(*rs),
                               len(rs), _p(fss_sums), _p(n_invalid), L_total, l_off, _p(ws), ws.numel() * 4, _stream()), "ldc_rollout_fss")


REGIONS_MAX, REGIONAL_MAX_MEMBERS, REGIONAL_SUMS, REGIONAL_COUNTS = 32, 64, 10, 3  # the limits and the record of ldc_rollout_regional


def rollout_regional(forecast, truth, truth_slot, clim, clim_slot, lat_weight, region_mask, sums, counts, *, R, M, C, L, H, W, member_stride,
                     lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, clim_slot_stride=0, clim_channel_stride=0,
                     mean=None, std=None, target_std=1.0, L_total, l_off=0):
    """sums (fp64) [R][C][L_total][10]; counts (int32) [R][C][L_total][3]: columns l_off .. l_off + L - 1 of L lead times in one launch
    (ladcast_hip.h: ldc_rollout_regional); region_mask: device int32 / uint32 words [H * W], bit r = region r; truth_slot / clim_slot:
    device int32 [L]"""
    _dev(forecast, truth, truth_slot, clim, clim_slot, lat_weight, region_mask, sums, counts, mean, std)
    nbytes = int(lib.ldc_rollout_regional_workspace_bytes(M, R, C, L, H, W))
    ws = _workspace("rollout_regional", forecast.device, max(nbytes, 4), grow=True)
    _check(lib.ldc_rollout_regional(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                    *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(clim), clim_slot_stride,
                                    clim_channel_stride, _p(clim_slot), _p(lat_weight), _p(region_mask), R, M, C, L, H, W, _p(sums), _p(counts),
                                    L_total, l_off, _p(ws), ws.numel() * 4, _stream()), "ldc_rollout_regional")


SCORE_MAPS_TERMS, SCORE_MAPS_COUNTS, SCORE_MAPS_MAX_MEMBERS = 8, 3, 64  # LDC_SCORE_MAPS_* (ladcast_hip_ext.h) and the largest ensemble


def score_maps_bytes(Cm, P, H, W):
    """bytes of the two accumulators of ldc_rollout_score_maps together (76 per channel, plane and point); 0 for sizes the call refuses"""
    return int(lib.ldc_score_maps_bytes(Cm, P, H, W))


def rollout_score_maps(forecast, truth, truth_slot, clim, clim_slot, channel_idx, plane_of_lead, sums, counts, *, Cm, P, M, C, L, H, W,
                       member_stride, lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, clim_slot_stride=0,
                       clim_channel_stride=0, mean=None, std=None, target_std=1.0):
    """sums (fp64) [Cm][P][8][H * W] and counts (int32) [Cm][P][3][H * W] += the L lead times of this call, lead l into plane
    plane_of_lead[l] (-1: skipped), for the channels channel_idx (ladcast_hip_ext.h: ldc_rollout_score_maps); channel_idx [Cm],
    plane_of_lead / truth_slot / clim_slot [L]: device int32, their values checked by the caller"""
    _dev(forecast, truth, truth_slot, clim, clim_slot, channel_idx, plane_of_lead, sums, counts, mean, std)
    _check(lib.ldc_rollout_score_maps(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                      *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(clim), clim_slot_stride,
                                      clim_channel_stride, _p(clim_slot), _p(channel_idx), Cm, _p(plane_of_lead), P, M, C, L, H, W, _p(sums),
                                      _p(counts), _stream()), "ldc_rollout_score_maps")


ENERGY_MAX_MEMBERS, ENERGY_MAX_GROUPS, ENERGY_PLANES = 256, 32, 5  # the limits of ldc_rollout_energy and the planes of its score buffers


def rollout_energy(forecast, truth, truth_slot, lat_weight, energy, n_invalid, *, M, C, L, H, W, member_stride, lead_stride, channel_stride,
                   truth_slot_stride, truth_channel_stride, group_mask=None, inv_scale2=None, G=0, energy_group=None, dist2=None, mean=None,
                   std=None, target_std=1.0, L_total, l_off=0):
    """energy (fp64) [5][C][L_total] = es, es_fair, skill, spread, Wv; energy_group (fp64) [5][G][L_total] (None iff G == 0); n_invalid
    (int32) [C][L_total]; dist2 (fp64) [C][L_total][M + 1][M + 1] or None: columns l_off .. l_off + L - 1 of L lead times in one call
    (ladcast_hip.h: ldc_rollout_energy); group_mask: device int32 / uint32 words [C], bit g = group g; inv_scale2: device fp64 [C];
    truth_slot: device int32 [L]"""
    _dev(forecast, truth, truth_slot, lat_weight, group_mask, inv_scale2, energy, energy_group, n_invalid, dist2, mean, std)
    nbytes = int(lib.ldc_rollout_energy_workspace_bytes(M, C, G, L, H, W))
    ws = _workspace("rollout_energy", forecast.device, max(nbytes, 8), grow=True)
    _check(lib.ldc_rollout_energy(*_forecast_args(forecast, member_stride, lead_stride, channel_stride, mean, std, target_std),
                                  *_truth_args(truth, truth_slot_stride, truth_channel_stride, truth_slot), _p(lat_weight), _p(group_mask),
                                  _p(inv_scale2), G, M, C, L, H, W, _p(energy), _p(energy_group), _p(n_invalid), _p(dist2), L_total, l_off,
                                  _p(ws), ws.numel() * 4, _stream()), "ldc_rollout_energy")


def recon_preprocess(x, mean, std, out, nan_mask=None, *, B, C, H, W, batch_stride, channel_stride, row_stride, sst_channel=-1):
    """out (B, C, H, W) = (x - mean_c) / std_c of the strided raw frames x; channel `sst_channel`: NaN -> -2 and nan_mask (B, H, W)
    uint8 records where (ladcast_hip.h: ldc_recon_preprocess)"""
    _dev(x, mean, std, out, nan_mask)
    _check(lib.ldc_recon_preprocess(_p(x), batch_stride, channel_stride, row_stride, B, C, H, W, _p(mean), _p(std), sst_channel, _p(out),
                                    _p(nan_mask), _stream()), "ldc_recon_preprocess")


def recon_scores(pred, target, static, nan_mask, lat_weight, mean, std, rel, lw_mse, *, B, C, S, H, W, static_batch_stride=0, sst_channel=-1,
                 abs_norm=None):
    """rel / abs_norm [B][C + S], lw_mse [C + S] of a reconstruction against target + static channels (ladcast_hip.h: ldc_recon_scores)"""
    _dev(pred, target, static, nan_mask, lat_weight, mean, std, rel, lw_mse, abs_norm)
    ws = _workspace("recon_scores", pred.device, int(lib.ldc_recon_scores_workspace_bytes(B, C + S, H, W)), grow=True)
    _check(lib.ldc_recon_scores(_p(pred), _p(target), _p(static), static_batch_stride, _p(nan_mask), _p(lat_weight), _p(mean), _p(std), B, C, S,
                                H, W, sst_channel, _p(rel), _p(abs_norm), _p(lw_mse), _p(ws), ws.numel() * 4, _stream()), "ldc_recon_scores")


def field_moments(x, state, *, B, C, H, W, batch_stride, channel_stride, row_stride, accumulate):
    """state [C][3] fp64 = (n, mean, M2) of the non-NaN values of the strided fp32 batch x, overwritten or merged into
    (ladcast_hip.h: ldc_field_moments)"""
    _dev(x, state)
    nbytes = int(lib.ldc_field_moments_workspace_bytes(B, C, H, W))
    ws = _workspace("field_moments", x.device, max(nbytes, 16), grow=True)
    _check(lib.ldc_field_moments(_p(x), batch_stride, channel_stride, row_stride, B, C, H, W, _p(state), 1 if accumulate else 0, _p(ws),
                                 ws.numel() * 4, _stream()), "ldc_field_moments")


def climatology_accumulate(x, slots, sum, count, *, B, C, H, W, n_slots, batch_stride, channel_stride, row_stride):
    """sum (fp64) / count (int32) [n_slots][C][H][W] += the non-NaN values of frame b of the strided fp32 batch x at slot slots[b]
    (device int32 [B]; outside [0, n_slots): skipped), in frame order (ladcast_hip.h: ldc_climatology_accumulate)"""
    _dev(x, slots, sum, count)
    _check(lib.ldc_climatology_accumulate(_p(x), batch_stride, channel_stride, row_stride, B, C, H, W, _p(slots), n_slots, _p(sum), _p(count),
                                          _stream()), "ldc_climatology_accumulate")


def climatology_smooth(sum, count, weights, out, n_empty=None, *, n_days, n_hours, C, plane):
    """out (fp32) [n_days][n_hours][C * plane] = the weighted mean over the circular day window (weights: device fp64 [window]) of the
    accumulated state; n_empty (int64 [C], zeroed by the caller) += the outputs without a sample (ladcast_hip.h: ldc_climatology_smooth)"""
    _dev(sum, count, weights, out, n_empty)
    _check(lib.ldc_climatology_smooth(_p(sum), _p(count), _p(weights), int(weights.numel()), n_days, n_hours, C, plane, _p(out), _p(n_empty),
                                      _stream()), "ldc_climatology_smooth")


def paired_bootstrap_workspace_bytes(N, K, R, D):
    return int(lib.ldc_paired_bootstrap_workspace_bytes(N, K, R, D))


def paired_bootstrap(a, b, draws, stats, counts, *, N, K, ld, R, D, kind, tail_ppm):
    """stats (fp64 [K][8]) / counts (int32 [K][4]) of the paired bootstrap of the score arrays a, b (fp32, element (i, k) at i * ld + k) over
    the replicates draws (device int32 [R][D], every value in [0, N): checked by the caller) (ladcast_hip.h: ldc_paired_bootstrap)"""
    _dev(a, b, draws, stats, counts)
    nbytes = paired_bootstrap_workspace_bytes(N, K, R, D)
    ws = _workspace("paired_bootstrap", a.device, max(nbytes, 16), grow=True)
    _check(lib.ldc_paired_bootstrap(_p(a), _p(b), ld, N, K, _p(draws), R, D, kind, tail_ppm, _p(stats), _p(counts), _p(ws), ws.numel() * 4,
                                    _stream()), "ldc_paired_bootstrap")


def compact_rope_table(cos, sin):
    """the reference's [rows][128] cos / sin tables (every value twice: get_1d_rotary_pos_embed's repeat_interleave(2)) -> the
    [rows][64][2] (cos_i, sin_i) table of `qkv_epilogue`; refuses tables that are not of that form"""
    if not (torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])):
        raise ValueError("rotary tables must hold every (cos, sin) value twice (adjacent-pair RoPE)")
    return torch.stack([cos[:, 0::2], sin[:, 0::2]], dim=-1).reshape(cos.shape[0], cos.shape[1]).contiguous()


def qkv_epilogue(wq=None, wk=None, rope=None, *, eps=1e-7, heads, rope_row0=0, qscale=0.0):
    """epilogue of one QKV-projection problem of `gemm_grouped_qkv` (ldc_qkv_epilogue); rope = `compact_rope_table(cos, sin)`;
    returns (struct, keep-alive tuple)"""
    _dev(wq, wk, rope)
    pv = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return QkvEpilogue(pv(wq), pv(wk), pv(rope), None, eps, qscale, heads, rope_row0), (wq, wk, rope)


_DEFAULT_QSCALE = ctypes.c_float(0.08838834764831845 * 1.4426950408889634).value  # log2(e) / sqrt(128) as the library rounds it


def gemm_grouped_qkv_f32(problems, epilogues):
    """exact-fp32 `gemm_grouped` where problem i with a non-None epilogue is a QKV projection whose epilogue applies the per-head RMSNorm
    and the rotary embedding (ldc_gemm_grouped_qkv_f32; epilogues built with qscale=1).  Returns False - and launches nothing - when the
    ring kernel does not serve the launch (LDC_ERR_UNSUPPORTED): the caller then runs `gemm_grouped` + `qk_rmsnorm_rope`."""
    n = len(problems)
    if not 1 <= n <= MAX_GROUPED or len(epilogues) != n:
        raise ValueError(f"gemm_grouped_qkv_f32 takes 1..{MAX_GROUPED} problems and one epilogue (or None) per problem")
    arr = (GemmProblem * n)(*[p[0] for p in problems])
    epi = (QkvEpilogue * n)(*[(e[0] if e is not None else QkvEpilogue()) for e in epilogues])
    ws = _grouped_workspace(problems[0][1][2].device)
    st = lib.ldc_gemm_grouped_qkv_f32(arr, epi, n, c_void_p(ws.data_ptr()), ws.numel() * 4, _stream())
    if st == ERR_UNSUPPORTED:
        return False
    _check(st, "ldc_gemm_grouped_qkv_f32")
    return True


def gemm_grouped_qkv(problems, epilogues, force_fallback=False):
    """`gemm_grouped(split_bf16=True)` where problem i with a non-None epilogue is a fused QKV projection whose C receives the
    attention operand rows of `attn_fwd_split` (bias -> per-head RMSNorm -> rotary embedding -> q scale -> hi / lo split).
    When the fused kernel does not serve the launch (LDC_ERR_UNSUPPORTED: K not a whole k-step, more tiles than hand-off counters)
    this runs what include/ladcast_hip.h documents for that status - the plain grouped GEMM, then `ldc_attn_qkv_prepare_split` in
    place on every QKV problem's output (split-bf16 mode only; `force_fallback` takes that route unconditionally, for tests)."""
    n = len(problems)
    if not 1 <= n <= MAX_GROUPED or len(epilogues) != n:
        raise ValueError(f"gemm_grouped_qkv takes 1..{MAX_GROUPED} problems and one epilogue (or None) per problem")
    arr = (GemmProblem * n)(*[p[0] for p in problems])
    epi = (QkvEpilogue * n)(*[(e[0] if e is not None else QkvEpilogue()) for e in epilogues])
    ws = _grouped_workspace(problems[0][1][2].device)
    st = ERR_UNSUPPORTED if force_fallback else lib.ldc_gemm_grouped_bf16x3_qkv(arr, epi, n, c_void_p(ws.data_ptr()), ws.numel() * 4, _stream())
    if st != ERR_UNSUPPORTED:
        _check(st, "ldc_gemm_grouped_bf16x3_qkv")
        return
    if any(p[0].d.flags & GEMM_BF16_1TERM for p in problems):
        raise RuntimeError("ldc_gemm_grouped_bf16x3_qkv: shape not served by the fused kernel, and the plain-GEMM + ldc_attn_qkv_prepare_split "
                           "route only writes split-bf16 operand rows (status -3 in the single-term bf16 mode)")
    _check(lib.ldc_gemm_grouped_bf16x3(arr, n, c_void_p(ws.data_ptr()), ws.numel() * 4, _stream()), "ldc_gemm_grouped_bf16x3 (QKV fallback)")
    for (p, keep), e in zip(problems, epilogues):
        if e is None:
            continue
        q, (wq, wk, rope) = e
        if q.qscale not in (0.0, _DEFAULT_QSCALE):  # ldc_attn_qkv_prepare_split applies the default scale only: never two answers for one call
            raise RuntimeError("ldc_gemm_grouped_bf16x3_qkv: shape not served by the fused kernel, and the plain-GEMM + ldc_attn_qkv_prepare_split "
                               f"route applies the default q scale log2(e)/sqrt(128), not qscale={q.qscale!r}")
        d, C = p.d, keep[2]
        D, S = q.heads * 128, d.M
        if d.N != 3 * D:
            raise RuntimeError("ldc_gemm_grouped_bf16x3_qkv failed with status -1")  # what the fused launch reports for a wrong width
        cos = sin = None
        if rope is not None:  # the compact (cos_i, sin_i) table back in the [rows][128] form of ldc_attn_qkv_prepare_split
            t = rope.reshape(-1, 64, 2)[q.rope_row0 : q.rope_row0 + S]
            cos, sin = t[..., 0].repeat_interleave(2, dim=1).contiguous(), t[..., 1].repeat_interleave(2, dim=1).contiguous()
        base = C.data_ptr()
        _check(lib.ldc_attn_qkv_prepare_split(c_void_p(base), c_void_p(base + 4 * D), c_void_p(base + 8 * D), d.batch, S, q.heads, d.ldc, d.c_bs, S,
                                              _p(wq), _p(wk), _p(cos), _p(sin), None, None, None, None, q.eps, _stream()), "ldc_attn_qkv_prepare_split")


def attn_qkv_prepare_split(Q, K, V, *, B, S, H, ld_qkv, qkv_bs, split_row, seg0=(None, None, None, None), seg1=(None, None, None, None), eps=1e-7):
    """fp32 q / k / v views of a fused buffer -> the operand rows of `attn_fwd_split`, in place (segN = (wq, wk, cos, sin))"""
    _dev(Q, K, V, *seg0, *seg1)
    _check(lib.ldc_attn_qkv_prepare_split(_p(Q), _p(K), _p(V), B, S, H, ld_qkv, qkv_bs, split_row, _p(seg0[0]), _p(seg0[1]), _p(seg0[2]), _p(seg0[3]),
                                          _p(seg1[0]), _p(seg1[1]), _p(seg1[2]), _p(seg1[3]), eps, _stream()), "ldc_attn_qkv_prepare_split")


def _attn_workspace(device, nbytes):
    """scratch of the attention's TAIL schedule (more units than CUs), allocated at the largest size any call shape can ask for
    (ldc_attn_fwd_split_workspace_max_bytes, 17.8 MB): a regrown workspace would leave the older graphs writing their partials into
    freed memory"""
    ws = _workspace("attn_fwd_split", device, lib.ldc_attn_fwd_split_workspace_max_bytes())
    if ws.numel() * 4 < nbytes:
        raise RuntimeError(f"attn_fwd_split: call shape asks for {nbytes} workspace bytes, more than ldc_attn_fwd_split_workspace_max_bytes")
    return ws


def attn_fwd_split(Q, K, V, O, *, B, S, H, ld_qkv, qkv_bs, ldo, o_bs, out_split=False, one_term=False, key_bias=None, use_workspace=True, Sq=None):
    """attention on row-major split-bf16 operand rows (ldc_attn_fwd_split); key_bias: additive score bias per key, padded to a multiple
    of 32 entries (`pad_key_bias`), or None.  use_workspace=False: never the TAIL schedule (A/B, tests).  Sq: the queries are the first
    Sq token rows only (keys / values: all S; rows >= Sq of O untouched; ldc_attn_fwd_split_qrows)"""
    _dev(Q, K, V, O, key_bias)
    if Sq is None:
        nbytes = lib.ldc_attn_fwd_split_workspace_bytes(B, S, H) if use_workspace else 0
    else:
        nbytes = lib.ldc_attn_fwd_split_qrows_workspace_bytes(B, S, Sq, H) if use_workspace else 0
    ws = _attn_workspace(Q.device, nbytes) if nbytes > 0 else None
    if key_bias is not None and key_bias.numel() < 32 * ((S + 31) // 32):
        raise ValueError("key_bias must be padded to a multiple of 32 keys (hip.pad_key_bias)")
    flags = (ATTN_OUT_BF16 if int(out_split) == FMT_BF16 else ATTN_OUT_SPLIT if out_split else 0) | (ATTN_BF16_1TERM if one_term else 0)
    if Sq is None:
        _check(lib.ldc_attn_fwd_split(_p(Q), _p(K), _p(V), _p(O), B, S, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), flags, _p(ws), 0 if ws is None else ws.numel() * 4,
                                      _stream()), "ldc_attn_fwd_split")
    else:
        _check(lib.ldc_attn_fwd_split_qrows(_p(Q), _p(K), _p(V), _p(O), B, S, Sq, H, ld_qkv, qkv_bs, ldo, o_bs, _p(key_bias), flags, _p(ws),
                                            0 if ws is None else ws.numel() * 4, _stream()), "ldc_attn_fwd_split_qrows")


def pad_key_bias(bias):
    """[S] -> [32 * ceil(S / 32)] (zero-padded, contiguous): the form `attn_fwd_split` reads 16 bytes at a time"""
    S = bias.numel()
    out = torch.zeros(32 * ((S + 31) // 32), device=bias.device, dtype=torch.float32)
    out[:S] = bias.reshape(-1)
    return out


def qk_rmsnorm_rope(q, k, *, B, row0, rows, H, ld, bs, wq, wk, eps, cos=None, sin=None):
    _dev(q, k, wq, wk, cos, sin)
    _check(lib.ldc_qk_rmsnorm_rope(_p(q), _p(k), B, row0, rows, H, ld, bs, _p(wq), _p(wk), eps, _p(cos), _p(sin), _stream()),
           "ldc_qk_rmsnorm_rope")


def layernorm_mod(x, y, *, B, rows, D, ldx, x_bs, ldy, y_bs, scale=None, shift=None, mod_bs=0, mode=0, eps=1e-6, out_split=False,
                  split_row=None, scale2=None, shift2=None):
    """split_row: rows [split_row, rows) take scale2 / shift2 (two token streams normalised by one launch)"""
    _dev(x, y, scale, shift, scale2, shift2)
    if split_row is None:
        _check(lib.ldc_layernorm_mod(_p(x), _p(y), B, rows, D, ldx, x_bs, ldy, y_bs, _p(scale), _p(shift), mod_bs, mode, eps,
                                     int(out_split), _stream()),
               "ldc_layernorm_mod")
    else:
        _check(lib.ldc_layernorm_mod2(_p(x), _p(y), B, rows, D, ldx, x_bs, ldy, y_bs, _p(scale), _p(shift), split_row, _p(scale2), _p(shift2),
                                      mod_bs, mode, eps, int(out_split), _stream()),
               "ldc_layernorm_mod2")


def mean_rows(x, y, *, B, rows, D, ldx, x_bs, x_split=None, lds=None, s_bs=None, fmt=FMT_SPLIT):
    """x_split: also write x in the split (fmt FMT_SPLIT) or plain-bf16 (FMT_BF16) activation format to this buffer (row stride lds,
    batch stride s_bs, in floats)"""
    _dev(x, y, x_split)
    if x_split is None:
        _check(lib.ldc_mean_rows(_p(x), _p(y), B, rows, D, ldx, x_bs, _stream()), "ldc_mean_rows")
    else:
        _check(lib.ldc_mean_rows_split(_p(x), _p(y), _p(x_split), B, rows, D, ldx, x_bs, lds if lds is not None else ldx,
                                       s_bs if s_bs is not None else x_bs, int(fmt), _stream()), "ldc_mean_rows_split")


def gate_residual(resid, y, gate, out, *, B, rows, D, ld_res, res_bs, ld_y, y_bs, gate_bs):
    _dev(resid, y, gate, out)
    _check(lib.ldc_gate_residual(_p(resid), _p(y), _p(gate), _p(out), B, rows, D, ld_res, res_bs, ld_y, y_bs, gate_bs, _stream()),
           "ldc_gate_residual")


def chan_to_token(x, out, *, B, C, N, ldo, fill_cols=None, out_split=False):
    _dev(x, out)
    _check(lib.ldc_chan_to_token_split(_p(x), _p(out), B, C, N, ldo, ldo if fill_cols is None else fill_cols, int(out_split), _stream()),
           "ldc_chan_to_token")


def token_to_chan(x, out, *, B, C, N, ldi):
    _dev(x, out)
    _check(lib.ldc_token_to_chan(_p(x), _p(out), B, C, N, ldi, _stream()), "ldc_token_to_chan")


def timestep_embedding(t, out, n):
    _dev(t, out)
    _check(lib.ldc_timestep_embedding(_p(t), _p(out), n, _stream()), "ldc_timestep_embedding")


def temb_modulate(temb, te, *, B, D, te_rows):
    _dev(temb, te)
    _check(lib.ldc_temb_modulate(_p(temb), _p(te), B, D, te_rows, _stream()), "ldc_temb_modulate")


def chan_affine(x, y, mean, std, target_std, *, outer, C, inner, inverse):
    _dev(x, y, mean, std)
    _check(lib.ldc_chan_affine(_p(x), _p(y), _p(mean), _p(std), target_std, outer, C, inner, int(inverse), _stream()), "ldc_chan_affine")


TRACK_MAX_CHANNELS, TRACK_MAX_BOXES, TRACK_MAX_INNER, TRACK_MAX_GRID = 8, 8, 30, 1024  # LDC_TRACK_MAX_* of ladcast_hip.h


def _int_array(values):
    return (c_int * len(values))(*[int(v) for v in values])


def track_gather(x, out, channels, mean, std, *, sb, st, sc, B, T, HW, T_total, t_off, target_std=1.0):
    """out (B, T_total, len(channels), HW)[:, t_off:t_off + T] = inverse-normalised channels of x (ldc_track_gather)"""
    _dev(x, out, mean, std)
    _check(lib.ldc_track_gather(_p(x), sb, st, sc, B, T, HW, _int_array(channels), len(channels), _p(mean), _p(std), float(target_std),
                                _p(out), T_total, t_off, _stream()), "ldc_track_gather")


def derive_desc(fields):
    """the ldc_derive_desc array for a sequence of (kind, channels): kind one of DERIVE_*, as many channels as `DERIVE_INPUTS` states.
    Host only; the channel range is checked by the caller, who knows C."""
    fs = [(int(k), [int(c) for c in ch]) for k, ch in fields]
    if not 1 <= len(fs) <= DERIVE_MAX_FIELDS:
        raise ValueError(f"{len(fs)} derived fields: ldc_derive_fields takes 1 .. {DERIVE_MAX_FIELDS} per call")
    arr = (DeriveDesc * len(fs))()
    for d, (kind, ch) in zip(arr, fs):
        if kind not in DERIVE_INPUTS or len(ch) != DERIVE_INPUTS[kind]:
            raise ValueError(f"derived field (kind {kind}, channels {ch}): kind {DERIVE_SPEED} / {DERIVE_DIFF} reads 2 channels, {DERIVE_SHEAR} reads 4")
        d.kind = kind
        for j, c in enumerate(ch):
            d.ch[j] = c
    return arr


def derive_fields(src, out, desc, *, outer_stride, lead_stride, channel_stride, n_outer, L, C, HW, out_outer_stride, out_lead_stride,
                  out_channel_stride, slot=None, mean=None, std=None, target_std=1.0):
    """out[o][l][k] = field k of `desc` (`derive_desc`) computed from the inverse-normalised channels of src (ladcast_hip.h:
    ldc_derive_fields); slot: device int32 [L] or None; the three out strides place the planes"""
    _dev(src, out, slot, mean, std)
    _check(lib.ldc_derive_fields(_p(src), outer_stride, lead_stride, channel_stride, _p(slot), _p(mean), _p(std), float(target_std), n_outer, L, C,
                                 HW, desc, len(desc), _p(out), out_outer_stride, out_lead_stride, out_channel_stride, _stream()), "ldc_derive_fields")


def sphere_desc(fields):
    """the ldc_sphere_desc array for a sequence of (kind, (u, v)): kind SPHERE_VORTICITY or SPHERE_DIVERGENCE, the two wind channels.
    Host only; the channel range is checked by the caller, who knows C."""
    fs = [(int(k), [int(c) for c in ch]) for k, ch in fields]
    if not 1 <= len(fs) <= DERIVE_MAX_FIELDS:
        raise ValueError(f"{len(fs)} derived fields: ldc_derive_sphere takes 1 .. {DERIVE_MAX_FIELDS} per call")
    arr = (SphereDesc * len(fs))()
    for d, (kind, ch) in zip(arr, fs):
        if kind not in (SPHERE_VORTICITY, SPHERE_DIVERGENCE) or len(ch) != 2:
            raise ValueError(f"derived field (kind {kind}, channels {ch}): kind {SPHERE_VORTICITY} / {SPHERE_DIVERGENCE} reads the 2 channels u, v")
        d.kind = kind
        d.ch[0], d.ch[1] = ch
    return arr


def derive_sphere(src, out, desc, row_tables, k, *, outer_stride, lead_stride, channel_stride, n_outer, L, C, H, W, out_outer_stride,
                  out_lead_stride, out_channel_stride, slot=None, mean=None, std=None, target_std=1.0):
    """out[o][l][f] = field f of `desc` (`sphere_desc`): the vorticity or divergence of the inverse-normalised wind channels of src
    (ladcast_hip.h: ldc_derive_sphere); row_tables: device fp64 (4, H) = c, q, r, pc and k, as `evaluate.derived.sphere_row_tables` makes
    them; slot: device int32 [L] or None; the three out strides place the planes"""
    _dev(src, out, row_tables, slot, mean, std)
    if row_tables.dtype != torch.float64 or tuple(row_tables.shape) != (4, H) or not row_tables.is_contiguous():
        raise ValueError(f"row_tables must be a contiguous fp64 (4, H) = (4, {H}) tensor")
    _check(lib.ldc_derive_sphere(_p(src), outer_stride, lead_stride, channel_stride, _p(slot), _p(mean), _p(std), float(target_std), n_outer, L, C,
                                 H, W, _p(row_tables), float(k), desc, len(desc), _p(out), out_outer_stride, out_lead_stride, out_channel_stride,
                                 _stream()), "ldc_derive_sphere")


def track_nanmean(x, out, *, member_stride, E, n):
    _dev(x, out)
    _check(lib.ldc_track_nanmean(_p(x), member_stride, E, n, _p(out), _stream()), "ldc_track_nanmean")


def track_storms(fields, lat, lon, lat0, lon0, out_lat, out_lon, out_code, *, track_stride, frame_stride, mslp_off, z_off, lsm, H, W,
                 n_tracks, n_steps, inner_box_sizes, enforce_msl):
    _dev(fields, lat, lon, lat0, lon0, out_lat, out_lon, out_code, lsm)
    _check(lib.ldc_track_storms(_p(fields), track_stride, frame_stride, mslp_off, z_off, _p(lsm), _p(lat), H, _p(lon), W, _p(lat0), _p(lon0),
                                n_tracks, n_steps, _int_array(inner_box_sizes), len(inner_box_sizes), int(bool(enforce_msl)), _p(out_lat),
                                _p(out_lon), _p(out_code), _stream()), "ldc_track_storms")


def track_local_min(fields, field_idx, lat, lon, lat0, lon0, inner, found, out_lat, out_lon, out_val, *, field_stride, H, W, n_queries):
    _dev(fields, field_idx, lat, lon, lat0, lon0, inner, found, out_lat, out_lon, out_val)
    _check(lib.ldc_track_local_min(_p(fields), field_stride, _p(field_idx), _p(lat), H, _p(lon), W, _p(lat0), _p(lon0), _p(inner), n_queries,
                                   _p(found), _p(out_lat), _p(out_lon), _p(out_val), _stream()), "ldc_track_local_min")


def edm_scale_f64_to_f32(x, c_in, out):
    _dev(x, out)
    _check(lib.ldc_edm_scale_f64_to_f32(_p(x), c_in, _p(out), x.numel(), _stream()), "ldc_edm_scale_f64_to_f32")


def edm_init_state(noise, sigma0, x):
    _dev(noise, x)
    _check(lib.ldc_edm_init_state(_p(noise), sigma0, _p(x), x.numel(), _stream()), "ldc_edm_init_state")


def edm_churn(x_cur, noise, coef, x_hat):
    """x_hat = x_cur + coef * noise (fp64; the stochastic branch of the EDM sampler)"""
    _dev(x_cur, noise, x_hat)
    if noise.dtype != torch.float64 or x_cur.dtype != torch.float64:
        raise TypeError("edm_churn works on the fp64 sampler state")
    _check(lib.ldc_edm_churn(_p(x_cur), _p(noise), coef, _p(x_hat), x_cur.numel(), _stream()), "ldc_edm_churn")


def edm_euler(x_hat, F, c_skip, c_out, t_hat, dt, x_next, d_cur):
    _dev(x_hat, F, x_next, d_cur)
    _check(lib.ldc_edm_euler(_p(x_hat), _p(F), c_skip, c_out, t_hat, dt, _p(x_next), _p(d_cur), x_hat.numel(), _stream()), "ldc_edm_euler")


def edm_heun(x_hat, x_next, F, d_cur, c_skip, c_out, t_next, dt):
    _dev(x_hat, x_next, F, d_cur)
    _check(lib.ldc_edm_heun(_p(x_hat), _p(x_next), _p(F), _p(d_cur), c_skip, c_out, t_next, dt, x_hat.numel(), _stream()), "ldc_edm_heun")


def f64_to_f32(x, y):
    _dev(x, y)
    _check(lib.ldc_f64_to_f32(_p(x), _p(y), x.numel(), _stream()), "ldc_f64_to_f32")


def dpm_step(sample, F, m1, x0, prev, c_skip, c_out, a, b, inv_r0, order):
    _dev(sample, F, m1, x0, prev)
    _check(lib.ldc_dpm_step(_p(sample), _p(F), _p(m1), _p(x0), _p(prev), c_skip, c_out, a, b, inv_r0, order, sample.numel(), _stream()),
           "ldc_dpm_step")


def ddim_step(sample, F, noise, x0, prev, sqrt_alpha_t, sqrt_beta_t, sqrt_alpha_prev, dir_coef, std_dev, clip_range, prediction_type, reclip):
    _dev(sample, F, noise, x0, prev)
    _check(lib.ldc_ddim_step(_p(sample), _p(F), _p(noise), _p(x0), _p(prev), sqrt_alpha_t, sqrt_beta_t, sqrt_alpha_prev, dir_coef, std_dev,
                             clip_range, prediction_type, int(bool(reclip)), sample.numel(), _stream()), "ldc_ddim_step")


def ddpm_step(sample, F, noise, x0, prev, sqrt_alpha_t, sqrt_beta_t, x0_coef, sample_coef, std_dev, clip_range, prediction_type):
    _dev(sample, F, noise, x0, prev)
    _check(lib.ldc_ddpm_step(_p(sample), _p(F), _p(noise), _p(x0), _p(prev), sqrt_alpha_t, sqrt_beta_t, x0_coef, sample_coef, std_dev, clip_range,
                             prediction_type, sample.numel(), _stream()), "ldc_ddpm_step")


def scale_f32(x, s, y):
    _dev(x, y)
    _check(lib.ldc_scale_f32(_p(x), s, _p(y), x.numel(), _stream()), "ldc_scale_f32")


def axpby_f32(x, a, y, b, out):
    _dev(x, y, out)
    _check(lib.ldc_axpby_f32(_p(x), a, _p(y), b, _p(out), x.numel(), _stream()), "ldc_axpby_f32")


# -- EDM denoising objective, one noise level per sample (ladcast_hip.h: ldc_edm_noise_inputs / _denoise / _denoise_loss) -------------
def _f32c(what, *ts):
    for t in ts:
        if t is not None and not (t.dtype == torch.float32 and t.is_contiguous()):
            raise TypeError(f"{what}: contiguous fp32 tensors only")


def _per_sample(what, B, *vs):
    for v in vs:
        if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == B):
            raise ValueError(f"{what}: per-sample coefficients are contiguous fp32 device vectors with one entry per sample ({B})")


def edm_noise_inputs(clean, noise, sigma, c_in, noisy, x_in):
    """noisy = clean + noise * sigma_b, x_in = noisy * c_in_b in one launch; noise None: noisy = clean; noisy or x_in None: not written"""
    _dev(clean, noise, sigma, c_in, noisy, x_in)
    _f32c("edm_noise_inputs", clean, noise, noisy, x_in)
    B = clean.shape[0]
    _per_sample("edm_noise_inputs", B, sigma, c_in)
    for t in (noise, noisy, x_in):
        if t is not None and t.shape != clean.shape:
            raise ValueError("edm_noise_inputs: all tensors have the shape of `clean`")
    _check(lib.ldc_edm_noise_inputs(_p(clean), _p(noise), _p(sigma), _p(c_in), _p(noisy), _p(x_in), B, clean.numel() // max(B, 1), _stream()),
           "ldc_edm_noise_inputs")


def _t_slice_frames(what, t, shape):
    """frames of the contiguous (B, C, frames, H, W) tensor that `t` (shape (B, C, T, H, W)) is a T-slice of"""
    B, C, T, H, W = shape
    if tuple(t.shape) != tuple(shape) or t.dtype != torch.float32:
        raise ValueError(f"{what}: fp32 tensors of one shape (B, C, T, H, W)")
    plane = H * W
    sb, sc, st, sh, sw = t.stride()
    ok = (sw == 1 or W == 1) and (sh == W or H == 1) and (st == plane or T == 1)
    frames = sc // plane if C > 1 else (sb // (C * plane) if B > 1 else T)
    ok = ok and frames >= T and (C == 1 or sc == frames * plane) and (B == 1 or sb == C * frames * plane)
    if not ok:
        raise ValueError(f"{what}: tensors must be contiguous or slices along T of contiguous tensors (strides {t.stride()})")
    return frames


def edm_denoise(noisy, F, c_skip, c_out, denoised):
    """denoised = c_skip_b * noisy + c_out_b * F; the three (B, C, T, H, W) tensors may be slices along T of contiguous tensors"""
    _dev(noisy, F, c_skip, c_out, denoised)
    B, C, T, H, W = noisy.shape
    _per_sample("edm_denoise", B, c_skip, c_out)
    fr = [_t_slice_frames("edm_denoise", t, noisy.shape) for t in (noisy, F, denoised)]
    _check(lib.ldc_edm_denoise(_p(noisy), _p(F), _p(c_skip), _p(c_out), _p(denoised), B, C, T, H * W, fr[0], fr[1], fr[2], _stream()),
           "ldc_edm_denoise")


def edm_denoise_loss(noisy, F, target, c_skip, c_out, weight, table, lat_weight=None, denoised=None):
    """table (B, C, T) = plane means of w * ((c_skip_b * noisy + c_out_b * F) - target)^2, w = weight_b or lat_weight[h] * weight_b
    (ladcast_hip.h: ldc_edm_denoise_loss); denoised: also write the preconditioned output"""
    _dev(noisy, F, target, c_skip, c_out, weight, table, lat_weight, denoised)
    _f32c("edm_denoise_loss", noisy, F, target, table, lat_weight, denoised)
    B, C, T, H, W = noisy.shape
    _per_sample("edm_denoise_loss", B, c_skip, c_out, weight)
    for t in (F, target, denoised):
        if t is not None and t.shape != noisy.shape:
            raise ValueError("edm_denoise_loss: noisy, F, target and denoised have one shape (B, C, T, H, W)")
    if table.numel() != B * C * T or (lat_weight is not None and lat_weight.numel() != H):
        raise ValueError("edm_denoise_loss: table holds B * C * T values, lat_weight H")
    _check(lib.ldc_edm_denoise_loss(_p(noisy), _p(F), _p(target), _p(c_skip), _p(c_out), _p(weight), _p(lat_weight), _p(table), _p(denoised),
                                    B, C, T, H, W, _stream()), "ldc_edm_denoise_loss")


# -- DCAE (NHWC) -------------------------------------------------------------------------------
def sphere_conv_nhwc(X, Wt, Y, *, B, H, W, cin, cout, ldx=None, ldy=None, bias=None, R=None, ldr=0, ksize=3, act=ACT_NONE):
    _dev(X, Wt, Y, bias, R)
    _check(lib.ldc_sphere_conv_nhwc(_p(X), _p(Wt), _p(bias), _p(R), _p(Y), B, H, W, cin, ldx if ldx is not None else cin, cout,
                                    ldy if ldy is not None else cout, ldr, ksize, act, _stream()), "ldc_sphere_conv_nhwc")


def conv_cin_padded(cin, cpk=32):
    """channels per tap of a packed conv weight: cpk * 2^j >= cin (cpk = channels per k-step: 32 split-bf16, 64 plain bf16)"""
    kt = -(-cin // cpk)
    p2 = 1
    while p2 < kt:
        p2 *= 2
    return cpk * p2


def sphere_conv_nhwc_split(X, Wp, Y, *, B, H, W, cin, cout, ldx, ldy=None, bias=None, R=None, ldr=0, ksize=3, act=ACT_NONE, in_fmt=FMT_SPLIT,
                           out_fmt=FMT_F32):
    """X: operand rows (FMT_SPLIT: Wp = pack_weight_bf16x2 of the [cout, k*k*conv_cin_padded(cin)] tap-major weight, zeros behind cin | FMT_BF16: Wp = pack_weight_bf16 of the taps padded to 64 * 2^j channels;
    ldx % 8 == 0); Y fp32 rows or (out_fmt = in_fmt) operand rows"""
    _dev(X, Wp, Y, bias, R)
    ws = _grouped_workspace(X.device)
    _check(lib.ldc_sphere_conv_nhwc_split(_p(X), _p(Wp), _p(bias), _p(R), _p(Y), B, H, W, cin, ldx, cout, ldy if ldy is not None else cout,
                                          ldr, ksize, act, int(in_fmt), int(out_fmt), _p(ws), ws.numel() * 4, _stream()), "ldc_sphere_conv_nhwc_split")


def sphere_conv_plan(B, H, W, cin, cout, ksize=3, in_fmt=FMT_SPLIT):
    """(halo, tile_rows, tile_w): which kernel `sphere_conv_nhwc_split` runs for the shape (ldc_sphere_conv_plan)"""
    bm, tw = c_int(0), c_int(0)
    halo = lib.ldc_sphere_conv_plan(B, H, W, cin, cout, ksize, int(in_fmt), ctypes.byref(bm), ctypes.byref(tw))
    return bool(halo), bm.value, tw.value


def split_rows(x, ys, *, rows, C, ldx=None, lds=None, fmt=FMT_SPLIT):
    _dev(x, ys)
    _check(lib.ldc_split_rows(_p(x), _p(ys), rows, C, ldx if ldx is not None else C, lds if lds is not None else -(-C // 8) * 8, int(fmt), _stream()),
           "ldc_split_rows")


def sphere_dwconv_nhwc(x, wt, y, *, B, H, W, C, ldx=None, ldy=None, bias=None, ksize=3, glu=False, out_fmt=FMT_F32):
    _dev(x, wt, y, bias)
    cy = C // 2 if glu else C
    _check(lib.ldc_sphere_dwconv_nhwc_fmt(_p(x), _p(wt), _p(bias), _p(y), B, H, W, C, ldx if ldx is not None else C,
                                          ldy if ldy is not None else cy, ksize, int(glu), int(out_fmt), _stream()), "ldc_sphere_dwconv_nhwc_fmt")


def grouped_conv1x1_nhwc(x, wt, y, *, M, groups, ldx, ldy):
    _dev(x, wt, y)
    _check(lib.ldc_grouped_conv1x1_nhwc(_p(x), _p(wt), _p(y), M, groups, ldx, ldy, _stream()), "ldc_grouped_conv1x1_nhwc")


def relu_linear_attn_nhwc(qkv, y, *, B, P, groups, ldq, ldy, eps, out_fmt=FMT_F32, sliced=True):
    """ReLU linear attention over consecutive 96-channel (q | k | v) groups.  sliced (default): 128-pixel slices, partial KV matrices
    in a scratch buffer of ldc_relu_linear_attn_workspace_bytes, two launches; sliced=False: one workgroup per (frame, group)"""
    _dev(qkv, y)
    ws, nbytes = None, 0
    if sliced:
        nbytes = lib.ldc_relu_linear_attn_workspace_bytes(B, P, groups)  # 0 below 1024 pixels: one launch there
        ws = torch.empty(nbytes // 4, device=qkv.device, dtype=torch.float32) if nbytes else None
    _check(lib.ldc_relu_linear_attn_nhwc_fmt(_p(qkv), _p(y), B, P, groups, ldq, ldy, eps, int(out_fmt), _p(ws), nbytes,
                                             _stream()),
           "ldc_relu_linear_attn_nhwc_fmt")


def rmsnorm_rows(x, w, y, *, rows, C, eps, b=None, resid=None, ldx=None, ldr=None, ldy=None, act=ACT_NONE, ys=None, lds=None, fmt=FMT_SPLIT):
    """y: fp32 rows and / or ys: operand rows (fmt = FMT_SPLIT | FMT_BF16, lds = C rounded up to 8 by default)"""
    _dev(x, w, b, resid, y, ys)
    _check(lib.ldc_rmsnorm_rows_split(_p(x), _p(w), _p(b), _p(resid), _p(y), _p(ys), rows, C, ldx if ldx is not None else C,
                                      ldr if ldr is not None else C, ldy if ldy is not None else C,
                                      (lds if lds is not None else -(-C // 8) * 8) if ys is not None else 0, int(fmt), eps, act, _stream()),
           "ldc_rmsnorm_rows_split")


def pixel_unshuffle_shortcut(cv, x, y, *, B, H2, W2, cout, cin, ys=None, lds=None, fmt=FMT_SPLIT):
    _dev(cv, x, y, ys)
    _check(lib.ldc_pixel_unshuffle_shortcut_split(_p(cv), _p(x), _p(y), _p(ys), B, H2, W2, cout, cin,
                                                  (lds if lds is not None else -(-cout // 8) * 8) if ys is not None else 0, int(fmt), _stream()),
           "ldc_pixel_unshuffle_shortcut_split")


def pixel_shuffle_to_chan(cv, out, *, B, H, W, cout, keep):
    """cv [B*H*W, 4*cout] NHWC conv rows -> out [B, keep, 2H, 2W] NCHW: pixel_shuffle without shortcut, first `keep` channels (ldc_pixel_shuffle_to_chan)"""
    _dev(cv, out)
    _check(lib.ldc_pixel_shuffle_to_chan(_p(cv), _p(out), B, H, W, cout, keep, _stream()), "ldc_pixel_shuffle_to_chan")


def pixel_shuffle_shortcut(cv, x, y, *, B, H, W, cout, cin, ys=None, lds=None, fmt=FMT_SPLIT):
    _dev(cv, x, y, ys)
    _check(lib.ldc_pixel_shuffle_shortcut_split(_p(cv), _p(x), _p(y), _p(ys), B, H, W, cout, cin,
                                                (lds if lds is not None else -(-cout // 8) * 8) if ys is not None else 0, int(fmt), _stream()),
           "ldc_pixel_shuffle_shortcut_split")


def upsample_nearest2x_rows(x, y, *, B, H, W, C, ldx=None, ldy=None, ys=None, lds=None, fmt=FMT_SPLIT):
    """NHWC rows [B*H*W, ldx] -> [B*2H*2W, C] nearest-neighbour x2 (F.interpolate(scale_factor=2, mode="nearest")): fp32 rows `y` and / or operand rows `ys`"""
    _dev(x, y, ys)
    _check(lib.ldc_upsample_nearest2x_rows(_p(x), _p(y), _p(ys), B, H, W, C, ldx if ldx is not None else C, ldy if ldy is not None else C,
                                           (lds if lds is not None else (ys.shape[1] if ys is not None else 0)), int(fmt), _stream()), "ldc_upsample_nearest2x_rows")


def chan_regroup(x, y, *, M, cin, cout):
    _dev(x, y)
    _check(lib.ldc_chan_regroup(_p(x), _p(y), M, cin, cout, _stream()), "ldc_chan_regroup")
