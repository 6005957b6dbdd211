"""Which arithmetic a workload really ran: every kernel name a launch sequence produced, classified by kernel family AND template
arguments (the exact-fp32 GEMM is `gemm_bf16x3_v3_kernel<128, 0, *>` - a bf16 substring says nothing).  A name outside the table is
an error: a new kernel (or a library GEMM) must be classified here before a mode audit can pass.  Used by tests/test_gpu_launch_audit.py;
the classifier itself is checked on the CPU (tests/test_launch_audit_cpu.py)."""
import re
import subprocess
from dataclasses import dataclass


@dataclass(frozen=True)
class Kernel:
    family: str
    args: tuple  # template arguments as written by the demangler ('128', '0', 'true')
    bf16_mfma: bool  # issues a bf16 MFMA (v_mfma_f32_*_bf16)
    terms: int  # bf16 products per fp32 product: 3 split-bf16, 1 single-term bf16, 0 no bf16 MFMA


def _int(a):
    return int(a.strip())


def _bool(a):
    a = a.strip()
    if a in ("true", "(bool)1", "1"):
        return True
    if a in ("false", "(bool)0", "0"):
        return False
    raise ValueError(a)


def _terms_v3(args):  # gemm_bf16x3_v3_kernel<BM, TERMS, CONV>: the ring kernel (TERMS 0: v_mfma_f32_16x16x4_f32 on fp32 rows)
    bm, t, conv = _int(args[0]), _int(args[1]), _bool(args[2])
    if bm not in (128, 256) or t not in (0, 1, 3) or (t == 0 and bm != 128):
        raise ValueError(args)
    del conv
    return t


def _terms_split(args):  # conv_halo_kernel<BM, TERMS>, attn_fwd_split_kernel<NGRP, TERMS, BIAS, TAIL>: bf16 MFMA, 1 or 3 terms
    t = _int(args[1])
    if t not in (1, 3):
        raise ValueError(args)
    for a in args[2:]:
        _bool(a)
    return t


# family -> (number of template arguments, args -> terms (0: no bf16 MFMA))
FAMILIES = {
    "gemm_bf16x3_v3_kernel": (3, _terms_v3),
    "conv_halo_kernel": (2, _terms_split),
    "attn_fwd_split_kernel": (4, _terms_split),
    "gemm_streamk_bf16x3_kernel": (0, lambda a: 3),  # register-staged split-bf16 stream-K (v_mfma_f32_32x32x16_bf16, three terms)
    # fp32 matrix cores (v_mfma_f32_32x32x2_f32 / 16x16x4_f32) or no MFMA at all
    "gemm_streamk_kernel": (0, None),
    "gemm_nt_f32_kernel": (1, None),
    "attn_fwd_f32_kernel": (2, None),
    "linear_rows_mfma_kernel": (2, None),
    "relu_linear_attn_kernel": (0, None),
    "relu_linear_attn_kv_slice_kernel": (0, None),
    "relu_linear_attn_apply_slice_kernel": (0, None),
    "grouped_conv1x1_kernel": (0, None),
    "qkv_prepare_split_kernel": (0, None),
    "attn_tail_merge_kernel": (0, None),
    "sphere_dwconv_kernel": (2, None),
    "sphere_dwconv_row_kernel": (2, None),
    "rmsnorm_rows_kernel": (1, None),
    "split_rows_kernel": (0, None),
    "pixel_unshuffle_shortcut_kernel": (0, None),
    "pixel_shuffle_shortcut_kernel": (0, None),
    "pixel_shuffle_to_chan_kernel": (0, None),
    "upsample_nearest2x_rows_kernel": (0, None),
    "chan_regroup_kernel": (0, None),
    "pack_weight_bf16x2_kernel": (0, None),
    "pack_weight_bf16_kernel": (0, None),
    "chan_to_token_kernel": (0, None),
    "token_to_chan_kernel": (0, None),
    "timestep_embedding_kernel": (0, None),
    "temb_modulate_kernel": (0, None),
    "chan_affine_kernel": (0, None),
    "layernorm_mod_kernel": (0, None),
    "qk_rmsnorm_rope_kernel": (0, None),
    "mean_rows_kernel": (0, None),
    "mean_rows_split_kernel": (0, None),
    "gate_residual_kernel": (0, None),
    "linear_small_kernel": (1, None),
    "linear_small_grouped_kernel": (0, None),
    "edm_scale_kernel": (0, None),
    "edm_init_kernel": (0, None),
    "edm_churn_kernel": (0, None),
    "edm_euler_kernel": (0, None),
    "edm_heun_kernel": (0, None),
    "f64_to_f32_kernel": (0, None),
    "dpm_step_kernel": (0, None),
    "dd_step_kernel": (0, None),
    "scale_f32_kernel": (0, None),
    "axpby_f32_kernel": (0, None),
    "ensemble_scores_kernel": (2, None),
    "ensemble_scores_finish_kernel": (0, None),
}
TORCH = Kernel("torch", (), False, 0)  # PyTorch's own element-wise / copy / fill / index kernels (at::native): no MFMA
COPY = Kernel("copy", (), False, 0)  # runtime memcpy / memset records

_NAME = re.compile(r"(?:^|[\s:])([A-Za-z_]\w*)\s*(?:<(.*)>)?\s*\(")


def demangle(name):
    if not name.startswith("_Z"):
        return name
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, timeout=30, check=True).stdout.strip() or name
    except (OSError, subprocess.SubprocessError):
        return name


def classify(name):
    """Kernel record for one launched kernel name (demangled or mangled); ValueError for a name outside the table"""
    name = demangle(name.strip()).replace("(anonymous namespace)::", "")
    if name.startswith(("Memcpy", "Memset", "hipMemcpy", "hipMemset", "__amd_rocclr_")):
        return COPY
    if "at::native::" in name:
        return TORCH
    head = name.split("(", 1)[0] + "(" if "(" in name else name + "("
    m = _NAME.search(head)
    if m is None or m.group(1) not in FAMILIES:
        raise ValueError(f"kernel not in the launch-audit table: {name!r}")
    fam = m.group(1)
    args = tuple(a.strip() for a in m.group(2).split(",")) if m.group(2) else ()
    nargs, rule = FAMILIES[fam]
    if len(args) != nargs:
        raise ValueError(f"unexpected template arguments for {fam}: {name!r}")
    try:
        terms = rule(args) if rule is not None else 0
    except ValueError:
        raise ValueError(f"unexpected template arguments for {fam}: {name!r}") from None
    return Kernel(fam, args, terms != 0, terms)


def violations(mode, names):
    """the launched names that break the mode's arithmetic: fp32 - anything that issues a bf16 MFMA; bf16x3 - any single-term
    (TERMS == 1) instance.  Raises ValueError for a name outside the table."""
    bad = []
    for n in names:
        k = classify(n)
        if (mode == "fp32" and k.bf16_mfma) or (mode == "bf16x3" and k.terms == 1):
            bad.append(n)
    return bad


def kernels_launched(body):
    """names of the GPU kernels (and copies) that body() launched, recorded by the torch profiler (kineto); synchronises the device"""
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        body()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
