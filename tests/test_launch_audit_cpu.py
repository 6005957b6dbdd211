"""The launch-audit classifier (tests/launch_audit.py) on kernel names as the profiler reports them: template arguments decide, a
name outside the table is an error."""
import pytest

from tests.launch_audit import classify, violations

RING_F32 = "void (anonymous namespace)::gemm_bf16x3_v3_kernel<128, 0, false>(SKArgs)"
RING_F32_CONV = "void (anonymous namespace)::gemm_bf16x3_v3_kernel<128, 0, true>(SKArgs)"
RING_SPLIT = "void (anonymous namespace)::gemm_bf16x3_v3_kernel<128, 3, false>(SKArgs)"
RING_ONE = "void (anonymous namespace)::gemm_bf16x3_v3_kernel<256, 1, true>(SKArgs)"
ATTN_SPLIT = "void (anonymous namespace)::attn_fwd_split_kernel<2, 3, false, true>(AttnArgs)"
ATTN_ONE = "void (anonymous namespace)::attn_fwd_split_kernel<2, 1, true, false>(AttnArgs)"
HALO = "void (anonymous namespace)::conv_halo_kernel<256, 3>(HaloArgs)"
FP32_OK = [RING_F32, RING_F32_CONV, "void (anonymous namespace)::attn_fwd_f32_kernel<4, true>(AttnArgs)",
           "void (anonymous namespace)::rmsnorm_rows_kernel<2>(float const*, float const*, float const*, float const*, float*, float*, int, int)",
           "edm_euler_kernel(double const*, float const*, double, double, double, double, double*, double*, long long)",
           "void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>, std::array<char*, 1ul> >(int, at::native::FillFunctor<float>, std::array<char*, 1ul>)",
           "Memcpy HtoD (Host -> Device)"]


def test_fp32_names_pass_and_bf16_mfma_is_flagged():
    assert violations("fp32", FP32_OK) == []
    assert classify(RING_F32).terms == 0 and not classify(RING_F32_CONV).bf16_mfma
    for bad in (RING_SPLIT, RING_ONE, ATTN_SPLIT, ATTN_ONE, HALO, "void (anonymous namespace)::gemm_streamk_bf16x3_kernel(SKArgs)"):
        assert violations("fp32", FP32_OK + [bad]) == [bad], bad


def test_bf16x3_mode_flags_single_term_instances_only():
    ok = [RING_SPLIT, ATTN_SPLIT, HALO, RING_F32] + FP32_OK
    assert violations("bf16x3", ok) == []
    for bad in (RING_ONE, ATTN_ONE, "void (anonymous namespace)::conv_halo_kernel<128, 1>(HaloArgs)"):
        assert violations("bf16x3", ok + [bad]) == [bad], bad
    assert violations("bf16", [RING_ONE, ATTN_ONE]) == []


def test_mangled_names_are_classified():
    k = classify("_ZN12_GLOBAL__N_121gemm_bf16x3_v3_kernelILi128ELi3ELb0EEEv6SKArgs")
    assert (k.family, k.terms, k.bf16_mfma) == ("gemm_bf16x3_v3_kernel", 3, True)


@pytest.mark.parametrize("name", ["void Cijk_Ailk_Bljk_BBS_BH_MT128x128x64(...)", "ldc_test_aggressor_kernel(float*, int)",
                                  "void (anonymous namespace)::gemm_bf16x3_v3_kernel<128, 2, false>(SKArgs)",
                                  "void (anonymous namespace)::gemm_bf16x3_v3_kernel<256, 0, false>(SKArgs)",
                                  "void (anonymous namespace)::gemm_bf16x3_v3_kernel<128, 3>(SKArgs)", "some_new_kernel(int)"])
def test_unknown_names_fail(name):
    with pytest.raises(ValueError):
        classify(name)
    with pytest.raises(ValueError):
        violations("fp32", [RING_F32, name])
