"""Per-mode error bands of the end-to-end GPU tests (test-only: the stated tolerances that bench.py prints live in
ladcast_amd/precision.py and are not these).  The model-level bounds of the suite sit above what the split-bf16 mode reaches, so on
their own they cannot tell the exact-fp32 mode from "split-bf16 somewhere".  Per stage, on the same inputs:
* fp32 ceiling = min(4 x the fp32 rel-L2 measured on this tree, 1/2 x the bf16x3 rel-L2 measured on this tree);
* bf16x3 "really on": err_bf16x3 >= 3 x err_fp32.
MEASURED: (fp32, bf16x3) rel-L2 against the oracle / the reference fixture, the largest over a test's cases, one MI355X run of the suite."""

MEASURED = {  # stage: (fp32, bf16x3) - the test that measures it
    "tiny_forward": (3.70e-7, 5.72e-6),  # test_gpu_model.py::test_tiny_forward_matches_oracle (3 shapes)
    "tiny_chunk_edm": (2.18e-7, 3.39e-6),  # test_gpu_model.py::test_tiny_sampler_chunk_matches_oracle
    "tiny_chunk_pipeline": (8.94e-7, 9.38e-6),
    "forward_375m": (4.19e-7, 5.99e-6),  # test_gpu_model.py::test_full_375m_forward_all_modes_one_and_two_members (3 cases)
    "forward_1p6b": (4.96e-7, 6.19e-6),  # test_gpu_model.py::test_full_1_6b_forward_matches_oracle_both_modes
    "chunk_375m_edm": (1.03e-7, 2.56e-6),  # test_gpu_chain.py::test_full_375m_chunk_matches_oracle
    "chunk_375m_pipeline": (5.26e-7, 4.91e-6),
    "chunk_1p6b_5fwd": (8.04e-7, 7.93e-6),  # test_gpu_chain.py::test_1_6b_heun_step_truncated_chunk
    "chunk_1p6b_truncated": (8.02e-7, 7.93e-6),
    "chain_375m_3chunks": (7.23e-7, 7.7e-6),  # test_gpu_chain.py::test_375m_two_members_three_chained_full_size_chunks (per chunk)
    "literal_chunk_1.6B": (1.13e-7, 2.67e-6),  # test_gpu_chain.py, committed-oracle chunks and chains
    "literal_chunk_375M": (1.03e-7, 2.55e-6),
    "literal_chain_cfg 4 literal (1.6B)": (1.2e-7, 2.66e-6),
    "literal_chain_cfg 3 literal (375M)": (1.15e-7, 2.55e-6),
    "dcae_full_encode": (1.58e-6, 1.18e-5),  # test_gpu_dcae.py::test_full_dcae_single_frame_all_modes
    "dcae_full_decode": (1.25e-6, 8.29e-6),
    "dcae_ray1024_encode": (1.49e-6, 1.06e-5),  # test_gpu_dcae.py::test_dc_ae_ray_1024_shape_one_frame
    "dcae_ray1024_decode": (1.16e-6, 7.32e-6),
    "tiny_dcae_encode": (1.06e-6, 1.57e-5),  # test_gpu_dcae.py::test_tiny_dcae_matches_oracle_and_pin
    "tiny_dcae_decode": (6.58e-7, 9.35e-6),
    "pin_ar_forward": (3.49e-7, 5.72e-6),  # test_gpu_reference_pins.py (reference-code fixtures)
    "pin_nope": (3.48e-7, 5.75e-6),
    "pin_dcae_encode": (1.06e-6, 1.57e-5),
    "pin_dcae_decode": (6.43e-7, 9.60e-6),
    "pin_dcae_layers0_encode": (5.69e-7, 8.21e-6),
    "pin_dcae_layers0_decode": (5.80e-7, 8.98e-6),
    "pin_dcae_temb_encode": (4.27e-7, 7.02e-6),
    "pin_dcae_temb_decode": (5.37e-7, 7.58e-6),
}
RATIO = 3.0


def ceiling(stage):
    f, b = MEASURED[stage]
    return min(4.0 * f, 0.5 * b)


def check_all(stage, pairs):
    """check() for several cases of one stage: every figure is printed before the first assert"""
    for e32, e3 in pairs:
        _show(stage, e32, e3)
    for e32, e3 in pairs:
        check(stage, e32, e3, show=False)


def _show(stage, e_fp32, e_bf16x3):
    have = MEASURED.get(stage)
    print(f"\nband {stage}: fp32 {e_fp32:.3e}" + (f", bf16x3 {e_bf16x3:.3e} (ratio {e_bf16x3 / e_fp32:.1f})" if e_bf16x3 is not None else "")
          + (f", ceiling {ceiling(stage):.2e}" if have else ", NOT IN TABLE"))


def check(stage, e_fp32, e_bf16x3=None, show=True):
    """assert the fp32 ceiling of `stage` and (given the bf16x3 error on the same inputs) the gap between the modes"""
    if show:
        _show(stage, e_fp32, e_bf16x3)
    have = MEASURED.get(stage)
    assert have is not None, f"no measured band for {stage}"
    assert e_fp32 < ceiling(stage), (stage, e_fp32, ceiling(stage))
    if e_bf16x3 is not None:
        assert e_bf16x3 >= RATIO * e_fp32, (stage, e_fp32, e_bf16x3)
