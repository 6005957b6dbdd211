"""The bounds of tests/mfma_edge_refs.py judged without a GPU: the kernels' arithmetic restated in fp32 torch (chunked accumulation in
k-step order, pieces summed in order, online softmax over key tiles with the mode's P quantisation, the conv as a gathered GEMM) passes
every bound at every case shape tests/test_gpu_mfma_edges.py runs, and each planted defect breaks its bound in at least one element -
which is what shows that the GPU test would notice the same defect in a kernel."""
import pytest
import torch

from tests import mfma_edge_refs as R
from tests.redzone import worst_ratio


def ratio(got, want, bound):
    return worst_ratio(got, want, bound.expand_as(want))[0]


# ---- GEMM -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
def test_gemm_emulation_passes_the_bound_at_every_case_shape(mode):
    worst = 0.0
    for M, N, K, batch, epi in R.gemm_shapes(mode, regstage=mode == "f32"):
        kw = R.gemm_inputs(M, N, K, batch, epi, mode)
        want, bound = R.gemm_ref(mode=mode, **kw)
        kt = -(-K // R.KSTEP[mode])
        for cuts in ((), tuple(range(1, kt))[:8]):  # whole tiles, and the deepest cut the bound counts (9 pieces)
            r = ratio(R.gemm_f32(mode=mode, cuts=cuts, **kw), want, bound)
            assert r <= 1.0, (M, N, K, batch, epi, cuts, r)
            worst = max(worst, r)
    print(f"gemm {mode}: worst err / bound of the fp32 restatement {worst:.3f}")


def _sweep_inputs(mode, name):
    out = []
    for i, (M, N, k32, batch) in enumerate(R.SWEEP_PROBLEMS[name]):
        out.append(R.gemm_inputs(M, N, R.sweep_K(mode, k32), batch, i, mode))
    return out


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", list(R.SWEEP_PROBLEMS))
def test_gemm_emulation_passes_at_the_sweep_shapes_for_every_cut(mode, name):
    for kw in _sweep_inputs(mode, name):
        want, bound = R.gemm_ref(mode=mode, **kw)
        kt = kw["A"].shape[-1] // R.KSTEP[mode]
        for pieces in range(1, min(kt, 9) + 1):
            cuts = tuple(round(i * kt / pieces) for i in range(1, pieces))
            assert ratio(R.gemm_f32(mode=mode, cuts=cuts, **kw), want, bound) <= 1.0, (name, pieces)


GEMM_MUTANTS = {
    "one k-step dropped in one tile": dict(drop_kstep=(2, 1, 4)),
    "the last valid row computed from row M - 2": dict(last_row_from_prev=True),
    "a two-piece tile with one piece added twice": dict(cuts=(5,), piece_twice=True),
}


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("mutant", list(GEMM_MUTANTS))
def test_gemm_mutants_break_the_bound(mode, mutant):
    kw = _sweep_inputs(mode, "3x3 tiles, 9 k-steps")[0]
    want, bound = R.gemm_ref(mode=mode, **kw)
    assert ratio(R.gemm_f32(mode=mode, **kw), want, bound) <= 1.0
    assert ratio(R.gemm_f32(mode=mode, **dict(kw, **GEMM_MUTANTS[mutant])), want, bound) > 1.0


def test_gemm_lo_hi_term_dropped_in_one_column_panel_breaks_the_bound():
    kw = _sweep_inputs("bf16x3", "3x3 tiles, 9 k-steps")[0]
    want, bound = R.gemm_ref(mode="bf16x3", **kw)
    got = R.gemm_f32(mode="bf16x3", drop_lohi_panel=1, **kw)
    assert ratio(got, want, bound) > 1.0
    assert ratio(got[..., :128], want[..., :128], bound[..., :128]) <= 1.0  # the other panels are untouched


# ---- attention ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(R.ATTN_MODES))
@pytest.mark.parametrize("S", R.ATTN_S)
def test_attention_emulation_passes_the_bound_at_every_case_shape(mode, S):
    for Sq, H, B, kind in R.attn_combos(S):
        q, k, v = R.attn_inputs(B, S, H)
        bias = R.key_bias(S, kind)
        want, bound = R.attn_ref(q, k, v, bias, Sq, mode)
        r = ratio(R.attn_f32(q, k, v, bias, Sq, mode), want, bound)
        assert r <= 1.0, (S, Sq, H, B, kind, r)


@pytest.mark.parametrize("mode", list(R.ATTN_MODES))
def test_attention_emulation_passes_the_bound_at_the_schedule_case(mode):
    S, Sq, H, B, kind = R.ATTN_SCHEDULE_CASE
    q, k, v = R.attn_inputs(B, S, H)
    bias = R.key_bias(S, kind)
    want, bound = R.attn_ref(q, k, v, bias, Sq, mode)
    assert ratio(R.attn_f32(q, k, v, bias, Sq, mode), want, bound) <= 1.0


@pytest.mark.parametrize("mode", list(R.ATTN_MODES))
def test_attention_mutants_break_the_bound(mode):
    S, H, B = 129, 3, 2
    q, k, v = R.attn_inputs(B, S, H)
    bias = R.key_bias(S, "key in the ragged last tile")
    want, bound = R.attn_ref(q, k, v, bias, S, mode)
    assert ratio(R.attn_f32(q, k, v, bias, S, mode), want, bound) <= 1.0
    assert ratio(R.attn_f32(q, k, v, bias, S, mode, skip_tile=2), want, bound) > 1.0  # one key tile skipped
    assert ratio(R.attn_f32(q, k, v, bias, S, mode, ignore_bias_key=128), want, bound) > 1.0  # one key's bias ignored (the ragged tile's key)


# ---- convs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.CONV_CASES + [R.HALO_CASE], ids=str)
def test_conv_emulation_passes_the_bound(mode, case):
    B, H, W, cin, cout, ks, has_res = case
    kw = R.conv_inputs(*case)
    for act in (1,) if case != R.HALO_CASE else (0,):  # (the activation each GPU case runs)
        want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, mode, act=act, R=kw["R"])
        assert ratio(R.conv_f32(kw["x"], kw["w"], kw["bias"], ks, mode, act=act, R=kw["R"]), want, bound) <= 1.0


@pytest.mark.parametrize("mode", R.MODES)
def test_conv_wrap_around_column_from_the_wrong_side_breaks_the_bound(mode):
    case = R.CONV_CASES[0]
    kw = R.conv_inputs(*case)
    want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], 3, mode)
    got = R.conv_f32(kw["x"], kw["w"], kw["bias"], 3, mode, wrap_wrong_side=True)
    assert ratio(got, want, bound) > 1.0
    assert ratio(got[:, 1:-1, 1:-1], want[:, 1:-1, 1:-1], bound[:, 1:-1, 1:-1]) <= 1.0  # only the frame's first / last row and column see it
