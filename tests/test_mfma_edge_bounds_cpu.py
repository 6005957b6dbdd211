"""The bounds of tests/mfma_edge_refs.py judged without a GPU: the kernels' arithmetic restated in fp32 torch (chunked accumulation in
k-step order, pieces summed in order, online softmax over key tiles with the mode's P quantisation, the conv as a gathered GEMM) passes
every bound at every case shape tests/test_gpu_mfma_edges.py runs, and each planted defect breaks its bound in at least one element -
which is what shows that the GPU test would notice the same defect in a kernel.  For the tile-per-workgroup kernel of gemm_f32.hip:
its 175 GEMM shapes and seven conv cases, the defects that kernel can have (ragged last k-tile dropped, a stale LDS stage, a row from its
neighbour, no pole roll, no pole flip, one image base per tile), and the float64 gather-GEMM that defines its conv at H = 2 held to the
oracle conv at every H >= 3 case."""
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


# ---- the tile-per-workgroup kernel of gemm_f32.hip: ldc_gemm_bias_act and ldc_sphere_conv_nhwc -------------------------------------
@pytest.mark.parametrize("K", R.TILE_GEMM_K)
def test_tile_gemm_emulation_passes_the_bound_at_every_case_shape(K):
    """no cuts: the kernel sums a tile in one piece (the bound still counts the 9 pieces of the ring kernel: it only grows)"""
    worst, n = 0.0, 0
    for M, N, K_, batch, epi in R.tile_gemm_shapes(K):
        kw = R.gemm_inputs(M, N, K_, batch, epi, "f32")
        want, bound = R.gemm_case_ref(M, N, K_, batch, epi, "f32")
        r = ratio(R.gemm_f32(**kw), want, bound)
        assert r <= 1.0, (M, N, K_, batch, epi, r)
        worst, n = max(worst, r), n + 1
    assert n == len(R.GEMM_M) * len(R.TILE_GEMM_N)
    print(f"tile gemm K {K}: worst err / bound of the fp32 restatement {worst:.3f}")


def test_tile_gemm_case_table():
    cases = list(R.tile_gemm_shapes())
    assert len(cases) == 175 and sum(len(list(R.tile_gemm_shapes(K))) for K in R.TILE_GEMM_K) == 175
    assert {(b, e) for _, _, _, b, e in cases} == {(b, e) for b in (1, 3) for e in range(len(R.EPILOGUES))}  # batch x epilogue: every pair
    for K in R.TILE_GEMM_K:  # at every depth: both batch sizes, every epilogue
        assert {b for _, _, _, b, _ in R.tile_gemm_shapes(K)} == {1, 3}
        assert {e for _, _, _, _, e in R.tile_gemm_shapes(K)} == set(range(len(R.EPILOGUES)))


def _tile_gemm_mutant(K, **defect):
    """worst ratio of the mutant over the cases of depth K with at least two rows; the unmutated restatement passes each of them"""
    out = []
    for M, N, K_, batch, epi in R.tile_gemm_shapes(K):
        if M == 1 or R.EPILOGUES[epi][3] == 3:  # (one row has no neighbour; ReLU may hide a defect behind its zero)
            continue
        kw = R.gemm_inputs(M, N, K_, batch, epi, "f32")
        want, bound = R.gemm_case_ref(M, N, K_, batch, epi, "f32")
        out.append(ratio(R.gemm_f32(**kw, **defect), want, bound))
    return out


@pytest.mark.parametrize("K", (36, 84))
def test_tile_gemm_ragged_last_kstep_dropped_breaks_the_bound(K):
    """the ragged k-tile (4 resp. 20 of 32 columns) of tile (0, 0) skipped: at EVERY case of that depth"""
    assert min(_tile_gemm_mutant(K, drop_kstep=(0, 0, K // 32))) > 1.0


def test_tile_gemm_stale_lds_stage_breaks_the_bound():
    """K = 96: the third k-step reads stage 0 before it was refilled, i.e. multiplies the first k-step's operands again"""
    assert min(_tile_gemm_mutant(96, stale_stage=True)) > 1.0
    assert max(_tile_gemm_mutant(64, stale_stage=True)) <= 1.0  # two k-steps: no stage is reused, the defect cannot show


@pytest.mark.parametrize("K", R.TILE_GEMM_K)
def test_tile_gemm_row_from_its_neighbour_breaks_the_bound(K):
    assert min(_tile_gemm_mutant(K, last_row_from_prev=True)) > 1.0


TILE_CONV_ALL = R.TILE_CONV_CASES + [R.MODULE_CONV_CASE]


@pytest.mark.parametrize("case", TILE_CONV_ALL, ids=str)
def test_tile_conv_emulation_passes_the_bound(case):
    kw = R.conv_inputs(*case)
    ks = case[5]
    for act in (0, 1):
        want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32", act=act, R=kw["R"])
        assert ratio(R.conv_f32(kw["x"], kw["w"], kw["bias"], ks, "f32", act=act, R=kw["R"]), want, bound) <= 1.0


# float64 sums of K terms differ by at most 2 K 2**-53 S between two orders of summation; the bound is more than K 2**-24 S: the two
# float64 references agree to 2**-28 of the bound (the activation passes both through the same function)
F64_AGREEMENT = 2.0 ** -28


@pytest.mark.parametrize("case", TILE_CONV_ALL + R.CONV_CASES[1:2], ids=str)
def test_gather_gemm_equals_the_oracle_conv_wherever_the_oracle_is_defined(case):
    """what lets conv_ref(via_gather=True) serve as the reference at H = 2: at every H >= 3 case it gives the oracle's value (and bound)"""
    kw = R.conv_inputs(*case)
    ks = case[5]
    assert case[1] >= 3
    for act in (0, 1):
        want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32", act=act, R=kw["R"])
        got, gbound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32", act=act, R=kw["R"], via_gather=True)
        assert ratio(got, want, bound) <= F64_AGREEMENT
        assert ratio(gbound, bound, bound) <= F64_AGREEMENT


def test_the_oracle_conv_is_undefined_at_two_rows_and_the_gather_is_not():
    case = R.TILE_CONV_H2_CASE
    kw = R.conv_inputs(*case)
    with pytest.raises(Exception):
        R.conv_ref(kw["x"], kw["w"], kw["bias"], 3, "f32")
    for act in (0, 1):
        want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], 3, "f32", act=act, via_gather=True)
        assert torch.isfinite(want).all() and (bound > 0).all()
        assert ratio(R.conv_f32(kw["x"], kw["w"], kw["bias"], 3, "f32", act=act), want, bound) <= 1.0
    # both rows are pole rows: row 0 reads row 0 mirrored (ky = 0) and row 1, row 1 reads row 0 and row 1 mirrored (ky = 2), both rolled and flipped
    g = R.sphere_gather(torch.arange(2 * 4, dtype=torch.float32).reshape(1, 2, 4, 1), 3)[0, :, :, :, 0]
    assert g[0, 0].tolist() == [3.0, 2.0, 1.0, 3.0, 0.0, 1.0, 7.0, 4.0, 5.0]
    assert g[1, 0].tolist() == [3.0, 0.0, 1.0, 7.0, 4.0, 5.0, 7.0, 6.0, 5.0]


def _conv_mutant(case, **defect):
    kw = R.conv_inputs(*case)
    ks = case[5]
    want, bound = R.conv_ref(kw["x"], kw["w"], kw["bias"], ks, "f32", R=kw["R"])
    assert ratio(R.conv_f32(kw["x"], kw["w"], kw["bias"], ks, "f32", R=kw["R"]), want, bound) <= 1.0
    return R.conv_f32(kw["x"], kw["w"], kw["bias"], ks, "f32", R=kw["R"], **defect), want, bound


POLE_CASES = [R.TILE_CONV_CASES[0], R.TILE_CONV_CASES[2]]  # ks = 3 at H = 4, ks = 5 at H = 3


@pytest.mark.parametrize("case", POLE_CASES, ids=str)
@pytest.mark.parametrize("defect", ["no_pole_roll", "no_pole_flip"])
def test_tile_conv_pole_defects_break_the_bound(case, defect):
    H, ks = case[1], case[5]
    assert ks == (3, 5)[POLE_CASES.index(case)]
    got, want, bound = _conv_mutant(case, **{defect: True})
    assert ratio(got, want, bound) > 1.0
    p = ks // 2
    if defect == "no_pole_flip":  # only rows 0 and H - 1 flip
        assert ratio(got[:, 1:-1], want[:, 1:-1], bound[:, 1:-1]) <= 1.0
        for h in (0, H - 1):
            assert ratio(got[:, h], want[:, h], bound[:, h]) > 1.0
    elif H > 2 * p:  # rows that reach over no pole are untouched (none at H = 3, ks = 5)
        assert ratio(got[:, p:H - p], want[:, p:H - p], bound[:, p:H - p]) <= 1.0


@pytest.mark.parametrize("case", R.TILE_CONV_STRADDLING, ids=str)
def test_tile_conv_image_base_of_the_tiles_first_row_breaks_the_bound(case):
    B, H, W = case[:3]
    got, want, bound = _conv_mutant(case, tile_first_image=True)
    flat = lambda t: t.reshape(B * H * W, -1)  # noqa: E731
    pix = torch.arange(B * H * W)
    wrong = pix // (H * W) != pix // 128 * 128 // (H * W)  # pixels whose tile began in an earlier image
    assert 0 < int(wrong.sum()) < B * H * W
    assert ratio(flat(got)[wrong], flat(want)[wrong], flat(bound)[wrong]) > 1.0
    assert ratio(flat(got)[~wrong], flat(want)[~wrong], flat(bound)[~wrong]) <= 1.0
