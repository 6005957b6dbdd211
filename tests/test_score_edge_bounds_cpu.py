"""The bounds of tests/score_edge_refs.py judged without a GPU: the scoring kernels' arithmetic restated in fp32 torch (member-order sum,
sorted weighted sum, 256-point workgroups, fixed reduction order; multiply-adds contracted and not) passes every bound at every case
shape tests/test_gpu_score_edges.py runs, so does the reference's own torch arithmetic (oracle/scoring.py, tests/validation_oracle.py in
fp32), and each planted defect breaks a bound or the bit-equality of the integer maps in at least one element - which is what shows that
the GPU test would notice the same defect in a kernel."""
import pytest
import torch

from oracle import scoring as S
from tests import score_edge_refs as R


def judge_all(got, ref, what):
    """maps, scores and validation of `got` against `ref`; -> worst ratio"""
    worst = 0.0
    for group in ("maps", "scores", "validation"):
        for k, r in ref[group].items():
            worst = max(worst, R.judge(got[group][k], r, f"{what} {group} {k}"))
    return worst


def worst_of(got, ref, groups=("maps", "scores", "validation")):
    return max(R.ratio_of(got[g][k], *ref[g][k]) for g in groups for k in ref[g])


def maps_are_the_float64_value_rounded_once(got, ref):
    return all(R.same_bits(got["maps"][k], ref["maps"][k][0].float()) for k in ("skill", "spread"))


# ---- every bound admits the kernel's order and the reference's ----------------------------------------------------------------------
@pytest.mark.parametrize("arm", R.ARMS)
def test_integer_cases_bit_exact_maps_and_bounded_scores(arm):
    for M in (m for m in R.ALL_M if R.sort_arm(m) == arm):
        c = R.integer_case(M)
        ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"])
        for fma in (True, False):
            got = R.kernel_f32(c["x"], c["t"], c["cl"], c["w"], fma=fma)
            assert maps_are_the_float64_value_rounded_once(got, ref), (M, fma)
            judge_all(got, ref, f"M={M} fma={fma}")
        orc = R.oracle_f32(c["x"], c["t"], c["cl"], c["w"])
        assert maps_are_the_float64_value_rounded_once(orc, ref), M  # exact sums, one division: the reference's fp32 gives the same bits
        judge_all(orc, ref, f"M={M} reference in fp32")
        # the power-of-two normalisation is exact on these integers, so the fused load leaves integers
        n = R.POW2_NORM
        x2 = R.inv_norm_f32(c["x"], torch.tensor(n["mean"]), torch.tensor(n["std"]), n["target_std"])
        assert torch.equal(x2.double(), c["x"].double() * 2 * torch.tensor(n["std"]).double().view(1, -1, 1, 1) + torch.tensor(n["mean"]).double().view(1, -1, 1, 1))
        assert float((x2.abs().amax() * 63 * 64) * 2) < 2 ** 24


@pytest.mark.parametrize("M", R.PHYS_M)
def test_physical_scale_within_the_bounds(M):
    c = R.physical_case(M)
    assert torch.equal(c["x"], (c["v"] / 0.5) * c["std"].view(1, -1, 1, 1, 1) + c["mean"].view(1, -1, 1, 1, 1))
    for l in range(c["x"].shape[2]):
        x, t, cl = c["x"][:, :, l], c["t"][:, l], c["cl"][:, l]
        ref = R.scores_ref(x, t, cl, c["w"])
        r = [judge_all(R.kernel_f32(x, t, cl, c["w"], fma=fma), ref, f"M={M} lead {l} fma={fma}") for fma in (True, False)]
        ro = judge_all(R.oracle_f32(x, t, cl, c["w"]), ref, f"M={M} lead {l} reference in fp32")
        print(f"physical M={M} lead {l}: worst err / bound: restatement {max(r):.3f}, reference in fp32 {ro:.3f}")


@pytest.mark.parametrize("H,W", R.FINISH_SHAPES)
def test_finish_loop_cases_within_the_bounds(H, W):
    c = R.finish_case(H, W)
    assert -(-H * W // R.TPB) in (65, 129)
    ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"])
    judge_all(R.kernel_f32(c["x"], c["t"], c["cl"], c["w"]), ref, "restatement")
    judge_all(R.oracle_f32(c["x"], c["t"], c["cl"], c["w"]), ref, "reference in fp32")
    x = c["x"].clone()
    x[1, 0, H - 1, W - 1] = float("nan")  # one NaN member in the last record
    for nan_channel, finite in ((-1, False), (0, True)):
        ref = R.scores_ref(x, c["t"], c["cl"], c["w"], nan_channel)
        assert bool(torch.isfinite(ref["scores"]["crps"][0]).all()) == finite and bool(torch.isfinite(ref["scores"]["ens_acc"][0]).all())
        judge_all(R.kernel_f32(x, c["t"], c["cl"], c["w"], nan_channel), ref, f"NaN member, nan_channel {nan_channel}")
        judge_all(R.oracle_f32(x, c["t"], c["cl"], c["w"], nan_channel), ref, f"NaN member, nan_channel {nan_channel}, reference in fp32")


@pytest.mark.parametrize("case", R.GUARD_CASES)
def test_guard_band_cases_within_the_bounds(case):
    M, C, L, H, W, sst = case
    c = R.guard_case(*case)
    for l in range(L):
        x, t, cl = c["x"][:, :, l], c["truth_table"][c["t_slots"][l]], c["clim_table"][c["c_slots"][l]]
        ref = R.scores_ref(x, t, cl, c["w"], sst)
        judge_all(R.kernel_f32(x, t, cl, c["w"], sst), ref, f"lead {l}")
        judge_all(R.oracle_f32(x, t, cl, c["w"], sst), ref, f"lead {l} reference in fp32")


@pytest.mark.parametrize("nan_channel", [0, 1, 2, 3])
@pytest.mark.parametrize("M", [R.NAN_M, 1])
def test_nan_inf_table_follows_the_reference(M, nan_channel):
    c = R.nan_table_case(M)
    ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"], nan_channel)
    want = S.ensemble_scores(c["x"].double(), c["t"].double(), c["cl"].double(), c["w"].double(), sst_channel=nan_channel)  # the contract
    for k in R.KEYS:
        assert R.ratio_of(ref["scores"][k][0], want[k], 1e-12 * want[k].abs().nan_to_num(posinf=0.0) + 1e-300) <= 1.0, k
    assert R.ratio_of(ref["maps"]["skill"][0], S.pointwise_crps_skill(c["x"].double(), c["t"].double().unsqueeze(0), 0), 1e-300) <= 1.0
    assert R.ratio_of(ref["maps"]["spread"][0], S.pointwise_crps_spread(c["x"].double(), 0), 1e-300) <= 1.0
    sc = ref["scores"]
    if M > 1:  # what the table is there for: each rule shows
        assert bool(torch.isfinite(sc["crps"][0][0])) == (nan_channel == 0)  # NaN patterns only: finite by nanmean alone
        assert bool(torch.isfinite(sc["ens_acc"][0][0]))  # ACC: always its own three nanmeans
        assert bool(torch.isinf(sc["crps_skill"][0][1])) == (nan_channel == 1)
        # an inf member: crps = inf - inf = NaN at that point, which nanmean leaves out; inf in truth: crps = +inf stays in
        assert bool(torch.isinf(sc["crps"][0][1])) == (nan_channel == 1) and bool(torch.isnan(sc["crps"][0][1])) == (nan_channel != 1)
        assert bool(torch.isnan(sc["crps"][0][2])) and bool(torch.isnan(sc["ens_acc"][0][2]))  # all-NaN channel, nanmean or not
    assert all(bool(torch.isfinite(sc[k][0][3])) for k in R.KEYS)
    judge_all(R.kernel_f32(c["x"], c["t"], c["cl"], c["w"], nan_channel), ref, "restatement")
    judge_all(R.oracle_f32(c["x"], c["t"], c["cl"], c["w"], nan_channel), ref, "reference in fp32")


# ---- every planted defect is caught -------------------------------------------------------------------------------------------------
def _unit(M):
    """the unit-scale channel of the physical case, lead 0"""
    c = R.physical_case(M)
    return c["x"][:, 5:, 0], c["t"][5:, 0], c["cl"][5:, 0], c["w"]


def _z50(M):
    c = R.physical_case(M)
    return c["x"][:, :1, 0], c["t"][:1, 0], c["cl"][:1, 0], c["w"]


@pytest.mark.parametrize("defect", ["swap", "short"])
@pytest.mark.parametrize("arm", R.ARMS)
def test_sort_defects_are_caught_by_the_integer_and_the_unit_scale_cases(arm, defect):
    """... and NOT reliably at physical scale, where the worst-case spread bound is wider than one exchanged pair: printed below"""
    lo = max(arm[1] - 7, 2)
    for M in (lo, arm[1]):
        c = R.integer_case(M)
        ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"])
        bad = R.kernel_f32(c["x"], c["t"], c["cl"], c["w"], defect=defect)
        assert R.same_bits(bad["maps"]["skill"], ref["maps"]["skill"][0].float())
        assert not R.same_bits(bad["maps"]["spread"], ref["maps"]["spread"][0].float()), M  # the bit-equality breaks
        assert R.ratio_of(bad["maps"]["spread"], *ref["maps"]["spread"]) > 1.0, M  # and so does the bound
    for M in (m for m in R.PHYS_M if R.sort_arm(m) == arm):
        x, t, cl, w = _unit(M)
        ref = R.scores_ref(x, t, cl, w)
        assert R.ratio_of(R.kernel_f32(x, t, cl, w)["maps"]["spread"], *ref["maps"]["spread"]) <= 1.0
        assert R.ratio_of(R.kernel_f32(x, t, cl, w, defect=defect)["maps"]["spread"], *ref["maps"]["spread"]) > 1.0, M
        x, t, cl, w = _z50(M)
        ref = R.scores_ref(x, t, cl, w)
        print(f"{defect} M={M}: z50 spread map err / bound {R.ratio_of(R.kernel_f32(x, t, cl, w, defect=defect)['maps']['spread'], *ref['maps']['spread']):.3f}")


@pytest.mark.parametrize("defect", ["MM", "weight"])
@pytest.mark.parametrize("M", [2, 8, 9, 25, 33, 41, 50, 64])
def test_scale_and_weight_defects_break_the_spread_bound(M, defect):
    c = R.integer_case(M)
    ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"])
    bad = R.kernel_f32(c["x"], c["t"], c["cl"], c["w"], defect=defect)
    assert not R.same_bits(bad["maps"]["spread"], ref["maps"]["spread"][0].float())
    assert R.ratio_of(bad["maps"]["spread"], *ref["maps"]["spread"]) > 1.0
    assert R.ratio_of(bad["scores"]["crps_spread"], *ref["scores"]["crps_spread"]) > 1.0
    assert R.ratio_of(bad["scores"]["crps_skill"], *ref["scores"]["crps_skill"]) <= 1.0
    if M in R.PHYS_M:  # at physical scale too: both move every point by far more than the bound
        p = R.physical_case(M)
        x, t, cl = p["x"][:, :, 0], p["t"][:, 0], p["cl"][:, 0]
        ref = R.scores_ref(x, t, cl, p["w"])
        bad = R.kernel_f32(x, t, cl, p["w"], defect=defect)
        for ch in range(len(R.PHYS)):
            assert R.ratio_of(bad["maps"]["spread"][ch], ref["maps"]["spread"][0][ch], ref["maps"]["spread"][1][ch]) > 1.0, R.PHYS[ch][0]


@pytest.mark.parametrize("defect", ["record_twice", "point_HW"])
def test_reduction_and_extent_defects_break_the_score_bounds(defect):
    cases = [R.integer_case(M) for M in (1, 7, 50)] + [R.finish_case(*hw) for hw in R.FINISH_SHAPES]
    p = R.physical_case(50)
    cases.append(dict(x=p["x"][:, :, 0], t=p["t"][:, 0], cl=p["cl"][:, 0], w=p["w"]))
    for c in cases:
        ref = R.scores_ref(c["x"], c["t"], c["cl"], c["w"])
        good, bad = R.kernel_f32(c["x"], c["t"], c["cl"], c["w"]), R.kernel_f32(c["x"], c["t"], c["cl"], c["w"], defect=defect)
        assert worst_of(good, ref) <= 1.0
        assert worst_of(bad, ref, ("maps",)) <= 1.0  # the point maps do not see it
        for k in ("crps_skill", "ens_mse"):
            assert R.ratio_of(bad["scores"][k], *ref["scores"][k]) > 1.0, (defect, k, tuple(c["x"].shape))
        assert R.ratio_of(bad["validation"]["single_mse"], *ref["validation"]["single_mse"]) > 1.0


@pytest.mark.parametrize("M", R.PHYS_M)
def test_truth_of_the_next_lead_breaks_the_bounds(M):
    c = R.physical_case(M)
    L = c["x"].shape[2]
    for l in range(L):
        x, cl = c["x"][:, :, l], c["cl"][:, l]
        ref = R.scores_ref(x, c["t"][:, l], cl, c["w"])
        bad = R.kernel_f32(x, c["t"][:, (l + 1) % L], cl, c["w"])
        for k in ("crps_skill", "ens_mse", "crps", "ens_acc"):
            r = torch.stack([torch.as_tensor(R.ratio_of(bad["scores"][k][ch], ref["scores"][k][0][ch], ref["scores"][k][1][ch])) for ch in range(len(R.PHYS))])
            # (ACC of two independent draws is near 0 with either truth, and its interval bound is wide where b_mean is not small
            # against the ensemble-mean anomaly: only the small-centre channels q700 and unit are held to it)
            assert bool((r[4:] > 1.0).all() if k == "ens_acc" else (r > 1.0).all()), (k, r.tolist())
        assert R.ratio_of(bad["maps"]["skill"], *ref["maps"]["skill"]) > 1.0
