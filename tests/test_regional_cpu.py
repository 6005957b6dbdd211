"""Host side of the regional scores (csrc/regional.hip, ladcast_amd.evaluate.regional, the --region flags of evaluate_ens_gpu).  No GPU:
  a. the fp32 restatement of the kernel (tests/regional_refs.py) meets the oracle at every case; the oracle equals the brute-force loop;
     every planted defect fails at least one case
  b. regional_scores: pooling, empty regions, one member, the scale of the weights, the CRPS identity
  c. region_mask: the named regions, inclusive bounds, the box across 0 degrees, surfaces
  d. the command line's file handling with an injected scorer
  e. rollout_regional raises the shared exceptions in the shared order
  f. the library's exports"""
import json

import numpy as np
import pytest
import torch

from tests import regional_refs as R


# ---- a. the restatement against the oracle -----------------------------------------------------------------------------------------------
def _ref(c):
    return R.regional_ref(c["x"], c["t"], c["w"], c["mask"], c["R"], c["cl"])


def _restated(c, defect=None):
    return R.kernel_f32(c["v"], c["t"], c["w"], c["mask"], c["R"], c["cl"], c["norm"], defect=defect)


def test_clean_restatement_meets_every_bound():
    worst = 0.0
    for name, c in R.cpu_cases():
        got, ref = _restated(c), _ref(c)
        worst = max(worst, R.check(got, ref, name))
        if name.startswith("integer"):
            assert R.exact(got, ref), f"{name}: the integer cases are exact"
    print(f"worst err / bound {worst:.4f}")


def test_oracle_equals_the_definitions_point_by_point():
    for c in (R.integer_case(9, 3, 50, 32), R.integer_case(1, 1, 257, 3), R.nan_table_case(), R.physical_case(8), R.named_case()):
        ref, b = _ref(c), R.brute_force(c["x"], c["t"], c["w"], c["mask"], c["R"], c["cl"])
        assert torch.equal(ref["counts"], b["counts"])
        s = ref["sums"][0]
        assert torch.equal(torch.isnan(s), torch.isnan(b["sums"])) and torch.equal(torch.isinf(s), torch.isinf(b["sums"]))
        fin = torch.isfinite(s)
        assert torch.allclose(s[fin], b["sums"][fin], rtol=1e-11, atol=1e-9)


def test_nan_table_counts():
    c = R.nan_table_case()
    ref = _ref(c)["counts"]
    bits, kind = R.region_bits(c["mask"], c["R"]), c["kind"]
    for r in range(c["R"]):
        n = [int((bits[r] & (kind == k)).sum()) for k in range(len(R.PATTERNS))]
        assert all(v > 0 for v in n), (r, n)  # every pattern occurs in every region
        assert ref[r, 0].tolist() == ref[r, 1].tolist() == [n[0] + n[3] + n[4], n[1] + n[2], n[0] + n[4]]
    assert not bool(bits[:, c["outside"]].any()) and bool(c["outside"][2 * R.TPB : 3 * R.TPB].all())  # a whole tile outside every region
    clean = R.nan_table_case(poison=False)
    a, b = _ref(c), _ref(clean)
    assert torch.equal(a["counts"], b["counts"]) and torch.equal(torch.nan_to_num(a["sums"][0], nan=7.0), torch.nan_to_num(b["sums"][0], nan=7.0))


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    cases = [("nan table", R.nan_table_case()), ("physical", R.physical_case(8)), ("integer", R.integer_case(9, 3, 50, 32)),
             ("integer", R.integer_case(2, 5, 103, 3)), ("named", R.named_case())]
    caught = []
    for name, c in cases:
        if defect == "wrap_threshold":
            got = _restated(R.named_case(defect=defect)) if name == "named" else _restated(c)
        else:
            got = _restated(c, defect)
        if not R.passes(got, _ref(c)):
            caught.append(name)
    assert caught, f"defect {defect!r} passes every case: the tables have no teeth"
    print(defect, "caught by", caught)


def test_case_tables_cover_the_kernel_paths():
    from tests.score_edge_refs import ARMS, sort_arm

    assert {sort_arm(M) for M in R.INT_M} == {(8, 8), (16, 16), (32, 24), (32, 32), (64, 56), (64, 64)} <= set(ARMS)
    assert {sort_arm(M) for M in (8, 9, 24, 25)} == {(8, 8), (16, 16), (32, 24), (32, 32)}  # both sides of two edges of the ladder
    assert [-(-H * W // R.TPB) for H, W in R.INT_GRIDS] == [1, 3, 2] and all(H * W % R.TPB for H, W in R.INT_GRIDS)
    assert [R.n_records(H * W) for _, H, W, _ in R.INT_EXTRA] == [2]  # several records
    c = R.integer_case(9, 5, 103, 32)
    cnt = _ref(c)["counts"]
    bits = R.region_bits(c["mask"], 32)
    assert int(cnt[5].sum()) == 0 and cnt[7, 0].tolist() == [1, 0, 1] and bool(bits[7, -1]) and int(cnt[31, 0, 0]) > 100  # empty / one point / bit 31
    assert int((bits.sum(0) > 1).sum()) > 100 and int((bits.sum(0) == 0).sum()) > 10  # overlap; points of no region
    c3 = R.integer_case(9, 5, 103, 3)
    assert _ref(c3)["counts"][:, 0, 0].tolist() == [515, 0, 1]
    assert bool((torch.as_tensor(c3["mask"]) >> 3).any())  # garbage above bit R - 1


# ---- b. regional_scores ------------------------------------------------------------------------------------------------------------------
def _sums_of(M, N, seed, acc=True):
    """sufficient statistics of N random points in float64, and the points"""
    g = np.random.default_rng(seed)
    x, t, a, w = g.normal(1.0, 2.0, (M, N)), g.normal(1.0, 2.0, N), g.normal(1.0, 0.5, N), g.uniform(0.2, 1.5, N)
    return dict(x=x, t=t, a=a, w=w), _stats(x, t, a, w)


def _stats(x, t, a, w):
    M = x.shape[0]
    mean = x.mean(0)
    e = mean - t
    var = x.var(0, ddof=1) if M > 1 else np.zeros_like(t)
    skill = np.abs(t - x).mean(0)
    coef = 2.0 * np.arange(1, M + 1) - M - 1
    spread = 2.0 / (M * (M - 1)) * (np.sort(x, 0) * coef[:, None]).sum(0) if M > 1 else np.zeros_like(t)
    fa, ta = mean - a, t - a
    s = np.array([w.sum(), (w * e).sum(), (w * e * e).sum(), (w * var).sum(), (w * skill).sum(), (w * spread).sum(), w.sum(), (w * fa * ta).sum(),
                  (w * fa * fa).sum(), (w * ta * ta).sum()])
    return s, np.array([t.size, 0, t.size])


@pytest.mark.parametrize("M", [1, 2, 7, 50])
def test_regional_scores_pooling_and_identities(M):
    from ladcast_amd.evaluate import regional_scores

    p1, (s1, n1) = _sums_of(M, 300, 11 * M)
    p2, (s2, n2) = _sums_of(M, 450, 13 * M)
    cat = {k: np.concatenate([p1[k], p2[k]], -1) for k in p1}
    s12, n12 = _stats(cat["x"], cat["t"], cat["a"], cat["w"])
    pooled, direct = regional_scores(s1 + s2, n1 + n2, M), regional_scores(s12, n12, M)
    for k in ("bias", "ens_mse", "rmse", "ens_var", "crps_skill", "crps_spread", "crps", "ens_acc", "weight") + (("ssr",) if M > 1 else ()):
        assert abs(pooled[k] - direct[k]) <= 1e-12 * max(abs(direct[k]), 1.0), k
    assert pooled["n_valid"] == 750
    # the definitions, from the points
    w = cat["w"]
    mean = cat["x"].mean(0)
    assert abs(direct["bias"] - (w * (mean - cat["t"])).sum() / w.sum()) <= 1e-12
    assert abs(direct["rmse"] - np.sqrt((w * (mean - cat["t"]) ** 2).sum() / w.sum())) <= 1e-12
    assert direct["crps"] == direct["crps_skill"] - direct["crps_spread"] / 2
    fa, ta = mean - cat["a"], cat["t"] - cat["a"]
    assert abs(direct["ens_acc"] - (w * fa * ta).sum() / np.sqrt((w * fa * fa).sum() * (w * ta * ta).sum())) <= 1e-12
    if M == 1:
        assert np.isnan(direct["ssr"]) and direct["ens_var"] == 0 and direct["crps_spread"] == 0
    else:
        assert abs(direct["ssr"] - np.sqrt((M + 1) / M) * np.sqrt(direct["ens_var"] / direct["ens_mse"])) <= 1e-15
    # averaging the two initial times' scores is NOT the pooled score: the sums have to be pooled
    a, b = regional_scores(s1, n1, M), regional_scores(s2, n2, M)
    assert abs(0.5 * (a["rmse"] + b["rmse"]) - direct["rmse"]) > 1e-6
    # the scale of the weights cancels; leading dimensions
    both = regional_scores(np.stack([s12, 8 * s12]), np.stack([n12, n12]), M)
    for k in ("bias", "ens_mse", "rmse", "ens_var", "crps_skill", "crps_spread", "crps", "ens_acc"):
        assert both[k].shape == (2,) and both[k][0] == direct[k] and abs(both[k][1] - direct[k]) <= 1e-13 * max(abs(direct[k]), 1.0), k
    assert both["weight"][1] == 8 * both["weight"][0]


def test_regional_scores_empty_regions_and_bad_shapes():
    from ladcast_amd.evaluate import REGIONAL_SCORE_NAMES, regional_scores

    _, (s, n) = _sums_of(4, 50, 3)
    sums, counts = np.zeros((3, 2, 10)), np.zeros((3, 2, 3), dtype=np.int32)
    sums[0, 0], counts[0, 0] = s, n
    sums[2, 1, :6], counts[2, 1] = s[:6], (50, 0, 0)  # valid points, none ACC-valid (no climatology)
    counts[1, 1] = (0, 9, 0)  # a region whose points are all invalid
    sc = regional_scores(sums, counts, 4)
    assert set(sc) == set(REGIONAL_SCORE_NAMES)
    for k in ("bias", "ens_mse", "rmse", "ens_var", "ssr", "crps_skill", "crps_spread", "crps", "ens_acc"):
        assert sc[k].shape == (3, 2) and np.isfinite(sc[k][0, 0]) and np.isnan(sc[k][1]).all() and np.isnan(sc[k][0, 1]) and np.isnan(sc[k][2, 0]), k
    assert np.isfinite(sc["rmse"][2, 1]) and np.isnan(sc["ens_acc"][2, 1])
    assert sc["n_valid"].tolist() == [[50, 0], [0, 0], [0, 50]] and sc["weight"][1].tolist() == [0.0, 0.0]
    for bad in ((np.zeros((2, 9)), np.zeros((2, 3))), (np.zeros((2, 10)), np.zeros((3, 3))), (np.zeros(10), np.zeros(2))):
        with pytest.raises(ValueError):
            regional_scores(*bad, 4)
    with pytest.raises(ValueError):
        regional_scores(np.zeros(10), np.zeros(3), 0)


# ---- c. region_mask ------------------------------------------------------------------------------------------------------------------------
def _bit(mask, r):
    return ((mask >> np.uint32(r)) & np.uint32(1)).astype(bool)


def test_named_regions_on_the_120_row_grid():
    from ladcast_amd.evaluate import NAMED_REGIONS, region_mask
    from ladcast_amd.evaluate.evaluate_ens_gpu import row_latitudes
    from ladcast_amd.evaluate.track import longitude_grid

    names = list(NAMED_REGIONS)
    assert names == ["global", "tropics", "extratropics", "nh_extratropics", "sh_extratropics", "arctic", "antarctic", "europe", "north_america",
                     "north_atlantic", "north_pacific", "east_asia", "ausnz"]
    lat, lon = row_latitudes(120), longitude_grid()
    mask = region_mask(list(NAMED_REGIONS.values()), lat, lon)
    assert mask.shape == (120, 240) and mask.dtype == np.uint32
    b = {n: _bit(mask, i) for i, n in enumerate(names)}
    assert b["global"].all()
    assert np.array_equal(b["extratropics"], b["nh_extratropics"] | b["sh_extratropics"]) and not (b["nh_extratropics"] & b["sh_extratropics"]).any()
    assert np.array_equal(b["extratropics"], ~b["tropics"]) and np.array_equal(b["tropics"], np.broadcast_to((np.abs(lat) <= 20)[:, None], mask.shape))
    eu = b["europe"]
    assert np.array_equal(eu.any(1), (lat >= 35) & (lat <= 75))
    assert np.array_equal(eu.any(0), (lon >= 347.5) | (lon <= 42.5)) and eu.any(0)[lon >= 347.5].all() and eu.any(0).sum() == 8 + 29
    na = b["north_america"]
    assert np.array_equal(na.any(0), (lon >= 240) & (lon <= 285)) and na[:, lon == 240.0].any() and na[:, lon == 285.0].any()  # inclusive
    assert (b["arctic"] <= b["nh_extratropics"]).all() and (b["antarctic"] <= b["sh_extratropics"]).all()
    for n in names:
        assert b[n].any(), n


def test_region_mask_bounds_wrap_and_surfaces():
    from ladcast_amd.evaluate import Region, region_mask

    lat, lon = np.array([-30.0, -10.0, 0.0, 10.0, 30.0]), np.arange(8) * 45.0
    m = region_mask([Region("a", -10, 10, 45, 90), Region("b", 0, 0, 315, 45), Region("c", -90, 90, -45, 45), Region("d", -30, -30, 0, 360),
                     Region("e", 10, 30, 90, 90)], lat, lon)
    assert _bit(m, 0).nonzero()[0].tolist() == [1, 1, 2, 2, 3, 3] and _bit(m, 0).nonzero()[1].tolist() == [1, 2] * 3  # both bounds inclusive
    assert _bit(m, 1).nonzero()[0].tolist() == [2, 2, 2] and _bit(m, 1).nonzero()[1].tolist() == [0, 1, 7]  # across 0 degrees
    assert np.array_equal(_bit(m, 2), np.broadcast_to(np.isin(np.arange(8), [0, 1, 7]), (5, 8)))  # a negative longitude is taken modulo 360
    assert np.array_equal(_bit(m, 3), np.broadcast_to((lat == -30)[:, None], (5, 8)))
    assert _bit(m, 4).sum() == 2 and _bit(m, 4)[3:, 2].all()
    assert np.array_equal(region_mask([Region("x", -90, 90, 0, 360)], lat, lon - 360.0), np.ones((5, 8), dtype=np.uint32))
    land = np.zeros((5, 8))
    land[:, :3] = 1.0
    land[0, 0] = 0.5
    land[0, 1] = 0.49
    ms = region_mask([Region("l", -90, 90, 0, 360, "land"), Region("s", -90, 90, 0, 360, "sea"), Region("c", -10, 10, 45, 90, "sea")], lat, lon, land)
    assert np.array_equal(_bit(ms, 0), land >= 0.5) and np.array_equal(_bit(ms, 1), land < 0.5) and not _bit(ms, 2).any()
    with pytest.raises(ValueError, match="land_sea_mask"):
        region_mask([Region("l", -90, 90, 0, 360, "land")], lat, lon)
    with pytest.raises(ValueError):
        region_mask([Region("l", -90, 90, 0, 360, "ice")], lat, lon, land)
    with pytest.raises(ValueError):
        region_mask([Region("l", 10, -10, 0, 360)], lat, lon)
    with pytest.raises(ValueError):
        region_mask([], lat, lon)
    with pytest.raises(ValueError):
        region_mask([Region(str(i), -90, 90, 0, 360) for i in range(33)], lat, lon)
    with pytest.raises(ValueError):
        region_mask([Region("l", -90, 90, 0, 360, "land")], lat, lon, land[:4])
    m32 = region_mask([Region(str(i), -90, 90, 0, 360) for i in range(32)], lat, lon)
    assert m32.dtype == np.uint32 and (m32 == 0xFFFFFFFF).all()
    assert np.array_equal(R.named_mask(24, 48), R.named_mask(24, 48, defect=None))
    assert (R.named_mask(24, 48, defect="wrap_threshold") != R.named_mask(24, 48)).sum() == _bit(R.named_mask(24, 48), 7)[:, 24:].sum() > 0


# ---- d. the command line -------------------------------------------------------------------------------------------------------------------
SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")


def _run_main(tmp_path, name, extra, M=3):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    if not res.exists():
        res.mkdir()
        for ts in (2018123000, 2018123106):
            np.save(res / f"latent_{ts}.npy", np.zeros((M, 1, 1, 1, 1), dtype=np.float32))
    C, T = 3, 4
    n_reg = sum(f in ("--region", "--region_box") for f in extra)
    g = np.random.default_rng(5)
    per_init = []

    def score(path, time_str, t_slots, c_slots):
        out = {k: np.full((C, T), 1.0 + i, dtype=np.float32) for i, k in enumerate(SCORES)}
        if n_reg:
            s = g.uniform(0.5, 2.0, (n_reg, C, T, 10))
            n = g.integers(1, 50, (n_reg, C, T, 3)).astype(np.int32)
            n[-1] = 0  # the last region holds no point
            s[-1] = 0.0
            per_init.append((s, n))
            out.update(regional_sums=torch.from_numpy(s), regional_counts=torch.from_numpy(n))
        return out

    out_dir = tmp_path / name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + extra, score=score)
    return out_dir, out, per_init


def test_main_region_flags_write_the_regional_files(tmp_path):
    from ladcast_amd.evaluate import REGIONAL_SCORE_NAMES, regional_scores

    plain, _, _ = _run_main(tmp_path, "plain", [])
    flags = ["--region", "tropics", "--region_box", "alps", "43", "49", "5", "17", "--region", "europe", "--region_box", "dateline", "-10", "10", "170", "-170"]
    with_reg, out, per_init = _run_main(tmp_path, "regions", flags)
    before = sorted(p.name for p in plain.iterdir())
    assert before == sorted([f"{t}_{k}.npy" for t in ("2018123000", "2018123106") for k in SCORES] + [f"{k}.npy" for k in SCORES] + ["timestamp.npy"])
    new = ["regional_sums.npy", "regional_counts.npy", "regions.json"] + [f"regional_{k}.npy" for k in REGIONAL_SCORE_NAMES]
    assert sorted(p.name for p in with_reg.iterdir()) == sorted(before + new)
    for p in plain.iterdir():  # a run without region flags writes exactly what it wrote before
        assert (with_reg / p.name).read_bytes() == p.read_bytes(), p.name
    Rn, C, T, M = 4, 3, 4, 3
    s, n = np.load(with_reg / "regional_sums.npy"), np.load(with_reg / "regional_counts.npy")
    assert s.shape == (Rn, C, T, 10) and s.dtype == np.float64 and n.shape == (Rn, C, T, 3) and n.dtype == np.int64
    assert len(per_init) == 2 and np.array_equal(s, per_init[0][0] + per_init[1][0]) and np.array_equal(n, per_init[0][1].astype(np.int64) + per_init[1][1])
    sc = regional_scores(s, n, M)
    for k in REGIONAL_SCORE_NAMES:
        f = np.load(with_reg / f"regional_{k}.npy")
        assert f.shape == (Rn, C, T) and np.array_equal(f, sc[k], equal_nan=True) and np.array_equal(f, out[f"regional_{k}"], equal_nan=True), k
    assert np.isfinite(np.load(with_reg / "regional_rmse.npy")[:3]).all() and np.isnan(np.load(with_reg / "regional_rmse.npy")[3]).all()
    meta = json.loads((with_reg / "regions.json").read_text())
    assert meta["members"] == M and len(meta["sums"]) == 10 and len(meta["counts"]) == 3
    assert [m["name"] for m in meta["regions"]] == ["tropics", "europe", "alps", "dateline"]  # named regions first
    assert meta["regions"][1]["boxes"] == [[35.0, 75.0, 347.5, 42.5]] and meta["regions"][3]["boxes"] == [[-10.0, 10.0, 170.0, -170.0]]
    assert all(set(m) == {"name", "boxes", "surface", "n_points", "weight"} for m in meta["regions"])
    # --region_per_init
    per, out2, pi2 = _run_main(tmp_path, "per_init", flags + ["--region_per_init"])
    assert sorted(p.name for p in per.iterdir()) == sorted(before + new + ["regional_sums_per_init.npy"])
    a = np.load(per / "regional_sums_per_init.npy")
    assert a.shape == (2, Rn, C, T, 10) and a.dtype == np.float64 and np.array_equal(a[0], pi2[0][0]) and np.array_equal(a[1], pi2[1][0])
    assert np.array_equal(a.sum(0), np.load(per / "regional_sums.npy"))


def test_main_region_flags_refuse_bad_entries(tmp_path):
    for bad in (["--region", "atlantis"], ["--region_box", "a", "0", "x", "0", "1"], ["--region_box", "a", "10", "-10", "0", "1"],
                ["--region", "tropics", "--region_box", "tropics", "0", "1", "0", "1"], ["--region", "tropics", "--region_surface", "europe", "land"],
                ["--region", "tropics", "--region_surface", "tropics", "ice"], ["--region", "tropics", "--region_surface", "tropics", "land"],
                ["--region_per_init"], ["--region_box", "a", "0", "nan", "0", "1"]):
        with pytest.raises(ValueError):
            _run_main(tmp_path, "bad", bad)
    with pytest.raises(ValueError, match="--region needs"):  # a scorer that does not return the regional arrays
        from ladcast_amd.evaluate import evaluate_ens_gpu as EG

        EG.main(["--result_path", str(tmp_path / "rollout"), "--output", str(tmp_path / "o"), "--start_date", "2018-12-29", "--end_date",
                 "2019-01-01T18", "--total_lead_time_hour", "24", "--region", "tropics"],
                score=lambda *a: {k: np.zeros((3, 4), dtype=np.float32) for k in SCORES})


def test_regions_json_counts_points_and_weights():
    from ladcast_amd.evaluate import NAMED_REGIONS
    from ladcast_amd.evaluate.regional import region_metadata

    regions = [NAMED_REGIONS["global"], NAMED_REGIONS["tropics"], NAMED_REGIONS["europe"]]
    mask = R.named_mask(24, 48, ["global", "tropics", "europe"])
    w = R.cos_weights(24).numpy()
    meta = region_metadata(regions, mask, w)
    assert [m["n_points"] for m in meta] == [24 * 48, int(_bit(mask, 1).sum()), int(_bit(mask, 2).sum())] and meta[2]["n_points"] > 0
    assert abs(meta[0]["weight"] - 48 * w.astype(np.float64).sum()) <= 1e-9 and meta[1]["weight"] < meta[0]["weight"]
    json.dumps(meta)


# ---- e. the wrapper's argument errors ------------------------------------------------------------------------------------------------------
_M, _C, _L, _H, _W = 2, 1, 1, 3, 8


def _call(*, forecast=None, weight=None, mask=None, R_=2, **kw):
    from ladcast_amd import evaluate as E

    x = torch.zeros(_M, _C, _L, _H, _W) if forecast is None else forecast
    t, w = torch.zeros(_C, _L, _H, _W), torch.ones(_H) if weight is None else weight
    return E.rollout_regional(x, t, w, np.ones((_H, _W), dtype=np.uint32) if mask is None else mask, R_, **kw)


def test_rollout_regional_shares_the_argument_errors():
    cl = torch.zeros(_C, _L, _H, _W)
    cases = [
        (dict(forecast=torch.zeros(_M, _C, _H, _W)), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(lead_dim=1), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(forecast=torch.zeros(_M, _C, _L, _H, _W, dtype=torch.float64)), NotImplementedError, "fp32 only"),
        (dict(forecast=torch.zeros(65, _C, _L, _H, _W)), ValueError, "members"),
        (dict(clim=torch.zeros(_C, _L, _H + 1, _W)), ValueError, "clim must be"),
        (dict(weight=torch.ones(_H + 1)), ValueError, "lat_weight must have one value per latitude row"),
        (dict(mean=torch.zeros(_C)), ValueError, "mean and std go together"),
        (dict(mean=torch.zeros(_C + 1), std=torch.ones(_C + 1)), ValueError, r"mean / std must hold one value per channel \(1\)"),
        (dict(R_=0), ValueError, "regions"),
        (dict(R_=33), ValueError, "regions"),
        (dict(mask=np.ones((_H, _W + 1), dtype=np.uint32)), ValueError, "region_mask must be"),
        (dict(mask=np.ones((_H, _W))), ValueError, "integer"),
        (dict(l_off=-1), ValueError, "l_off"),
        (dict(out={}), ValueError, "out must be"),
    ]
    for kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            _call(**kw)
    with pytest.raises(RuntimeError, match="device tensors"):  # nothing wrong but the host tensors
        _call()
    with pytest.raises(RuntimeError, match="device tensors"):
        _call(clim=cl, mean=torch.zeros(_C), std=torch.ones(_C), mask=torch.ones(_H, _W, dtype=torch.int64))


def test_score_latent_rollout_refuses_bad_region_arguments():
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    args = (torch.zeros(2, 1, 1, 2, 2), None, None, None, torch.zeros(3, 1, 4, 4), [0], None, None, torch.ones(4))
    with pytest.raises(ValueError, match="regions"):
        EG.score_latent_rollout(*args, region_mask=np.ones((4, 4), dtype=np.uint32))
    with pytest.raises(ValueError, match="regions"):
        EG.score_latent_rollout(*args, regions=33, region_mask=np.ones((4, 4), dtype=np.uint32))
    with pytest.raises(ValueError, match="region_mask"):
        EG.score_latent_rollout(*args, regions=2)


# ---- f. the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_symbols():
    from ladcast_amd import hip

    for name in ("ldc_rollout_regional", "ldc_rollout_regional_workspace_bytes"):
        assert hasattr(hip.lib, name) and name in hip.SIGNATURES
    assert hip.lib.ldc_abi_version() == 5
    assert (hip.REGIONS_MAX, hip.REGIONAL_MAX_MEMBERS, hip.REGIONAL_SUMS, hip.REGIONAL_COUNTS) == (R.MAX_R, R.MAX_M, R.NS, R.NC)
    wb = hip.lib.ldc_rollout_regional_workspace_bytes
    for M, Rn, C, L, H, W in ((5, 3, 2, 2, 3, 50), (64, 1, 1, 1, 16, 16), (9, 32, 2, 1, 9, 257), (50, 32, 84, 4, 120, 240)):
        assert wb(M, Rn, C, L, H, W) == R.workspace_bytes(C, L, H * W)
    assert wb(50, 1, 84, 4, 120, 240) == wb(50, 32, 84, 4, 120, 240) == 84 * 4 * 15 * 3072  # 15.5 MB: the record does not depend on R
    assert wb(50, 32, 1, 1, 120, 240) / (120 * 240) <= 1.6  # 1.5 bytes per point, plus the last record's unused tiles
    for bad in ((0, 1, 1, 1, 4, 4), (65, 1, 1, 1, 4, 4), (4, 0, 1, 1, 4, 4), (4, 33, 1, 1, 4, 4), (4, 1, 0, 1, 4, 4), (4, 1, 65536, 1, 4, 4),
                (4, 1, 1, 0, 4, 4), (4, 1, 1, 65536, 4, 4), (4, 1, 1, 1, 0, 4), (4, 1, 1, 1, 4, 0), (4, 1, 1, 1, 4097, 4096)):
        assert wb(*bad) == 0, bad
