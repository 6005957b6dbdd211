"""Host side of the scorecard (ladcast_amd.evaluate.scorecard): the float64 reference of tests/scorecard_refs.py against a second,
brute-force statement of the definitions in exact rational arithmetic, the block-bootstrap table, the pairing of two score directories
and the command line with `bootstrap=` set to the reference.  Nothing here needs a GPU."""
import csv
import json
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import scorecard_refs as SR


@pytest.fixture(scope="module")
def SC():
    from ladcast_amd.evaluate import scorecard
    return scorecard


# ---- the reference against a brute-force statement -----------------------------------------------------------------------------------
def _brute(a, b, draws, kind, tail_ppm):
    """per series and replicate in plain Python: exact rational sums, one rounding to double, then the definitions word by word"""
    N, K = a.shape

    def th(S, m):
        mean = float(S) / float(m)  # S is exactly representable in every case this is used on
        return (math.sqrt(mean) if mean >= 0 else math.nan) if kind == 1 else mean

    def div(x, y):
        if y == 0:
            return math.nan if (x == 0 or math.isnan(x)) else math.copysign(math.inf, x) * math.copysign(1.0, y)
        return x / y

    def pick(vals):
        vals = sorted(vals, key=lambda v: (v, not math.copysign(1.0, v) < 0))
        if not vals:
            return math.nan, math.nan
        lo = (tail_ppm * len(vals)) // 1000000
        return vals[lo], vals[len(vals) - 1 - lo]

    stats, counts = np.full((K, 8), np.nan), np.zeros((K, 4), dtype=np.int32)
    for k in range(K):
        ok = [bool(np.isfinite(a[i, k]) and np.isfinite(b[i, k])) for i in range(N)]

        def sums(idx):
            idx = [i for i in idx if ok[i]]
            return sum((Fraction(float(a[i, k])) for i in idx), Fraction(0)), sum((Fraction(float(b[i, k])) for i in idx), Fraction(0)), len(idx)

        SA, SB, m = sums(range(N))
        counts[k, 0] = m
        if m:
            ah, bh = th(SA, m), th(SB, m)
            stats[k, :4] = ah, bh, bh - ah, div(bh, ah)
        ds, qs = [], []
        for row in draws:
            SA, SB, m = sums(int(i) for i in row)
            if m == 0:
                continue
            ar, br = th(SA, m), th(SB, m)
            if math.isfinite(br - ar):
                ds.append(br - ar)
            if math.isfinite(div(br, ar)):
                qs.append(div(br, ar))
        counts[k, 1:] = len(ds), sum(v <= 0 for v in ds), sum(v >= 0 for v in ds)
        stats[k, 4:6] = pick(ds)
        stats[k, 6:8] = pick(qs)
    return stats, counts


def _same(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.int64), np.asarray(y, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 3, 5, 2), (7, 4, 40, 7), (7, 3, 33, 17), (5, 2, 9, 4)])
def test_reference_matches_the_brute_force_statement(shape, kind):
    N, K, R, D = shape
    a, b, draws = (SR.positive_integer_case if kind else SR.integer_case)(3 + N, N, K, R, D)
    if N >= 5:  # invalid pairs, a replicate that draws only those, and a series with a_hat == 0
        a[0, 0], b[1, 0] = np.nan, np.inf
        draws[0] = np.resize(np.array([0, 1], dtype=np.int32), D)
        if kind == 0:
            a[:, 1] = np.resize(np.array([1.0, -1.0], dtype=np.float32), N) * (np.arange(N) < N - N % 2)
    for ppm in (0, 25000, 499999):
        want = _brute(a, b, draws, kind, ppm)
        got = SR.paired_bootstrap_ref(a, b, draws, kind, ppm)
        assert np.array_equal(got[1], want[1]), (shape, kind, ppm)
        assert _same(np.nan_to_num(got[0], nan=-1e300), np.nan_to_num(want[0], nan=-1e300)), (shape, kind, ppm, got[0], want[0])
        assert np.array_equal(np.isnan(got[0]), np.isnan(want[0]))
    if N >= 5:
        hits_valid = sum(bool((row > 1).any()) for row in draws)  # replicates with a valid draw of series 0
        assert got[1][0, 0] == N - 2 and got[1][0, 1] == hits_valid <= R - 1
        if kind == 0:
            assert got[0][1, 0] == 0.0 and not np.isfinite(got[0][1, 3]) and np.isfinite(got[0][1, 2])


def test_reference_on_identical_and_shifted_runs(SC):
    a, _, draws = SR.integer_case(5, 8, 3, 50, 8)  # eight draws: every mean of integers is exact
    stats, counts = SR.paired_bootstrap_ref(a, a, draws, 0, 25000)
    assert (stats[:, 2] == 0).all() and (stats[:, 4] == 0).all() and (stats[:, 5] == 0).all()
    assert (counts[:, 1] == 50).all() and (counts[:, 2] == 50).all() and (counts[:, 3] == 50).all()
    assert (SC.p_value_from_counts(counts) == 1.0).all()
    for c in (3.0, -2.0):
        stats, counts = SR.paired_bootstrap_ref(a, a + np.float32(c), draws, 0, 25000)
        assert (stats[:, 2] == c).all() and (stats[:, 4] == c).all() and (stats[:, 5] == c).all()
        assert (counts[:, 2] == (50 if c < 0 else 0)).all() and (counts[:, 3] == (0 if c < 0 else 50)).all()
        assert np.allclose(SC.p_value_from_counts(counts), 2.0 / 51.0, rtol=1e-15)
    # the bound is a bound: float64 sums in another order stay inside it
    a, b, draws, (stats, counts, bounds) = SR.physical_case(2, 40, 3, 30, 1)
    W = np.stack([np.bincount(r, minlength=40) for r in draws]).astype(np.float64)
    d = np.sqrt(W @ b.astype(np.float64) / 40) - np.sqrt(W @ a.astype(np.float64) / 40)
    lo, hi = SR.ranks(30, 25000)
    assert (np.abs(np.sort(d, axis=0)[lo] - stats[:, 4]) <= bounds["diff"]).all() and (bounds["diff"] < 1e-12 * np.abs(stats[:, 0])).all()


def test_ranks_are_integer_arithmetic():
    assert SR.ranks(10000, 25000) == (250, 9749) and SR.ranks(1, 25000) == (0, 0) and SR.ranks(39, 25000) == (0, 38) and SR.ranks(40, 25000) == (1, 38)
    assert SR.ranks(9999, 499999) == (4999, 4999) and SR.ranks(10000, 0) == (0, 9999)


# ---- block_bootstrap_draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,block", [(10, 1), (10, 10), (10, 3), (17, 8), (1, 1), (64, 8)])
def test_block_bootstrap_draws_are_blocks_of_consecutive_times(SC, n, block):
    d = SC.block_bootstrap_draws(n, 25, block, seed=4)
    assert d.shape == (25, n) and d.dtype == np.int32 and d.flags.c_contiguous and d.min() >= 0 and d.max() < n
    for row in d:
        for s in range(0, n, block):
            run = row[s : s + block].astype(np.int64)  # the last run is truncated
            assert ((run - run[0]) % n == np.arange(len(run))).all(), (row, s)
    assert np.array_equal(d, SC.block_bootstrap_draws(n, 25, block, seed=4))
    if n > 1:
        assert not np.array_equal(d, SC.block_bootstrap_draws(n, 25, block, seed=5))
        starts = SC.block_bootstrap_draws(n, 400, block, seed=6)[:, ::block]
        assert set(np.unique(starts)) == set(range(n))  # every start occurs, the wrap-around ones too


def test_block_bootstrap_draws_refuses_bad_sizes(SC):
    for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 6)):
        with pytest.raises(ValueError):
            SC.block_bootstrap_draws(*bad, seed=0)
    with pytest.raises(ValueError):
        SC.tail_ppm_of(1.0)
    assert SC.tail_ppm_of(0.05) == 25000 and SC.tail_ppm_of(0.1) == 50000


# ---- pair_score_dirs ---------------------------------------------------------------------------------------------------------------
C, L = 3, 5
TIMES = [2018123100, 2018123106, 2018123112, 2018123118, 2019010100, 2019010106, 2019010112, 2019010118, 2019010200, 2019010206]


def _scores(seed, times, shift=0.0):
    """five reference score arrays (len(times), C, L): a function of the TIME, so that pairing mistakes show; crps of run B a touch larger"""
    out = {}
    for j, name in enumerate(("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")):
        x = np.empty((len(times), C, L), dtype=np.float32)
        for i, t in enumerate(times):
            rng = np.random.default_rng([seed, j, t])
            x[i] = rng.gamma(4.0, 0.25, size=(C, L)) * (1.0 + (shift if name in ("crps", "ens_mse") else -shift if name == "ens_acc" else 0.0))
        out[name] = x
    return out


def test_pair_score_dirs(SC, tmp_path):
    assert np.float32(2018123118) == np.float32(2018123112)  # the collision the per-time file names resolve
    SR.write_score_dir(tmp_path / "a", TIMES[:7], _scores(1, TIMES[:7]))
    SR.write_score_dir(tmp_path / "b", TIMES[2:][::-1], _scores(2, TIMES[2:][::-1]))  # written in another order: stacked ascending all the same
    SR.write_score_dir(tmp_path / "c", TIMES[8:], _scores(3, TIMES[8:]))
    times, ia, ib, only_a, only_b = SC.pair_score_dirs(str(tmp_path / "a"), str(tmp_path / "b"))
    assert times == TIMES[2:7] and ia.tolist() == [2, 3, 4, 5, 6] and ib.tolist() == [0, 1, 2, 3, 4]
    assert only_a == TIMES[:2] and only_b == TIMES[7:]
    assert 2018123112 in times and 2018123118 in times
    # the rows named are the rows of those times
    for d, idx in (("a", ia), ("b", ib)):
        stacked = np.load(tmp_path / d / "crps.npy")
        for t, i in zip(times, idx):
            assert np.array_equal(stacked[i], np.load(tmp_path / d / f"{t}_crps.npy"))
    times, ia, ib, only_a, only_b = SC.pair_score_dirs(str(tmp_path / "a"), str(tmp_path / "c"))
    assert times == [] and len(ia) == 0 and len(ib) == 0 and only_a == TIMES[:7] and only_b == TIMES[8:]
    # a stacked array that is one initial time short, a timestamp that names another time, a directory without per-time files
    np.save(tmp_path / "c" / "crps.npy", np.load(tmp_path / "c" / "crps.npy")[:1])
    with pytest.raises(ValueError, match="crps.npy"):
        SC.pair_score_dirs(str(tmp_path / "a"), str(tmp_path / "c"))
    stamp = np.load(tmp_path / "b" / "timestamp.npy")
    stamp[3] = np.float32(2019010300)
    np.save(tmp_path / "b" / "timestamp.npy", stamp)
    with pytest.raises(ValueError, match="timestamp.npy"):
        SC.pair_score_dirs(str(tmp_path / "a"), str(tmp_path / "b"))
    (tmp_path / "e").mkdir()
    with pytest.raises(ValueError):
        SC.pair_score_dirs(str(tmp_path / "a"), str(tmp_path / "e"))


# ---- the command line ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cards")
    ta, tb = TIMES[:9], TIMES[1:]
    a = _scores(1, ta)
    b = {k: v.copy() for k, v in _scores(1, tb, shift=0.02).items()}  # the same forecast, 2 % worse on crps / ens_mse / ens_acc
    b["crps"][:, 2, :] = _scores(1, tb)["crps"][:, 2, :]  # but channel 2 of crps: identical
    a["energy"] = a["crps"].astype(np.float64) * (1 + 2.0 ** -30)  # a float64 file whose values are no fp32 numbers
    b["energy"] = b["crps"].astype(np.float64)
    a["only_in_a"] = a["crps"]
    SR.write_score_dir(d / "a", ta, a)
    SR.write_score_dir(d / "b", tb, b)
    return d, a, b, ta, tb


def test_command_line_with_the_reference_bootstrap(SC, two_dirs):
    d, a, b, ta, tb = two_dirs
    calls = []

    def boot(xa, xb, draws, kind, alpha):
        calls.append((xa.copy(), xb.copy(), draws.copy(), kind, alpha))
        return SR.reference_bootstrap(xa, xb, draws, kind, alpha)

    names = d / "names.json"
    names.write_text(json.dumps(["z500", "t850", "sst"]))
    out = SC.main(["--a", str(d / "a"), "--b", str(d / "b"), "--output", str(d / "card"), "--n_boot", "60", "--block", "3", "--seed", "7", "--rmse_of", "ens_mse",
                   "--leads", "1", "5", "--channel_names_json", str(names)], bootstrap=boot)
    common = TIMES[1:9]
    assert len(calls) == 6 and [c[3] for c in calls] == ["mean"] * 5 + ["root_mean"]
    draws = SC.block_bootstrap_draws(8, 60, 3, 7)
    for c in calls:
        assert c[0].shape == (8, C, L) and c[0].dtype == np.float32 and np.array_equal(c[2], draws) and c[4] == 0.05
    assert np.array_equal(calls[4][0], a["crps"][1:9]) and np.array_equal(calls[4][1], b["crps"][:8])  # crps is the fifth reference score
    saved = np.load(d / "card" / "scorecard.npz")
    fields = SR.STAT_FIELDS + SR.COUNT_FIELDS + ("p_value",)
    metrics = ["ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps", "ens_mse_rmse"]
    assert sorted(saved.files) == sorted(f"{m}_{f}" for m in metrics for f in fields)
    for k in saved.files:
        assert saved[k].shape == (C, L) and np.array_equal(saved[k], out[k], equal_nan=True)
    assert saved["crps_a_hat"].dtype == np.float64 and saved["crps_n_valid"].dtype == np.int32 and (saved["crps_n_valid"] == 8).all()
    assert np.allclose(saved["ens_mse_rmse_a_hat"], np.sqrt(saved["ens_mse_a_hat"]), rtol=1e-15)
    assert np.allclose(saved["crps_ratio_hat"][:2], 1.02, rtol=1e-6) and (saved["crps_diff_hat"][2] == 0).all()
    meta = json.load(open(d / "card" / "scorecard.json"))
    assert meta["common_times"] == common and meta["only_a"] == [TIMES[0]] and meta["only_b"] == [TIMES[9]] and meta["n_common"] == 8
    assert (meta["n_boot"], meta["block"], meta["alpha"], meta["seed"]) == (60, 3, 0.05, 7)
    assert meta["direction"]["ens_acc"] == "higher_is_better" and meta["direction"]["crps"] == "lower_is_better" and meta["kinds"]["ens_mse_rmse"] == "root_mean"
    rows = list(csv.DictReader(open(d / "card" / "scorecard.csv")))
    assert len(rows) == 6 * C * 2 and set(r["lead"] for r in rows) == {"1", "5"} and set(r["channel"] for r in rows) == {"z500", "t850", "sst"}
    by = {(r["metric"], r["channel"], r["lead"]): r for r in rows}
    # b = 1.02 a exactly up to fp32 rounding: every replicate's difference has one sign
    assert by[("crps", "z500", "1")]["verdict"] == "worse" and by[("ens_mse_rmse", "t850", "5")]["verdict"] == "worse"
    assert by[("ens_acc", "z500", "1")]["verdict"] == "worse"  # smaller, and higher is better
    assert by[("crps", "sst", "5")]["verdict"] == "neutral" and float(by[("crps", "sst", "5")]["change_pct"]) == 0.0 and float(by[("crps", "sst", "5")]["p_value"]) == 1.0
    assert abs(float(by[("crps", "z500", "1")]["change_pct"]) - 2.0) < 1e-3 and float(by[("crps", "z500", "1")]["change_lo_pct"]) <= float(by[("crps", "z500", "1")]["change_hi_pct"])
    assert float(by[("crps", "z500", "1")]["a"]) == float(saved["crps_a_hat"][0, 0])
    assert abs(float(by[("crps", "z500", "1")]["p_value"]) - 2.0 / 61.0) < 1e-6


def test_command_line_directions_metrics_and_errors(SC, two_dirs):
    d, a, b, ta, tb = two_dirs
    args = ["--a", str(d / "a"), "--b", str(d / "b"), "--n_boot", "20", "--block", "2"]
    out = SC.main(args + ["--output", str(d / "card2"), "--metrics", "crps", "energy", "--higher_is_better", "crps"], bootstrap=SR.reference_bootstrap)
    rows = list(csv.DictReader(open(d / "card2" / "scorecard.csv")))
    assert len(rows) == 2 * C * L and set(r["channel"] for r in rows) == {"0", "1", "2"}
    by = {(r["metric"], r["channel"], r["lead"]): r["verdict"] for r in rows}
    assert by[("crps", "0", "1")] == "better" and by[("energy", "0", "1")] == "worse"
    # the float64 file was rounded to fp32 on load: run A's energy is run A's crps again
    assert np.array_equal(out["energy_a_hat"], out["crps_a_hat"]) and np.array_equal(out["energy_diff_lo"], out["crps_diff_lo"])
    with pytest.raises(FileNotFoundError, match="only_in_a"):
        SC.main(args + ["--output", str(d / "card3"), "--metrics", "crps", "only_in_a"], bootstrap=SR.reference_bootstrap)
    with pytest.raises(ValueError, match="leads"):
        SC.main(args + ["--output", str(d / "card3"), "--metrics", "crps", "--leads", "6"], bootstrap=SR.reference_bootstrap)
    with pytest.raises(ValueError, match="block"):
        SC.main(args[:4] + ["--output", str(d / "card3"), "--block", "9"], bootstrap=SR.reference_bootstrap)
    assert SC.verdict(float("nan"), float("nan"), False) == "neutral" and SC.verdict(-2.0, -1.0, False) == "better" and SC.verdict(-2.0, 0.0, False) == "neutral"
