"""HIP paired bootstrap (C ABI ldc_paired_bootstrap, ladcast_amd.evaluate.scorecard.paired_bootstrap and its command line) against the
float64 reference of tests/scorecard_refs.py (tests/test_scorecard_cpu.py holds that reference to a brute-force statement in exact
arithmetic, so a failure here is the kernel's).

Integer-valued cases: every sum is exact, so kind = mean must give the reference's bits and kind = root_mean at most one ulp more (both
sides round the same quotient; the square root is correctly rounded on both); counts are equal.  A NaN is compared as a NaN, whatever
its sign and payload.  Physical-scale cases: every statistic within the counted bound of scorecard_refs (sums in any order: D * 2^-53 *
sum|terms|, carried through theta; an order statistic is 1-Lipschitz in the sup norm), the sign counts equal because the builder
asserts that every |d*| exceeds its bound.

Shapes: one value; fewer replicates, series and initial times than a tile (64 x 64, 16 times per staged chunk) and more; D below, at and
above N; R = 1, 2, 5 (sort networks of 1, 2 and 8 keys), 100, 1000 and the cap.  a and b sit inside a wider buffer of finite 1e30
values, so a read outside the view changes a sum; stats, counts and the workspace sit between guard bands."""
import csv
import json
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from tests import scorecard_refs as SR
from tests.redzone import UNWRITTEN32, UNWRITTEN64, _signed, assert_untouched, guarded

pytestmark = pytest.mark.gpu

ARG, ALIGN, UNSUPPORTED = -1, -2, -3


@pytest.fixture(scope="module")
def hip():
    from ladcast_amd import hip
    return hip


@pytest.fixture(scope="module")
def SC():
    from ladcast_amd.evaluate import scorecard
    return scorecard


def _embed(x, ld=None, off=0):
    """the (N, K) array as columns off .. off + K - 1 of a device buffer (N, ld) of finite 1e30 values, with the same before and after"""
    N, K = x.shape
    ld = K if ld is None else ld
    pad = 1024
    flat = torch.full((N * ld + 2 * pad,), 1.0e30, dtype=torch.float32, device="cuda")
    body = flat[pad : pad + N * ld].view(N, ld)
    body[:, off : off + K] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return body[:, off : off + K], ld


def _buffers(hip, N, K, R, D, ws_bytes=None):
    nbytes = hip.paired_bootstrap_workspace_bytes(N, K, R, D) if ws_bytes is None else ws_bytes
    return (guarded(K, 8, dtype=torch.float64), guarded(K, 4, dtype=torch.int32), guarded(1, max(nbytes // 4, 4), dtype=torch.float32, align_bytes=16), nbytes)


def _run(hip, a, b, draws, kind, ppm=25000, ld=None, off=0):
    """one ldc_paired_bootstrap call between guard bands -> stats (K, 8), counts (K, 4) on the host"""
    N, K = a.shape
    R, D = draws.shape
    av, ld = _embed(a, ld, off)
    bv, _ = _embed(b, ld, off)
    dr = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.int32)).cuda()
    S, Cn, W, nbytes = _buffers(hip, N, K, R, D)
    assert nbytes > 0
    st = hip.lib.ldc_paired_bootstrap(hip._p(av), hip._p(bv), ld, N, K, hip._p(dr), R, D, kind, ppm, hip._p(S.t), hip._p(Cn.t), hip._p(W.t), nbytes,
                                      hip._stream())
    torch.cuda.synchronize()
    assert st == 0, st
    for buf, what in ((S, "stats"), (Cn, "counts"), (W, "workspace")):
        assert_untouched(buf, what)
    stats, counts = S.payload().reshape(K, 8).numpy(), Cn.payload().reshape(K, 4).numpy()
    assert not (stats.view(np.int64) == _signed(UNWRITTEN64, 64)).any() and not (counts == _signed(UNWRITTEN32, 32)).any()
    return stats, counts


def _assert_same(got, want, kind, what):
    """stats against the reference on exact sums: NaN where the reference has NaN; the same bits (mean) / within one ulp (root mean)"""
    (gs, gc), (ws, wc) = got, want
    assert np.array_equal(gc, wc), (what, "counts", gc, wc)
    assert np.array_equal(np.isnan(gs), np.isnan(ws)), (what, "NaN pattern", gs, ws)
    g, w = np.where(np.isnan(gs), 0.0, gs), np.where(np.isnan(ws), 0.0, ws)  # +-inf stay what they are
    if kind == 0:
        assert np.array_equal(g.view(np.int64), w.view(np.int64)), (what, g, w)
    else:
        fin = np.isfinite(w)
        assert np.array_equal(g[~fin], w[~fin]) and (np.abs(g[fin] - w[fin]) <= np.spacing(np.abs(w[fin]))).all(), (what, g, w)


# (N, K, R, D): N in {1, 2, 7, 64}, K in {1, 3, 65, 130}, R in {1, 2, 5, 100, 1000}, D in {N, N - 1, 2 N + 3}
INTEGER_SHAPES = [(1, 1, 1, 1), (1, 3, 5, 5), (2, 3, 2, 1), (2, 1, 5, 7), (2, 130, 100, 2), (7, 65, 100, 7), (7, 3, 1000, 17), (7, 130, 5, 6),
                  (64, 65, 100, 64), (64, 130, 2, 131), (64, 3, 1000, 63), (64, 1, 1, 64)]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", INTEGER_SHAPES)
def test_integer_cases_match_the_reference(hip, shape, kind):
    N, K, R, D = shape
    a, b, draws = (SR.positive_integer_case if kind else SR.integer_case)(100 + N + K, N, K, R, D)
    for ppm in (25000, 0, 499999) if R == 100 else (25000,):
        _assert_same(_run(hip, a, b, draws, kind, ppm), SR.paired_bootstrap_ref(a, b, draws, kind, ppm), kind, (shape, kind, ppm))


def test_the_cap_on_replicates(hip):
    cap = hip.lib.ldc_paired_bootstrap_max_replicates()
    assert cap >= 10000
    a, b, draws = SR.integer_case(7, 8, 2, cap, 8)
    got = _run(hip, a, b, draws, 0)
    _assert_same(got, SR.paired_bootstrap_ref(a, b, draws, 0, 25000), 0, "cap")
    assert (got[1][:, 1] == cap).all()
    # one more is refused, and nothing is launched
    more = np.concatenate([draws, draws[:1]])
    assert hip.paired_bootstrap_workspace_bytes(8, 2, cap + 1, 8) == 0
    av, ld = _embed(a)
    bv, _ = _embed(b)
    dr = torch.from_numpy(more).cuda()
    S, Cn, W, nbytes = _buffers(hip, 8, 2, cap, 8)
    st = hip.lib.ldc_paired_bootstrap(hip._p(av), hip._p(bv), ld, 8, 2, hip._p(dr), cap + 1, 8, 0, 25000, hip._p(S.t), hip._p(Cn.t), hip._p(W.t), nbytes,
                                      hip._stream())
    torch.cuda.synchronize()
    assert st == UNSUPPORTED
    _assert_nothing_written(S, Cn, W)


def _assert_nothing_written(S, Cn, W):
    for buf, what in ((S, "stats"), (Cn, "counts"), (W, "workspace")):
        assert_untouched(buf, what)
    assert bool((S.payload().view(torch.int64) == _signed(UNWRITTEN64, 64)).all()) and bool((Cn.payload() == _signed(UNWRITTEN32, 32)).all())
    assert bool((W.payload().view(torch.int32) == _signed(UNWRITTEN32, 32)).all())


@pytest.mark.parametrize("spread", [0.0, 16.0])
@pytest.mark.parametrize("kind", [0, 1])
def test_physical_scale_within_the_counted_bound(hip, kind, spread):
    """97 initial times (six staged chunks and a ragged seventh), 70 series (a whole tile and a ragged one), 130 replicates (two tiles and a ragged
    one).  spread 0: CRPS-like scores; a sum of 97 fp32 values of one magnitude is exact in fp64, so the error is 0.  spread 16: every score
    times e^u, u uniform in [-16, 16]: 46 binades inside a series, so the sums do round and their order matters"""
    N, K, R = 97, 70, 130
    a, b, draws, (ws, wc, bounds) = SR.physical_case(11 + kind, N, K, R, kind, spread=spread)
    gs, gc = _run(hip, a, b, draws, kind)
    assert np.array_equal(gc, wc) and (gc[:, 0] == N).all() and (gc[:, 1] == R).all()
    bound = np.concatenate([bounds["hat"], np.repeat(bounds["diff"][:, None], 2, axis=1), np.repeat(bounds["ratio"][:, None], 2, axis=1)], axis=1)
    err = np.abs(gs - ws)
    ratio = err / bound
    print(f"\npaired bootstrap, physical scale, kind {kind}, spread {spread}: worst |stat - ref| / bound = {ratio.max():.3g} (field {SR.STAT_FIELDS[int(ratio.max(axis=0).argmax())]}), "
          f"smallest |d*| / bound = {bounds['margin']:.3g}")
    assert np.isfinite(gs).all() and (err <= bound).all(), ratio.max()
    assert (gs[:, 4] <= gs[:, 5]).all() and (gs[:, 6] <= gs[:, 7]).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_the_validity_table(hip, kind):
    N, K, R, D = 8, 8, 6, 8
    rng = np.random.default_rng(5)
    a = rng.integers(1, 9, size=(N, K)).astype(np.float32)
    b = np.maximum(1, a + rng.integers(-2, 3, size=(N, K))).astype(np.float32)
    a[:, 0] = b[:, 0] = np.nan            # 0: no valid pair at all
    a[[1, 5], 1] = np.nan                 # 1: NaN only in a
    b[[0, 2, 7], 2] = np.nan              # 2: NaN only in b
    a[3, 3], b[6, 3] = np.inf, -np.inf    # 3: +-inf are invalid too
    a[:4, 4] = np.nan                     # 4: rows 0 .. 3 invalid, and replicate 0 draws only those
    a[:, 5] = [1, -1, 2, -2, 3, -3, 1, -1]  # 5: a_hat == 0
    a[:, 6] = -np.abs(a[:, 6])            # 6: a negative mean (NaN under root_mean)
    draws = rng.integers(0, N, size=(R, D)).astype(np.int32)
    draws[0] = [0, 1, 2, 3, 3, 2, 1, 0]
    draws[1:, 0] = 4 + np.arange(R - 1) % 4
    want = SR.paired_bootstrap_ref(a, b, draws, kind, 25000)
    gs, gc = got = _run(hip, a, b, draws, kind)
    _assert_same(got, want, kind, ("validity", kind))
    assert gc[0].tolist() == [0, 0, 0, 0] and np.isnan(gs[0]).all()
    assert gc[1, 0] == 6 and gc[2, 0] == 5 and gc[3, 0] == 6
    assert gc[4, 0] == 4 and gc[4, 1] == R - 1 and np.isfinite(gs[4]).all()
    assert (gc[[1, 2, 3, 7], 1] == R).all()
    if kind == 0:
        assert gs[5, 0] == 0.0 and not np.isfinite(gs[5, 3]) and np.isfinite(gs[5, [1, 2, 4, 5]]).all() and gc[5, 1] == R
        assert np.isfinite(gs[6]).all()
    else:
        assert np.isnan(gs[6, [0, 2, 3, 4, 5, 6, 7]]).all() and np.isfinite(gs[6, 1]) and gc[6].tolist() == [N, 0, 0, 0]


def test_a_series_has_the_same_bits_alone_in_a_wider_array_and_through_the_wrapper(hip, SC):
    N, K, R = 23, 130, 70
    a, b, draws, _ = SR.physical_case(21, N, K, R, 0, spread=16.0)  # sums that round: their order would show
    a[3, 64] = np.nan
    full = _run(hip, a, b, draws, 0)
    again = _run(hip, a, b, draws, 0)
    assert np.array_equal(full[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(full[1], again[1])
    wide = _run(hip, a, b, draws, 0, ld=K + 37, off=5)
    assert np.array_equal(full[0].view(np.int64), wide[0].view(np.int64)) and np.array_equal(full[1], wide[1])
    for k in (0, 64, 129):
        one = _run(hip, a[:, k : k + 1], b[:, k : k + 1], draws, 0, ld=K, off=k)
        assert np.array_equal(one[0].view(np.int64), full[0][k : k + 1].view(np.int64)) and np.array_equal(one[1], full[1][k : k + 1]), k
    # the wrapper: four chunks of at most 41 series, columns of the same arrays
    one = hip.paired_bootstrap_workspace_bytes(N, 1, R, N)
    per = hip.paired_bootstrap_workspace_bytes(N, 2, R, N) - one
    at, bt = torch.from_numpy(a).cuda().reshape(N, 10, 13), torch.from_numpy(b).cuda().reshape(N, 10, 13)
    for limit in (one + 40 * per, 256 << 20):
        res = SC.paired_bootstrap(at, bt, draws, kind="mean", alpha=0.05, max_workspace_bytes=limit)
        for i, f in enumerate(SR.STAT_FIELDS):
            assert res[f].shape == (10, 13) and np.array_equal(res[f].reshape(-1).view(np.int64), full[0][:, i].view(np.int64)), (limit, f)
        for i, f in enumerate(SR.COUNT_FIELDS):
            assert res[f].dtype == np.int32 and np.array_equal(res[f].reshape(-1), full[1][:, i]), (limit, f)
        assert np.array_equal(res["p_value"].reshape(-1), SC.p_value_from_counts(full[1]))
    assert full[1][64, 0] == N - 1
    for bad in (lambda: SC.paired_bootstrap(at, bt, draws, max_workspace_bytes=one - 1), lambda: SC.paired_bootstrap(at, bt[:-1], draws),
                lambda: SC.paired_bootstrap(at, bt, draws + 1), lambda: SC.paired_bootstrap(at, bt, draws - 1), lambda: SC.paired_bootstrap(at, bt, draws, kind="median"),
                lambda: SC.paired_bootstrap(at, bt, draws, alpha=1.0), lambda: SC.paired_bootstrap(at, bt, draws.astype(np.float32))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        SC.paired_bootstrap(at.cpu(), bt.cpu(), draws)


def test_refused_arguments_launch_nothing(hip):
    N, K, R, D = 7, 5, 9, 7
    a, b, draws = SR.integer_case(1, N, K, R, D)
    av, ld = _embed(a)
    bv, _ = _embed(b)
    dr = torch.from_numpy(draws).cuda()
    S, Cn, W, nb = _buffers(hip, N, K, R, D)
    f = hip.lib.ldc_paired_bootstrap
    A, B, Dp, Sp, Cp, Wp, st = hip._p(av), hip._p(bv), hip._p(dr), hip._p(S.t), hip._p(Cn.t), hip._p(W.t), hip._stream()
    assert f(None, B, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, None, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, None, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, None, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, Sp, None, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, None, nb, st) == ARG
    assert f(A, B, ld, 0, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, 0, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, 0, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, 0, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, -1, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, K - 1, N, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 2, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, -1, 25000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, -1, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, 500000, Sp, Cp, Wp, nb, st) == ARG
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb - 1, st) == ARG
    assert f(A, B, ld, N, K, Dp, hip.lib.ldc_paired_bootstrap_max_replicates() + 1, D, 0, 25000, Sp, Cp, Wp, nb, st) == UNSUPPORTED
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, c_void_p(S.t.data_ptr() + 4), Cp, Wp, nb, st) == ALIGN
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, c_void_p(W.t.data_ptr() + 8), nb, st) == ALIGN
    for sizes in ((0, K, R, D), (N, 0, R, D), (N, K, 0, D), (N, K, R, 0), (N, K, hip.lib.ldc_paired_bootstrap_max_replicates() + 1, D)):
        assert hip.paired_bootstrap_workspace_bytes(*sizes) == 0
    torch.cuda.synchronize()
    _assert_nothing_written(S, Cn, W)
    assert f(A, B, ld, N, K, Dp, R, D, 0, 25000, Sp, Cp, Wp, nb, st) == 0  # and the same buffers are served once the arguments are right
    torch.cuda.synchronize()
    for buf, what in ((S, "stats"), (Cn, "counts"), (W, "workspace")):
        assert_untouched(buf, what)
    _assert_same((S.payload().reshape(K, 8).numpy(), Cn.payload().reshape(K, 4).numpy()), SR.paired_bootstrap_ref(a, b, draws, 0, 25000), 0, "after the refusals")
    with pytest.raises(RuntimeError):
        hip.paired_bootstrap(av.cpu(), bv, dr, S.t, Cn.t, N=N, K=K, ld=ld, R=R, D=D, kind=0, tail_ppm=25000)


def test_command_line_equals_the_reference_on_the_same_draws(hip, SC, tmp_path):
    """integer-valued scores (every sum exact) in two directories that share 9 of their 11 initial times"""
    C, L = 3, 4
    times = [2018123100 + 6 * h for h in range(4)] + [2019010100 + 6 * h for h in range(4)] + [2019010200 + 6 * h for h in range(3)]
    rng = np.random.default_rng(31)
    base = {k: rng.integers(1, 60, size=(len(times), C, L)).astype(np.float32) for k in ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")}
    other = {k: np.maximum(1, v + rng.integers(-3, 4, size=v.shape)).astype(np.float32) for k, v in base.items()}
    base["crps"][4, 1, 2] = np.nan  # one missing score
    SR.write_score_dir(tmp_path / "a", times[:10], {k: v[:10] for k, v in base.items()})
    SR.write_score_dir(tmp_path / "b", times[1:], {k: v[1:] for k, v in other.items()})
    argv = ["--a", str(tmp_path / "a"), "--b", str(tmp_path / "b"), "--n_boot", "200", "--block", "3", "--seed", "3", "--rmse_of", "ens_mse", "--leads", "1", "4"]
    got = SC.main(argv + ["--output", str(tmp_path / "gpu")])
    want = SC.main(argv + ["--output", str(tmp_path / "ref")], bootstrap=SR.reference_bootstrap)
    assert sorted(got) == sorted(want) and len(got) == 6 * 13
    for k in want:
        kind = 1 if k.startswith("ens_mse_rmse") else 0
        if any(k.endswith(f) for f in SR.COUNT_FIELDS):
            assert np.array_equal(got[k], want[k]), k
        elif k.endswith("p_value"):
            assert np.array_equal(got[k], want[k], equal_nan=True), k
        else:
            g, w = np.asarray(got[k]), np.asarray(want[k])
            assert np.array_equal(np.isnan(g), np.isnan(w)), k
            g, w = np.where(np.isnan(g), 0.0, g), np.where(np.isnan(w), 0.0, w)
            assert np.isfinite(w).all() and (np.array_equal(g, w) if kind == 0 else (np.abs(g - w) <= np.spacing(np.abs(w))).all()), k
    assert got["crps_n_valid"][1, 2] == 8 and got["crps_n_valid"][0, 0] == 9
    meta = json.load(open(tmp_path / "gpu" / "scorecard.json"))
    assert meta["common_times"] == times[1:10] and meta["only_a"] == times[:1] and meta["only_b"] == times[10:]
    rows_g, rows_r = (list(csv.reader(open(tmp_path / d / "scorecard.csv"))) for d in ("gpu", "ref"))
    assert len(rows_g) == 1 + 6 * C * 2 and [r[:3] + r[9:] for r in rows_g] == [r[:3] + r[9:] for r in rows_r]  # the same verdicts
