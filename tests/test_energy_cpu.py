"""Host side of the energy score (csrc/energy.hip, ladcast_amd.evaluate.energy, the --energy flags of evaluate_ens_gpu).  No GPU:
  a. an fp32 restatement of the kernel's arithmetic that adds in ANOTHER order (tests/energy_refs.py) meets the oracle's counted bounds
     at every case - the bounds are not met by the oracle alone - and every planted defect fails at least one case
  b. the identities of the score in float64: one point is the CRPS, one member, a perfect ensemble, a group of one channel, and the
     shuffle of the members point by point that no pointwise score sees
  c. rollout_energy and score_latent_rollout raise ValueError for bad groups, scales and arguments without touching a device
  d. --energy / --energy_group: parsing, and the command line's file handling with an injected scorer
  e. the library's exports"""
import json

import numpy as np
import pytest
import torch

from tests import energy_refs as R


def _ref(c, groups=(), scales=None):
    return R.energy_ref(c["x"], c["t"], c["w"], groups, scales)


# ---- a. the restatement against the oracle -----------------------------------------------------------------------------------------------
def test_restatement_in_another_order_meets_every_bound():
    worst = 0.0
    for name, c, groups, scales in R.cpu_cases():
        got, ref = R.kernel_f32(c["v"], c["t"], c["w"], c["norm"], groups, scales), _ref(c, groups, scales)
        r = R.check(got, ref, name)
        print(f"{name}: worst err / bound {r:.4f}")
        worst = max(worst, r)
        if name.startswith("integer"):
            assert R.same_bits(got["dist2"], ref["dist2"][0]) and R.same_bits(got["energy"][4], ref["energy"][0][4]), f"{name}: D2 and Wv are exact"
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    caught = []
    for name, c, groups, scales in R.cpu_cases():
        got = R.kernel_f32(c["v"], c["t"], c["w"], c["norm"], groups, scales, defect=defect)
        if not R.passes(got, _ref(c, groups, scales)):
            caught.append(name)
    assert caught, f"defect {defect!r} passes every case: the tables have no teeth"
    print(defect, "caught by", caught)


def test_case_tables_cover_the_kernel_paths():
    geo = {M: R.geometry(M) for M in R.INT_M}
    assert [geo[M]["SL"] for M in R.INT_M] == [32, 32, 32, 16, 1, 1, 1, 1, 1]  # point slices: many, a few, one
    assert [geo[M]["NGRP"] for M in R.INT_M] == [1, 1, 1, 1, 1, 1, 1, 2, 9] and geo[87]["NBP"] == 253 and geo[88]["NBP"] == 276  # block groups
    assert geo[64]["NB"] == 17 and geo[65]["NB"] == 17 and geo[3]["N"] % 4 == 0 and geo[17]["N"] % 4 == 2  # full and ragged last blocks
    pts = sorted({H * W for _, H, W in R.INT_CASES})
    assert {1, 15, R.PT - 1, R.PT, R.PT + 1, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1} <= set(pts)
    assert any(W % 2 for _, _, W in R.INT_CASES) and max(H * W for M, H, W in R.INT_CASES if M == 256) < 400
    assert R.workspace_bytes(50, 84, 4, 120 * 240) == 84 * 4 * (9 * 91 * 128 + 8 * 8 + 8 + 8 * 4)
    c = R.nan_table_case()
    ref = _ref(c)
    assert ref["n_invalid"].tolist() == [0, 4, 4, 80, 0, 0]
    e = ref["energy"][0]
    assert bool(torch.isfinite(e[:, :3]).all()) and bool(torch.isnan(e[:4, 3]).all()) and float(e[4, 3]) == 0.0
    g = R.group_case()
    assert 0 < int(g["land"].sum()) < g["land"].numel() and not any(2 in gr for gr in g["groups"])


# ---- b. identities in float64 --------------------------------------------------------------------------------------------------------------
def _crps_parts(x, t):
    """the reference's pointwise_crps_skill and pointwise_crps_spread (ladcast/evaluate/utils.py) in float64: x (M, ...), t (...)"""
    M = x.shape[0]
    skill = np.abs(x - t[None]).mean(0)
    xs = np.sort(x, axis=0)
    coef = (2.0 * np.arange(1, M + 1) - M - 1).reshape((-1,) + (1,) * (x.ndim - 1))
    spread = 2.0 / (M * (M - 1)) * (xs * coef).sum(0) if M > 1 else np.zeros_like(t)
    return skill, spread


def _es(x, t, w, **kw):
    """energy_ref of float64-exact inputs: x (M, C, H, W), t (C, H, W) as fp32 tensors"""
    return R.energy_ref(x, t, w, **kw)


@pytest.mark.parametrize("M", [2, 5, 20])
def test_one_valid_point_is_the_crps(M):
    g = R.gen(151 + M)
    x, t = torch.randn(M, 3, 1, 1, generator=g) * 3, torch.randn(3, 1, 1, generator=g)
    e = _es(x, t, torch.tensor([0.7]))["energy"][0]
    skill, spread = _crps_parts(x.double().numpy()[:, :, 0, 0], t.double().numpy()[:, 0, 0])
    assert np.allclose(e[1].numpy(), skill - 0.5 * spread, rtol=1e-13, atol=1e-15)  # es_fair: the weight cancels
    assert np.allclose(e[2].numpy(), skill, rtol=1e-13) and np.allclose(e[3].numpy() * M / (M - 1), spread, rtol=1e-13)
    # and with a second point that is invalid in every channel
    x2, t2 = torch.cat([x, torch.full_like(x, float("nan"))], -1), torch.cat([t, torch.zeros_like(t)], -1)
    r2 = _es(x2, t2, torch.tensor([0.7]))
    assert R.same_bits(r2["energy"][0], _es(x, t, torch.tensor([0.7]))["energy"][0]) and r2["n_invalid"].tolist() == [1, 1, 1]


def test_one_member_and_a_perfect_ensemble():
    g = R.gen(157)
    x, t, w = torch.randn(1, 2, 4, 6, generator=g), torch.randn(2, 4, 6, generator=g), R.cos_weights(4)
    e = _es(x, t, w)["energy"][0]
    assert R.same_bits(e[0], e[2]) and R.same_bits(e[1], e[2]) and float(e[3].abs().sum()) == 0.0  # es == es_fair == skill
    d = (x[0].double() - t.double()) ** 2 * w.double().view(1, -1, 1)
    assert np.allclose(e[2].numpy(), np.sqrt(d.sum((1, 2)).numpy() / (6 * w.double().sum().item())), rtol=1e-13)  # the weighted RMS error
    same = t.unsqueeze(0).repeat(7, 1, 1, 1)
    z = _es(same, t, w)
    assert float(z["energy"][0][:4].abs().sum()) == 0.0 and float(z["dist2"][0].abs().sum()) == 0.0  # exactly 0
    k = R.kernel_f32(same, t, w)
    assert float(k["energy"][:4].abs().sum()) == 0.0


def test_a_group_of_one_channel_is_the_channel_over_its_scale():
    c = R.group_case()
    s = 4.0  # a power of two: the division by s^2 is exact, so the identity holds bit for bit
    scales = torch.full((R.GROUP_C,), s)
    ref = R.energy_ref(c["x"], c["t"], c["w"], [(k,) for k in range(R.GROUP_C)], scales)
    assert R.same_bits(ref["energy_group"][0][:4], ref["energy"][0][:4] / s) and R.same_bits(ref["energy_group"][0][4], ref["energy"][0][4])
    ref3 = R.energy_ref(c["x"], c["t"], c["w"], [(1,)], torch.tensor([1.0, 3.0, 1.0, 1.0, 1.0]))  # a general scale: to rounding
    assert np.allclose(ref3["energy_group"][0][:4, 0].numpy(), ref3["energy"][0][:4, 1].numpy() / 3.0, rtol=1e-14)


def test_shuffling_members_point_by_point_keeps_every_crps_and_changes_the_energy_score():
    """The property the feature exists for: members that are smooth fields against the same marginals shuffled at every point."""
    g = R.gen(163)
    M, H, W = 8, 12, 24
    lon = torch.arange(W) * (2 * np.pi / W)
    amp, phase = torch.randn(M + 1, 1, 1, generator=g), torch.rand(M + 1, 1, 1, generator=g) * 2 * np.pi
    fields = amp * torch.sin(lon.view(1, 1, W) + phase) + 0.3 * torch.randn(M + 1, 1, 1, generator=g)  # coherent: one wave per member
    fields = fields.expand(M + 1, H, W).contiguous()
    x, t = fields[:M].unsqueeze(1), fields[M].unsqueeze(0)
    perm = torch.rand(H, W, M, generator=g).argsort(-1).permute(2, 0, 1)  # an independent permutation of the members at every point
    xs = torch.gather(x[:, 0], 0, perm).unsqueeze(1)
    w = R.cos_weights(H)
    a, b = _crps_parts(x.double().numpy(), t.double().numpy()), _crps_parts(xs.double().numpy(), t.double().numpy())
    assert np.array_equal(a[0], b[0]) or np.allclose(a[0], b[0], rtol=1e-15, atol=1e-16)  # the skill: a sum over the same values
    assert np.allclose(a[1], b[1], rtol=1e-14, atol=1e-16)  # the spread sorts them: the same values
    e, es = _es(x, t, w)["energy"][0], _es(xs, t, w)["energy"][0]
    assert abs(float(e[0, 0]) - float(es[0, 0])) > 0.05 * abs(float(e[0, 0]))  # the energy score tells them apart
    assert float(es[3, 0]) > float(e[3, 0])  # shuffled members lie further from one another as fields


# ---- c. host-side validation ---------------------------------------------------------------------------------------------------------------
_M, _C, _L, _H, _W = 2, 3, 1, 3, 8


def _call(*, forecast=None, weight=None, **kw):
    from ladcast_amd import evaluate as E

    x = torch.zeros(_M, _C, _L, _H, _W) if forecast is None else forecast
    return E.rollout_energy(x, torch.zeros(_C, _L, _H, _W), torch.ones(_H) if weight is None else weight, **kw)


def test_rollout_energy_raises_before_it_touches_a_device():
    from ladcast_amd.evaluate import EnergyGroup

    ok = torch.ones(_C)
    grp = [EnergyGroup("a", (0, 1))]
    cases = [
        (dict(forecast=torch.zeros(_M, _C, _H, _W)), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(lead_dim=1), ValueError, r"forecast must be \(ens, C, L, H, W\)"),
        (dict(forecast=torch.zeros(_M, _C, _L, _H, _W, dtype=torch.float64)), NotImplementedError, "fp32 only"),
        (dict(forecast=torch.zeros(257, _C, _L, _H, _W)), ValueError, "members"),
        (dict(weight=torch.ones(_H + 1)), ValueError, "lat_weight must have one value per latitude row"),
        (dict(mean=torch.zeros(_C)), ValueError, "mean and std go together"),
        (dict(mean=torch.zeros(_C + 1), std=torch.ones(_C + 1)), ValueError, r"mean / std must hold one value per channel \(3\)"),
        (dict(groups=grp), ValueError, "groups need scales"),
        (dict(groups=[EnergyGroup("a", ())], scales=ok), ValueError, "holds no channel"),
        (dict(groups=[EnergyGroup("a", (0, 3))], scales=ok), ValueError, "not all among"),
        (dict(groups=[EnergyGroup("a", (-1,))], scales=ok), ValueError, "not all among"),
        (dict(groups=[EnergyGroup("a", (1, 1))], scales=ok), ValueError, "named twice"),
        (dict(groups=[EnergyGroup("a", (0.5,))], scales=ok), ValueError, "indices"),
        (dict(groups=[EnergyGroup("a", (0,)), EnergyGroup("a", (1,))], scales=ok), ValueError, "names must differ"),
        (dict(groups=[EnergyGroup(str(k), (0,)) for k in range(33)], scales=ok), ValueError, "at most 32"),
        (dict(groups=[("a",)], scales=ok), ValueError, "EnergyGroup"),
        (dict(groups=grp, scales=torch.ones(_C + 1)), ValueError, "one value per channel"),
        (dict(groups=grp, scales=torch.tensor([1.0, 0.0, 1.0])), ValueError, "positive and finite"),
        (dict(groups=grp, scales=torch.tensor([1.0, -2.0, 1.0])), ValueError, "positive and finite"),
        (dict(groups=grp, scales=torch.tensor([1.0, float("inf"), 1.0])), ValueError, "positive and finite"),
        (dict(groups=grp, scales=torch.tensor([1.0, float("nan"), 1.0])), ValueError, "positive and finite"),
        (dict(l_off=-1), ValueError, "l_off"),
        (dict(out={}), ValueError, "out must be"),
    ]
    for kw, exc, match in cases:
        with pytest.raises(exc, match=match):
            _call(**kw)
    with pytest.raises(RuntimeError, match="device tensors"):  # nothing wrong but the host tensors
        _call()
    with pytest.raises(RuntimeError, match="device tensors"):
        _call(groups=[("a", (0, 2)), ("b", torch.tensor([2]))], scales=[1.0, 2.0, 3.0], return_dist2=True, mean=torch.zeros(_C), std=ok)


def test_group_words_and_scales():
    from ladcast_amd.evaluate.energy import EnergyGroup, group_words, inverse_scale2

    groups = [EnergyGroup("a", (0, 2)), EnergyGroup("b", (2,))] + [EnergyGroup(str(k), (1,)) for k in range(2, 32)]
    words = group_words(groups, 4)
    assert words.dtype == torch.int32 and (words.long() & 0xFFFFFFFF).tolist() == [1, 0xFFFFFFFC, 3, 0]  # bit 31 set: a negative int32 word
    s = inverse_scale2(torch.tensor([2.0, 0.5, 3.0], dtype=torch.float32), 3)
    assert s.dtype == torch.float64 and s.tolist() == [0.25, 4.0, 1.0 / 9.0] and R.same_bits(s, R.inv_scale2([2.0, 0.5, 3.0]))


def test_score_latent_rollout_refuses_bad_energy_arguments():
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    args = (torch.zeros(2, 1, 1, 2, 2), None, None, None, torch.zeros(3, 1, 4, 4), [0], None, None, torch.ones(4))
    with pytest.raises(ValueError, match="energy_scales"):
        EG.score_latent_rollout(*args, energy=True, energy_scales=torch.ones(1))
    with pytest.raises(ValueError, match="named twice"):
        EG.score_latent_rollout(*args, energy_groups=[("a", (0, 0))])
    with pytest.raises(ValueError, match="holds no channel"):
        EG.score_latent_rollout(*args, energy_groups=[("a", ())])
    with pytest.raises(ValueError, match="positive and finite"):
        EG.score_latent_rollout(*args, energy_groups=[("a", (0,))], energy_scales=torch.tensor([0.0]))


# ---- d. the command line -------------------------------------------------------------------------------------------------------------------
def test_parse_energy_groups():
    from ladcast_amd.evaluate import EnergyGroup
    from ladcast_amd.evaluate.evaluate_ens_gpu import parse_energy_groups

    names = ["geopotential_level500", "temperature_level850", "mean_sea_level_pressure", "2m_temperature"]
    got = parse_energy_groups([["synoptic", "geopotential_level500", "temperature_level850", "2"], ["surface", "3", "mean_sea_level_pressure"]], names)
    assert got == [EnergyGroup("synoptic", (0, 1, 2)), EnergyGroup("surface", (3, 2))]
    assert parse_energy_groups([], names) == []
    for bad in ([["lonely"]], [["a", "no_such_channel"]], [["a", "4"]], [["a", "0", "geopotential_level500"]], [["a", "0"], ["a", "1"]],
                [[str(k), "0"] for k in range(33)]):
        with pytest.raises(ValueError):
            parse_energy_groups(bad, names)


SCORES = ("ens_acc", "ens_mse", "crps_spread", "crps_skill", "crps")
VARS = ["--variable_names", "geopotential", "2m_temperature", "--levels", "500", "850", "--num_atm_vars", "1"]  # three channels


def _run_main(tmp_path, name, extra, G=0, drop=None):
    from ladcast_amd.evaluate import evaluate_ens_gpu as EG

    res = tmp_path / "rollout"
    if not res.exists():
        res.mkdir()
        for ts in (2018123000, 2018123106):
            np.save(res / f"latent_{ts}.npy", np.zeros((3, 1, 1, 1, 1), dtype=np.float32))
    C, T = 3, 4
    g = np.random.default_rng(7)
    per_init = []

    def score(path, time_str, t_slots, c_slots):
        out = {k: np.full((C, T), 1.0 + i, dtype=np.float32) for i, k in enumerate(SCORES)}
        if extra:
            en = {k: torch.from_numpy(g.uniform(0.5, 2.0, (C, T))) for k in EG.ENERGY_NAMES}
            en["energy_n_invalid"] = torch.from_numpy(g.integers(0, 9, (C, T)).astype(np.int32))
            en.update({k: torch.from_numpy(g.uniform(0.5, 2.0, (G, T))) for k in (EG.ENERGY_GROUP_NAMES if G else ())})
            en.pop(drop, None)
            per_init.append(en)
            out.update(en)
        return out

    out_dir = tmp_path / name
    out = EG.main(["--result_path", str(res), "--output", str(out_dir), "--start_date", "2018-12-29", "--end_date", "2019-01-01T18",
                   "--total_lead_time_hour", "24", "--step_size_hour", "6"] + VARS + extra, score=score)
    return out_dir, out, per_init


def test_main_energy_flags_write_the_energy_files(tmp_path):
    plain, _, _ = _run_main(tmp_path, "plain", [])
    before = sorted(p.name for p in plain.iterdir())
    per_channel = ["energy_score.npy", "energy_score_fair.npy", "energy_skill.npy", "energy_spread.npy", "energy_n_invalid.npy", "energy.json"]
    alone, out, per_init = _run_main(tmp_path, "energy", ["--energy"])
    assert sorted(p.name for p in alone.iterdir()) == sorted(before + per_channel)
    for p in plain.iterdir():  # every other file is the bytes of a run without the flags
        assert (alone / p.name).read_bytes() == p.read_bytes(), p.name
    for k in per_channel[:-1]:
        a = np.load(alone / k)
        assert a.shape == (2, 3, 4) and a.dtype == (np.int32 if k == "energy_n_invalid.npy" else np.float64), k
        assert np.array_equal(a, np.stack([p[k[:-4]].numpy() for p in per_init])) and np.array_equal(a, out[k[:-4]]), k
    assert json.loads((alone / "energy.json").read_text())["groups"] == []
    flags = ["--energy_group", "both_z", "geopotential_level500", "1", "--energy_group", "surface", "2m_temperature", "geopotential_level850"]  # implies --energy
    grouped, out, per_init = _run_main(tmp_path, "groups", flags, G=2)
    group_files = ["energy_group_score.npy", "energy_group_score_fair.npy", "energy_group_skill.npy", "energy_group_spread.npy"]
    assert sorted(p.name for p in grouped.iterdir()) == sorted(before + per_channel + group_files)
    for p in plain.iterdir():
        assert (grouped / p.name).read_bytes() == p.read_bytes(), p.name
    for k in group_files:
        a = np.load(grouped / k)
        assert a.shape == (2, 2, 4) and a.dtype == np.float64 and np.array_equal(a, np.stack([p[k[:-4]].numpy() for p in per_init])), k
    meta = json.loads((grouped / "energy.json").read_text())
    assert [(m["name"], m["channels"], m["channel_names"]) for m in meta["groups"]] == \
        [("both_z", [0, 1], ["geopotential_level500", "geopotential_level850"]), ("surface", [2, 1], ["2m_temperature", "geopotential_level850"])]
    for bad in (["--energy_group", "lonely"], ["--energy_group", "a", "no_such_channel"], ["--energy_group", "a", "0", "--energy_group", "a", "1"]):
        with pytest.raises(ValueError):
            _run_main(tmp_path, "bad", bad)
    with pytest.raises(ValueError, match="--energy needs"):  # a scorer that does not return every array
        _run_main(tmp_path, "short", ["--energy"], drop="energy_skill")


# ---- e. the library ------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_two_symbols():
    from ladcast_amd import hip

    for name in ("ldc_rollout_energy", "ldc_rollout_energy_workspace_bytes"):
        assert hasattr(hip.lib, name) and name in hip.SIGNATURES
    assert hip.lib.ldc_abi_version() == 5
    assert (hip.ENERGY_MAX_MEMBERS, hip.ENERGY_MAX_GROUPS, hip.ENERGY_PLANES) == (R.MAX_M, R.MAX_G, 5)
    wb = hip.lib.ldc_rollout_energy_workspace_bytes
    for M, C, G, L, H, W in ((1, 1, 0, 1, 1, 1), (5, 3, 2, 2, 3, 50), (64, 1, 0, 1, 16, 16), (256, 2, 32, 1, 13, 23), (88, 2, 1, 3, 17, 241),
                             (50, 84, 3, 4, 120, 240)):
        assert wb(M, C, G, L, H, W) == R.workspace_bytes(M, C, L, H * W), (M, C, G, L, H, W)
    assert wb(50, 84, 0, 4, 120, 240) == wb(50, 84, 32, 4, 120, 240) < 36 << 20  # 35.3 MB; the groups need no scratch
    for bad in ((0, 1, 0, 1, 4, 4), (257, 1, 0, 1, 4, 4), (4, 1, -1, 1, 4, 4), (4, 1, 33, 1, 4, 4), (4, 0, 0, 1, 4, 4), (4, 65536, 0, 1, 4, 4),
                (4, 1, 0, 0, 4, 4), (4, 1, 0, 65536, 4, 4), (4, 1, 0, 1, 0, 4), (4, 1, 0, 1, 4, 0), (4, 1, 0, 1, 4097, 4096)):
        assert wb(*bad) == 0, bad
