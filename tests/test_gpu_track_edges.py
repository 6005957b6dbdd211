"""Edge tests of the four tracker entry points of track.hip (ldc_track_gather, ldc_track_nanmean, ldc_track_storms,
ldc_track_local_min) on the MI355X.  Every comparison is bit for bit; a NaN is compared as a NaN; there are no tolerances.

Search and tracker: tests/golden/track_edge_ref.npz - made by the reference's own functions on custom grids (regional, irregular, one
row, one column, 0 and 360 both present, the 1024 x 1024 cap), with centres off the grid and fields of small integers, so that exact
ties are the rule - through the public API and through the C ABI with every output between guard bands, every plane between planes
of finite -1e30 (a read outside the plane wins a minimum), the coordinate arrays continued in ascending order and the land-sea mask
between planes of the opposite value.  tests/test_track_cpu.py pins tests/track_oracle.py to the same fixture, so the random cases
here use the oracle.  Gather and mean: per element against numpy float32 in the documented order of operations.  Refusals: every
refused call returns its status and writes nothing, and the same buffers are served afterwards."""
import itertools
import os
import warnings
from datetime import datetime

import numpy as np
import pytest
import torch

from tests import track_oracle as O
from tests.redzone import UNWRITTEN32, UNWRITTEN64, _signed, assert_untouched, guarded

pytestmark = pytest.mark.gpu

EDGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_edge_ref.npz")
T0 = datetime(2018, 10, 1, 0)
DEV = "cuda:0"
ARG, UNSUPPORTED = -1, -3
U32, U64 = _signed(UNWRITTEN32, 32), _signed(UNWRITTEN64, 64)
LOW = -1.0e30  # finite, below every field value: wins any minimum that reads it


@pytest.fixture(scope="module")
def hip():
    from ladcast_amd import hip
    return hip


@pytest.fixture(scope="module")
def edge():
    return dict(np.load(EDGE))


def _names(edge):
    return [str(n) for n in edge["grid_names"]]


def _grid(edge, name):
    return edge[f"{name}_lat"], edge[f"{name}_lon"]


_fields_cache = {}


def _fields(edge, name):
    """(F, H, W) fp32 planes of one grid, built once and never changed; the 1024 x 1024 planes come from the stored formulas"""
    if name not in _fields_cache:
        if f"{name}_fields" in edge:
            f = edge[f"{name}_fields"]
        else:
            lat, lon = _grid(edge, name)
            f = np.stack([O.formula_field(lat.size, lon.size, *p) for p in edge[f"{name}_formulas"]])
        f.setflags(write=False)
        _fields_cache[name] = f
    return _fields_cache[name]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # a copy: the shared fields are read-only


def _latlon(track):
    return np.array([(la, lo) for _, la, lo in track], dtype=np.float64)


def _same_bits(a, b):
    """bit for bit, except that a NaN equals a NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    n = np.isnan(a) & np.isnan(b)
    iv = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return bool(np.all(n | (np.ascontiguousarray(a).view(iv) == np.ascontiguousarray(b).view(iv))))


def _queries_of(edge, name):
    return np.nonzero(edge["q_grid"] == _names(edge).index(name))[0]


def _check_queries(edge, qs, res, what):
    """res[i]: (la, lo, v) or None of fixture query qs[i]: coordinates, the value's bytes and the None pattern"""
    assert len(res) == len(qs)
    for q, r in zip(qs, res):
        if edge["q_found"][q]:
            assert r is not None, (what, q)
            assert (r[0], r[1]) == tuple(edge["q_latlon"][q]), (what, q, r, edge["q_latlon"][q], edge["q_center"][q], edge["q_inner"][q])
            assert np.float32(r[2]).tobytes() == edge["q_value"][q].tobytes(), (what, q)
        else:
            assert r is None, (what, q, r)


# ---- embedded inputs, guarded outputs ---------------------------------------------------------------------------------------
def _embed_coord(c):
    """the coordinate array between 8 finite values before and after it that continue the ascent -> its view of the device buffer"""
    step = 1.0 if c.size == 1 else float(c[-1] - c[0]) / (c.size - 1)
    full = np.concatenate([c[0] - step * np.arange(8, 0, -1), c, c[-1] + step * np.arange(1, 9)])
    assert np.all(np.diff(full) > 0)
    return _dev(full)[8 : 8 + c.size]


def _embed_planes(planes, fill=LOW):
    """(N, H, W) planes -> flat device buffer [fill plane, plane 0, fill plane, plane 1, ..., fill plane]; plane n starts at (2 n + 1) H W"""
    N, H, W = planes.shape
    flat = torch.full(((2 * N + 1) * H * W,), fill, dtype=torch.float32, device=DEV)
    flat[H * W :].view(-1)[: 2 * N * H * W].view(N, 2, H * W)[:, 0] = _dev(planes).reshape(N, H * W)
    return flat


def _local_min_abi(hip, planes, field_idx, lat, lon, centers, inner, embed=True):
    """one ldc_track_local_min launch through the C ABI with guarded outputs -> (found, la, lo, v numpy arrays, the four Guarded)"""
    planes = np.asarray(planes)
    F, H, W = planes.shape
    nq = len(centers)
    if embed:
        flat = _embed_planes(planes)
        fptr, stride = flat[H * W :], 2 * H * W
        glat, glon = _embed_coord(lat), _embed_coord(lon)
    else:
        flat = _dev(planes)
        fptr, stride = flat, H * W
        glat, glon = _dev(lat), _dev(lon)
    fi = _dev(np.asarray(field_idx, dtype=np.int32))
    la0 = _dev(np.array([c[0] for c in centers], dtype=np.float64))
    lo0 = _dev(np.array([c[1] for c in centers], dtype=np.float64))
    inn = _dev(np.asarray(inner, dtype=np.int32))
    G = (guarded(1, nq, dtype=torch.int32), guarded(1, nq, dtype=torch.float64), guarded(1, nq, dtype=torch.float64), guarded(1, nq, dtype=torch.float32))
    st = hip.lib.ldc_track_local_min(hip._p(fptr), stride, hip._p(fi), hip._p(glat), H, hip._p(glon), W, hip._p(la0), hip._p(lo0), hip._p(inn), nq,
                                     hip._p(G[0].t), hip._p(G[1].t), hip._p(G[2].t), hip._p(G[3].t), hip._stream())
    torch.cuda.synchronize()
    assert st == 0, st
    for g, what in zip(G, ("found", "out_lat", "out_lon", "out_val")):
        assert_untouched(g, what)
    return tuple(g.payload().reshape(nq).numpy() for g in G) + (G,)


def _decode(found, la, lo, v):
    assert set(np.unique(found).tolist()) <= {0, 1}, found
    return [(float(la[q]), float(lo[q]), float(v[q])) if found[q] else None for q in range(found.size)]


def _storms_abi(hip, mslp, z700, lsm, lat, lon, starts, n_steps, boxes, em, embed=True, shared=False, null_code=False):
    """one ldc_track_storms launch through the C ABI with guarded outputs.  mslp / z700: (E, T, H, W) (shared: (T, H, W), read by every
    track through track_stride = 0) -> (lat, lon (n_tracks, n_steps + 1), codes (n_tracks, n_steps), the Guarded outputs)"""
    n_tracks = len(starts)
    m = np.asarray(mslp)[None] if shared else np.asarray(mslp)
    E, T, H, W = m.shape
    HW = H * W
    chans = [m] if z700 is None else [m, np.asarray(z700)[None] if shared else np.asarray(z700)]
    nc = len(chans)
    planes = np.stack(chans, axis=2).reshape(E * T * nc, H, W)  # (track, frame, channel) order
    if embed:
        flat = _embed_planes(planes)
        fptr, plane = flat[HW:], 2 * HW
        glat, glon = _embed_coord(lat), _embed_coord(lon)
    else:
        flat = _dev(planes)
        fptr, plane = flat, HW
        glat, glon = _dev(lat), _dev(lon)
    frame_stride = nc * plane
    track_stride = 0 if shared else T * frame_stride
    z_off = plane if z700 is not None else -1
    lsm_d = None
    if lsm is not None:
        l = np.asarray(lsm, dtype=np.float32)
        lsm_flat = _dev(np.stack([1 - l, l, 1 - l]).reshape(-1)) if embed else _dev(l.reshape(-1))
        lsm_d = lsm_flat[HW : 2 * HW] if embed else lsm_flat
    la0 = _dev(np.array([s[0] for s in starts], dtype=np.float64))
    lo0 = _dev(np.array([s[1] for s in starts], dtype=np.float64))
    Gla, Glo = guarded(n_tracks, n_steps + 1, dtype=torch.float64), guarded(n_tracks, n_steps + 1, dtype=torch.float64)
    Gc = guarded(n_tracks, max(n_steps, 1), dtype=torch.int32)
    st = hip.lib.ldc_track_storms(hip._p(fptr), track_stride, frame_stride, 0, z_off, hip._p(lsm_d), hip._p(glat), H, hip._p(glon), W, hip._p(la0),
                                  hip._p(lo0), n_tracks, n_steps, hip._int_array(boxes), len(boxes), int(em), hip._p(Gla.t), hip._p(Glo.t),
                                  None if null_code else hip._p(Gc.t), hip._stream())
    torch.cuda.synchronize()
    assert st == 0, st
    for g, what in ((Gla, "out_lat"), (Glo, "out_lon"), (Gc, "out_code")):
        assert_untouched(g, what)
    codes = Gc.payload().reshape(n_tracks, max(n_steps, 1)).numpy()
    if n_steps == 0 or null_code:
        assert (codes == U32).all()  # no step: no code is written
    return Gla.payload().reshape(n_tracks, n_steps + 1).numpy(), Glo.payload().reshape(n_tracks, n_steps + 1).numpy(), codes[:, :n_steps], (Gla, Glo, Gc)


def _oracle_track(mslp, z700, lsm, lat, lon, start, n_steps, boxes, em):
    trk, codes = O.track_first_n_steps(T0, start[0], start[1], mslp, n_steps, boxes, em, z700, lsm, lat, lon, return_codes=True, round_start=False)
    return _latlon(trk), codes


# ---- the fixture ------------------------------------------------------------------------------------------------------------
GRIDS = ["G1", "G2", "G3", "G4a", "G4b", "G5", "G6"]


@pytest.mark.parametrize("name", GRIDS)
def test_fixture_queries_through_the_public_api(edge, name):
    from ladcast_amd.evaluate.track import find_local_minima

    lat, lon = _grid(edge, name)
    qs = _queries_of(edge, name)
    res = find_local_minima(_dev(_fields(edge, name)), [tuple(c) for c in edge["q_center"][qs]], edge["q_inner"][qs].tolist(),
                            edge["q_field"][qs].tolist(), lat=lat, lon=lon)
    _check_queries(edge, qs, res, name)


@pytest.mark.parametrize("name", GRIDS)
def test_fixture_queries_through_the_c_abi_between_guards(hip, edge, name):
    lat, lon = _grid(edge, name)
    qs = _queries_of(edge, name)
    centers, inner, fidx = [tuple(c) for c in edge["q_center"][qs]], edge["q_inner"][qs], edge["q_field"][qs]
    found, la, lo, v, _ = _local_min_abi(hip, _fields(edge, name), fidx, lat, lon, centers, inner, embed=True)
    _check_queries(edge, qs, _decode(found, la, lo, v), name)
    plain = _local_min_abi(hip, _fields(edge, name), fidx, lat, lon, centers, inner, embed=False)
    for a, b in zip((found, la, lo, v), plain[:4]):
        assert _same_bits(a, b), name  # the embedded run equals the unembedded one


def test_fixture_tracks_through_the_public_api_and_the_c_abi(hip, edge):
    from ladcast_amd.evaluate.track import round_to_grid, track_first_n_steps

    for i in range(int(edge["n_tracks"])):
        lat, lon = _grid(edge, str(edge[f"t{i}_grid"]))
        em = bool(edge[f"t{i}_enforce_msl"])
        mslp, z, lsm = edge[f"t{i}_mslp"], edge.get(f"t{i}_z700"), edge.get(f"t{i}_lsm")
        boxes = edge[f"t{i}_boxes"].tolist()
        n_steps = mslp.shape[0] - 1
        kw = {} if em else dict(z700=_dev(z), land_sea_mask=_dev(lsm))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            trk, codes = track_first_n_steps(T0, *edge[f"t{i}_start"], _dev(mslp), n_steps=n_steps, inner_box_sizes=boxes, enforce_msl=em,
                                             lat=lat, lon=lon, return_codes=True, **kw)
        assert np.array_equal(_latlon(trk), edge[f"t{i}_track"]), i
        start = (round_to_grid(edge[f"t{i}_start"][0]), round_to_grid(edge[f"t{i}_start"][1]))
        _, want_codes = _oracle_track(mslp, z, lsm, lat, lon, start, n_steps, boxes, em)
        assert list(codes) == want_codes, i
        for embed in (True, False):
            la, lo, cd, _ = _storms_abi(hip, mslp[None], None if em else z[None], None if em else lsm, lat, lon, [start], n_steps, boxes, em, embed=embed)
            assert np.array_equal(np.stack([la[0], lo[0]], 1), edge[f"t{i}_track"]) and list(cd[0]) == want_codes, (i, embed)


# ---- the sentinel path and non-finite centres -----------------------------------------------------------------------------
def test_sentinel_queries_write_found_only(hip, edge):
    """inner outside [0, 30] in a batch: found = LDC_ERR_UNSUPPORTED, the other three outputs keep their initial pattern; the valid
    queries of the same launch are served"""
    lat, lon = _grid(edge, "G2")
    fields = _fields(edge, "G2")
    centers = [(0.5, 120.5), (0.5, 120.5), (1.25, 119.0), (-3.0, 130.0), (0.5, 120.5), (9.5, 139.5)]
    inner = [1, -1, 5, 31, 12, 0]
    fidx = [0, 0, 1, 1, 1, 0]
    found, la, lo, v, G = _local_min_abi(hip, fields, fidx, lat, lon, centers, inner)
    for q in range(len(inner)):
        if inner[q] in (-1, 31):
            assert found[q] == UNSUPPORTED, q
            assert la.view(np.int64)[q] == U64 and lo.view(np.int64)[q] == U64 and v.view(np.int32)[q] == U32, q
        else:
            want = O.find_local_minimum(fields[fidx[q]], centers[q], inner[q], lat, lon)
            got = (float(la[q]), float(lo[q]), float(v[q])) if found[q] == 1 else None
            assert found[q] in (0, 1) and got == want, (q, got, want)
    assert sum(found == 1) >= 3


BAD = [float("nan"), float("inf"), float("-inf")]


def test_non_finite_centres_find_nothing(hip, edge):
    for name in ("G1", "G3", "G4a", "G4b"):
        lat, lon = _grid(edge, name)
        fields = _fields(edge, name)
        gla, glo = float(lat[lat.size // 2]), float(lon[lon.size // 2])
        centers = [(gla, glo)] + [c for b in BAD for c in ((b, glo), (gla, b), (b, b))] + [(gla, glo)]
        inner = [30] + [(0, 1, 30)[k % 3] for k in range(9)] + [30]
        found, la, lo, v, _ = _local_min_abi(hip, fields, [0] * len(centers), lat, lon, centers, inner)
        assert found.tolist() == [1] + [0] * 9 + [1], (name, found)
        assert (float(la[0]), float(lo[0]), float(v[0])) == O.find_local_minimum(fields[0], (gla, glo), 30, lat, lon)


@pytest.mark.parametrize("em", [True, False])
def test_non_finite_starts_stay_where_they_are(hip, edge, em):
    """with enforce_msl = False the land-sea mask's nearest lookup runs on the non-finite coordinate"""
    lat, lon = _grid(edge, "G2")
    mslp, z, lsm = edge["t1_mslp"], edge["t1_z700"], edge["t1_lsm"]
    starts = [(1.5, 121.5)] + [c for b in BAD for c in ((b, 121.5), (1.5, b), (b, b))]
    n_steps = mslp.shape[0] - 1
    la, lo, cd, _ = _storms_abi(hip, mslp, None if em else z, None if em else lsm, lat, lon, starts, n_steps, [7, 4, 1], em, shared=True)
    for e, s in enumerate(starts):
        want, wcodes = _oracle_track(mslp, z, lsm, lat, lon, s, n_steps, [7, 4, 1], em)
        assert _same_bits(np.stack([la[e], lo[e]], 1), want) and list(cd[e]) == wcodes, (e, s)
        if e:
            assert _same_bits(la[e], np.full(n_steps + 1, s[0])) and _same_bits(lo[e], np.full(n_steps + 1, s[1])) and not cd[e].any(), (e, s)
    assert cd[0].all()  # the finite start of the same launch moves


# ---- shapes of the launch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 65])
def test_query_and_track_counts(hip, edge, n):
    lat, lon = _grid(edge, "G2")
    qs = np.resize(_queries_of(edge, "G2")[::3], n)
    found, la, lo, v, _ = _local_min_abi(hip, _fields(edge, "G2"), edge["q_field"][qs], lat, lon, [tuple(c) for c in edge["q_center"][qs]], edge["q_inner"][qs])
    _check_queries(edge, qs, _decode(found, la, lo, v), n)
    # n tracks on one shared buffer (track_stride = 0) and on n copies of it (distinct strides): the same tracks, equal to the oracle
    mslp, z, lsm = edge["t1_mslp"], edge["t1_z700"], edge["t1_lsm"]
    rng = np.random.default_rng(n)
    starts = [(1.5, 121.5)] + [(float(rng.integers(-8 * 64, 8 * 64)) / 64, float(rng.integers(102 * 64, 138 * 64)) / 64) for _ in range(n - 1)]
    n_steps = mslp.shape[0] - 1
    a = _storms_abi(hip, mslp, z, lsm, lat, lon, starts, n_steps, [7, 4, 1], False, shared=True)
    b = _storms_abi(hip, np.repeat(mslp[None], n, 0), np.repeat(z[None], n, 0), lsm, lat, lon, starts, n_steps, [7, 4, 1], False)
    for x, y in zip(a[:3], b[:3]):
        assert _same_bits(x, y)
    for e in range(0, n, 8):
        want, wcodes = _oracle_track(mslp, z, lsm, lat, lon, starts[e], n_steps, [7, 4, 1], False)
        assert np.array_equal(np.stack([a[0][e], a[1][e]], 1), want) and list(a[2][e]) == wcodes, (e, starts[e])


def test_no_steps_writes_the_start_only(hip, edge):
    lat, lon = _grid(edge, "G2")
    starts = [(1.5, 121.5), (0.25, 110.0), (float("nan"), 3.0)]
    la, lo, _, (_, _, Gc) = _storms_abi(hip, edge["t0_mslp"], None, None, lat, lon, starts, 0, [7, 4, 1], True, shared=True, null_code=True)
    assert _same_bits(la[:, 0], np.array([s[0] for s in starts])) and _same_bits(lo[:, 0], np.array([s[1] for s in starts]))


@pytest.mark.parametrize("boxes", [[4], [30, 12, 7, 5, 4, 2, 1, 0]])
def test_one_and_eight_boxes(hip, edge, boxes):
    lat, lon = _grid(edge, "G2")
    mslp = edge["t0_mslp"]
    starts = [(1.5, 121.5), (-2.25, 118.75), (8.5, 135.015625)]
    n_steps = mslp.shape[0] - 1
    la, lo, cd, _ = _storms_abi(hip, mslp, None, None, lat, lon, starts, n_steps, boxes, True, shared=True)
    for e, s in enumerate(starts):
        want, wcodes = _oracle_track(mslp, None, None, lat, lon, s, n_steps, boxes, True)
        assert np.array_equal(np.stack([la[e], lo[e]], 1), want) and list(cd[e]) == wcodes, (e, s)


# ---- random cases against the oracle ----------------------------------------------------------------------------------------
def _random_grid(rng, kind):
    H, W = int(rng.integers(1, 49)), int(rng.integers(1, 49))
    step = float(rng.choice([0.25, 0.5, 1.0, 1.5, 2.0]))
    lat = float(rng.integers(-60, 40)) * 0.5 + step * np.arange(H)
    if kind == 0:  # dyadic-regular, anywhere
        lon = float(rng.integers(0, 500)) * 0.5 + step * np.arange(W)
    elif kind == 1:  # regional, starting at 0 or ending at 360
        lon = step * np.arange(W) if rng.random() < 0.5 else 360.0 - step * np.arange(W - 1, -1, -1)
    else:  # closing the seam: columns on both sides of 0 / 360, optionally with 0 and 360 both present
        a = int(rng.integers(0, W + 1))
        lon = np.concatenate([step * np.arange(a), 360.0 - step * np.arange(W - a, 0, -1) + (step if rng.random() < 0.3 and a < W else 0.0)])
    lon = lon[(lon >= 0) & (lon <= 360)] if kind else lon
    assert np.all(np.diff(lat) > 0) and np.all(np.diff(lon) > 0) and lon.size >= 1
    return lat, lon


def test_random_cases_on_random_small_grids_equal_oracle():
    """>= 120 seeded cases: one launch per (grid, box list, enforce_msl) group, integer fields with NaN patches, starts off the grid"""
    from ladcast_amd.evaluate.track import _track_launch

    rng = np.random.default_rng(11)
    box_lists = [[7, 2, 0], [12, 5, 1], [30], [5, 1], [2, 0], [1], [7, 5, 2], [30, 12, 0]]
    T, per, n = 3, 8, 0
    for g in range(16):
        lat, lon = _random_grid(rng, g % 3)
        H, W = lat.size, lon.size
        boxes, em = box_lists[g % len(box_lists)], bool((g + g // len(box_lists)) % 2)  # every box list under both settings
        mslp = rng.integers(0, 6, (per, T, H, W)).astype(np.float32)
        z = rng.integers(0, 6, (per, T, H, W)).astype(np.float32)
        for f in (mslp, z):
            for e in range(per):
                if rng.random() < 0.5:
                    r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
                    f[e, int(rng.integers(0, T)) :, r0 : r0 + int(rng.integers(1, 6)), c0 : c0 + int(rng.integers(1, 6))] = np.nan
        lsm = (rng.random((H, W)) < 0.4).astype(np.float32)
        starts = []
        for e in range(per):
            lo0 = float(np.round(rng.uniform(lon[0] - 2, lon[-1] + 2) * 64) / 64) if rng.random() < 0.7 else float(rng.choice([359.25, 360.75, -0.75, 0.0, 360.0]))
            starts.append((float(np.round(rng.uniform(lat[0] - 2, lat[-1] + 2) * 64) / 64), lo0))
        nc = 1 if em else 2
        buf = _dev(mslp[:, :, None] if em else np.stack([mslp, z], axis=2))
        lats, lons, codes = _track_launch(buf, track_stride=T * nc * H * W, frame_stride=nc * H * W, mslp_off=0, z_off=None if em else H * W,
                                          lsm=None if em else _dev(lsm), n_tracks=per, n_frames=T, n_steps=T - 1, lat0=[s[0] for s in starts],
                                          lon0=[s[1] for s in starts], inner_box_sizes=boxes, enforce_msl=em, lat=lat, lon=lon)
        dyadic = O.is_dyadic(lat, lon)
        assert dyadic

        def search(field, center, inner, la, lo):  # the precondition under which the kernel's key is the reference's
            fin = O.survivors(field, center, inner, la, lo)
            _, problem = O.key_check(fin, center, True)
            assert problem is None, problem
            return O.closest(fin, center)

        for e in range(per):
            trk, wcodes = O.track_first_n_steps(T0, *starts[e], mslp[e], T - 1, boxes, em, None if em else z[e], None if em else lsm, lat, lon,
                                                return_codes=True, search=search, round_start=False)
            assert np.array_equal(np.stack([lats[e], lons[e]], 1), _latlon(trk)), (g, e, lat.size, lon.size, boxes, em, starts[e])
            assert list(codes[e]) == wcodes, (g, e)
            n += 1
    assert n >= 120


def test_two_launches_are_bitwise_equal(hip, edge):
    """the irregular grid's searches with the most surviving candidates, twice"""
    lat, lon = _grid(edge, "G3")
    qs = _queries_of(edge, "G3")
    qs = qs[edge["q_found"][qs] == 1][:40]
    args = (hip, _fields(edge, "G3"), edge["q_field"][qs], lat, lon, [tuple(c) for c in edge["q_center"][qs]], edge["q_inner"][qs])
    a, b = _local_min_abi(*args), _local_min_abi(*args)
    for x, y in zip(a[:4], b[:4]):
        assert _same_bits(x, y)
    _check_queries(edge, qs, _decode(*a[:4]), "G3 twice")


# ---- gather -------------------------------------------------------------------------------------------------------------------
C_SRC = 8
CHANNEL_LISTS = [[2], [5, 0, 3, 7, 1, 6, 4, 2], [3, 3, 1]]


def _gather_source(rng, B, T, HW, layout):
    """x values (B, T, C, HW) inside a wider buffer of finite 1e30: planes 3 floats apart, 64 floats before and after ->
    (device buffer, view, sb, st, sc)"""
    ld = HW + 3
    flat = torch.full((64 + B * T * C_SRC * ld + 64,), 1.0e30, dtype=torch.float32, device=DEV)
    vals = (rng.standard_normal((B, T, C_SRC, HW)) * 3).astype(np.float32)
    if layout == "btc":
        sb, st, sc = T * C_SRC * ld, C_SRC * ld, ld
    else:  # (B, C, T, HW)
        sb, sc, st = C_SRC * T * ld, T * ld, ld
    view = flat.as_strided((B, T, C_SRC, HW), (sb, st, sc, 1), 64)
    view.copy_(_dev(vals))
    return flat, view, vals, sb, st, sc


@pytest.mark.parametrize("layout", ["btc", "bct"])
@pytest.mark.parametrize("HW", [1, 255, 256, 257])
def test_gather_per_element(hip, HW, layout):
    rng = np.random.default_rng(HW)
    mean = (rng.standard_normal(C_SRC) * 100).astype(np.float32)
    sd = (rng.random(C_SRC) * 3 + 0.5).astype(np.float32)
    md, sdd = _dev(mean), _dev(sd)
    for B, T in itertools.product((1, 3), (1, 2)):
        flat, view, vals, sb, st, sc = _gather_source(rng, B, T, HW, layout)
        T_total = T + 2
        for ch, t_off, ts in itertools.product(CHANNEL_LISTS, (0, 1, 2), (1.0, 0.5, 0.3)):
            n_ch = len(ch)
            out = guarded(B * T_total * n_ch, HW)
            st_ = hip.lib.ldc_track_gather(hip._p(view), sb, st, sc, B, T, HW, hip._int_array(ch), n_ch, hip._p(md), hip._p(sdd), ts, hip._p(out.t),
                                           T_total, t_off, hip._stream())
            torch.cuda.synchronize()
            assert st_ == 0
            assert_untouched(out, "gather out")
            got = out.payload().reshape(B, T_total, n_ch, HW).numpy()
            want = np.full((B, T_total, n_ch, HW), 0, dtype=np.int32).view(np.float32)
            want.view(np.int32)[...] = U32  # frames outside the window keep the initial pattern
            for k, c in enumerate(ch):  # numpy float32, one rounding per operation, in chan_affine's order
                want[:, t_off : t_off + T, k] = (vals[:, :, c] / np.float32(ts)) * sd[c] + mean[c]
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (B, T, ch, t_off, ts)


# ---- nanmean ------------------------------------------------------------------------------------------------------------------
def _sequential_nanmean(x):
    """NaN -> 0, fp32 sum in member order starting from member 0, one division by the count (tests/test_track_cpu.py)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(np.isnan(x[0]), np.float32(0), x[0])
        for e in range(1, x.shape[0]):
            acc = acc + np.where(np.isnan(x[e]), np.float32(0), x[e])
        cnt = (~np.isnan(x)).sum(axis=0)
        return (acc / cnt.astype(np.float32)).astype(np.float32)


def _special_columns(E):
    """(E,) columns: all NaN; -0.0 as the only valid member; +inf with -inf; one NaN among infinities"""
    nan, inf = np.float32("nan"), np.float32("inf")
    only = np.full(E, nan, np.float32)
    only[-1] = -0.0
    both = np.full(E, inf, np.float32)
    both[E // 2 :] = -inf  # E = 1: -inf alone
    among = np.full(E, inf, np.float32)
    among[E // 2] = nan
    return [np.full(E, nan, np.float32), only, both, among]


@pytest.mark.parametrize("E", [1, 2, 9])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_nanmean_per_element(hip, n, E):
    rng = np.random.default_rng(1000 * n + E)
    specials = _special_columns(E)
    variants = range(len(specials) + 1) if n == 1 else [0]  # one column: one launch per special column, and a plain one
    for variant in variants:
        x = (rng.standard_normal((E, n)) * 1000 + 101325).astype(np.float32)
        x[rng.random(x.shape) < 0.2] = np.nan
        if n == 1:
            if variant:
                x[:, 0] = specials[variant - 1]
        else:
            for k, col in enumerate(specials):
                x[:, 7 * k] = col
        for stride in (n, n + 37, 0):
            rows = 1 if stride == 0 else E
            ld = max(stride, n)
            flat = torch.full((64 + rows * ld + 64,), 1.0e30, dtype=torch.float32, device=DEV)
            view = flat.as_strided((rows, n), (ld, 1), 64)
            view.copy_(_dev(x[:rows]))
            src = np.repeat(x[:1], E, 0) if stride == 0 else x
            out = guarded(1, n)
            st = hip.lib.ldc_track_nanmean(hip._p(view), stride, E, n, hip._p(out.t), hip._stream())
            torch.cuda.synchronize()
            assert st == 0
            assert_untouched(out, "nanmean out")
            got, want = out.payload().reshape(n).numpy(), _sequential_nanmean(src)
            assert not (got.view(np.int32) == U32).any()
            assert _same_bits(got, want), (n, E, stride, variant, got[:32], want[:32])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _unwritten(*bufs):
    """every guard and every payload word of the guarded outputs holds its initial pattern"""
    for g in bufs:
        assert_untouched(g, "refused call")
        p = g.payload()
        if p.element_size() == 8:
            assert bool((p.view(torch.int64) == U64).all())
        else:
            assert bool((p.view(torch.int32) == U32).all())


def _call(f, order, base, **over):
    a = dict(base, **over)
    return f(*[a[k] for k in order])


def test_gather_refusals_launch_nothing(hip):
    rng = np.random.default_rng(2)
    B, T, HW, T_total, t_off, ch = 2, 2, 257, 4, 1, [5, 1]
    flat, view, vals, sb, st, sc = _gather_source(rng, B, T, HW, "btc")
    mean, sd = (rng.standard_normal(C_SRC) * 10).astype(np.float32), (rng.random(C_SRC) + 0.5).astype(np.float32)
    md, sdd = _dev(mean), _dev(sd)
    out = guarded(B * T_total * len(ch), HW)
    order = ["x", "sb", "st", "sc", "B", "T", "HW", "channels", "n_ch", "mean", "std", "ts", "out", "T_total", "t_off", "stream"]
    base = dict(x=hip._p(view), sb=sb, st=st, sc=sc, B=B, T=T, HW=HW, channels=hip._int_array(ch), n_ch=2, mean=hip._p(md), std=hip._p(sdd), ts=1.0,
                out=hip._p(out.t), T_total=T_total, t_off=t_off, stream=hip._stream())
    f = hip.lib.ldc_track_gather
    table = [(dict(x=None), ARG), (dict(channels=None), ARG), (dict(mean=None), ARG), (dict(std=None), ARG), (dict(out=None), ARG),
             (dict(B=0), ARG), (dict(B=-1), ARG), (dict(T=0), ARG), (dict(T=-2), ARG), (dict(HW=0), ARG), (dict(HW=-5), ARG),
             (dict(t_off=3), ARG), (dict(t_off=-1), ARG), (dict(T_total=2), ARG), (dict(n_ch=0), ARG), (dict(n_ch=-1), ARG),
             (dict(n_ch=9, channels=hip._int_array(list(range(9)))), UNSUPPORTED), (dict(channels=hip._int_array([5, -1])), ARG),
             (dict(B=65536), UNSUPPORTED),
             (dict(T=8192, T_total=8192, t_off=0, n_ch=8, channels=hip._int_array(list(range(8)))), UNSUPPORTED),  # T * n_ch = 65536
             (dict(T=65536, T_total=65536, t_off=0, n_ch=1), UNSUPPORTED)]
    for over, want in table:
        assert _call(f, order, base, **over) == want, over
    torch.cuda.synchronize()
    _unwritten(out)
    assert _call(f, order, base) == 0  # the same buffers are served once the arguments are right
    torch.cuda.synchronize()
    assert_untouched(out, "gather out")
    got = out.payload().reshape(B, T_total, 2, HW).numpy()
    for k, c in enumerate(ch):
        assert np.array_equal(got[:, t_off : t_off + T, k], (vals[:, :, c] / np.float32(1.0)) * sd[c] + mean[c])
    assert (got[:, [0, 3]].view(np.int32) == U32).all()


def test_nanmean_refusals_launch_nothing(hip):
    E, n = 3, 257
    x = np.random.default_rng(4).standard_normal((E, n)).astype(np.float32)
    xd = _dev(x)
    out = guarded(1, n)
    order = ["x", "stride", "E", "n", "out", "stream"]
    base = dict(x=hip._p(xd), stride=n, E=E, n=n, out=hip._p(out.t), stream=hip._stream())
    f = hip.lib.ldc_track_nanmean
    for over in (dict(x=None), dict(out=None), dict(E=0), dict(E=-1), dict(n=0), dict(n=-3), dict(stride=-1), dict(stride=-n)):
        assert _call(f, order, base, **over) == ARG, over
    torch.cuda.synchronize()
    _unwritten(out)
    assert _call(f, order, base) == 0
    torch.cuda.synchronize()
    assert_untouched(out, "nanmean out")
    assert _same_bits(out.payload().reshape(n).numpy(), _sequential_nanmean(x))


def test_storms_refusals_launch_nothing(hip, edge):
    lat, lon = _grid(edge, "G2")
    H, W = lat.size, lon.size
    mslp, z, lsm = edge["t1_mslp"], edge["t1_z700"], edge["t1_lsm"]
    T = mslp.shape[0]
    n_steps, boxes, starts = T - 1, [7, 4, 1], [(1.5, 121.5), (0.25, 110.0)]
    buf = _dev(np.stack([mslp, z], axis=1))  # (T, 2, H, W), shared by both tracks
    glat, glon, lsm_d = _dev(lat), _dev(lon), _dev(lsm)
    la0, lo0 = _dev(np.array([s[0] for s in starts])), _dev(np.array([s[1] for s in starts]))
    Gla, Glo, Gc = guarded(2, n_steps + 1, dtype=torch.float64), guarded(2, n_steps + 1, dtype=torch.float64), guarded(2, n_steps, dtype=torch.int32)
    order = ["fields", "ts", "fs", "mo", "zo", "lsm", "lat", "H", "lon", "W", "lat0", "lon0", "nt", "ns", "boxes", "nb", "em", "ola", "olo", "oc", "stream"]
    base = dict(fields=hip._p(buf), ts=0, fs=2 * H * W, mo=0, zo=H * W, lsm=hip._p(lsm_d), lat=hip._p(glat), H=H, lon=hip._p(glon), W=W, lat0=hip._p(la0),
                lon0=hip._p(lo0), nt=2, ns=n_steps, boxes=hip._int_array(boxes), nb=3, em=0, ola=hip._p(Gla.t), olo=hip._p(Glo.t), oc=hip._p(Gc.t),
                stream=hip._stream())
    f = hip.lib.ldc_track_storms
    table = [(dict(fields=None), ARG), (dict(lat=None), ARG), (dict(lon=None), ARG), (dict(lat0=None), ARG), (dict(lon0=None), ARG),
             (dict(boxes=None), ARG), (dict(ola=None), ARG), (dict(olo=None), ARG),
             (dict(H=0), ARG), (dict(W=0), ARG), (dict(H=-1), ARG), (dict(W=-1), ARG), (dict(H=1025), UNSUPPORTED), (dict(W=1025), UNSUPPORTED),
             (dict(nt=0), ARG), (dict(nt=-1), ARG), (dict(ns=-1), ARG), (dict(nb=0), ARG), (dict(nb=-1), ARG),
             (dict(nb=9, boxes=hip._int_array([1] * 9)), UNSUPPORTED), (dict(boxes=hip._int_array([7, -1, 1])), ARG),
             (dict(boxes=hip._int_array([7, 31, 1])), UNSUPPORTED), (dict(lsm=None), ARG), (dict(zo=-1), ARG), (dict(oc=None), ARG)]
    for over, want in table:
        assert _call(f, order, base, **over) == want, over
    torch.cuda.synchronize()
    _unwritten(Gla, Glo, Gc)
    assert _call(f, order, base) == 0
    torch.cuda.synchronize()
    for g in (Gla, Glo, Gc):
        assert_untouched(g, "storms out")
    la, lo, cd = Gla.payload().reshape(2, -1).numpy(), Glo.payload().reshape(2, -1).numpy(), Gc.payload().reshape(2, -1).numpy()
    for e, s in enumerate(starts):
        want, wcodes = _oracle_track(mslp, z, lsm, lat, lon, s, n_steps, boxes, False)
        assert np.array_equal(np.stack([la[e], lo[e]], 1), want) and list(cd[e]) == wcodes, e


def test_local_min_refusals_launch_nothing(hip, edge):
    lat, lon = _grid(edge, "G2")
    H, W = lat.size, lon.size
    fields = _fields(edge, "G2")
    centers, inner, fidx = [(0.5, 120.5), (1.25, 119.0), (-3.0, 130.0)], [1, 5, 12], [0, 1, 1]
    fd, glat, glon = _dev(fields), _dev(lat), _dev(lon)
    fi, inn = _dev(np.array(fidx, dtype=np.int32)), _dev(np.array(inner, dtype=np.int32))
    la0, lo0 = _dev(np.array([c[0] for c in centers])), _dev(np.array([c[1] for c in centers]))
    G = (guarded(1, 3, dtype=torch.int32), guarded(1, 3, dtype=torch.float64), guarded(1, 3, dtype=torch.float64), guarded(1, 3, dtype=torch.float32))
    order = ["fields", "fs", "fi", "lat", "H", "lon", "W", "lat0", "lon0", "inner", "nq", "found", "ola", "olo", "ov", "stream"]
    base = dict(fields=hip._p(fd), fs=H * W, fi=hip._p(fi), lat=hip._p(glat), H=H, lon=hip._p(glon), W=W, lat0=hip._p(la0), lon0=hip._p(lo0),
                inner=hip._p(inn), nq=3, found=hip._p(G[0].t), ola=hip._p(G[1].t), olo=hip._p(G[2].t), ov=hip._p(G[3].t), stream=hip._stream())
    f = hip.lib.ldc_track_local_min
    table = [(dict([(k, None)]), ARG) for k in ("fields", "fi", "lat", "lon", "lat0", "lon0", "inner", "found", "ola", "olo", "ov")]
    table += [(dict(H=0), ARG), (dict(W=0), ARG), (dict(H=-1), ARG), (dict(H=1025), UNSUPPORTED), (dict(W=1025), UNSUPPORTED), (dict(nq=0), ARG),
              (dict(nq=-1), ARG)]
    for over, want in table:
        assert _call(f, order, base, **over) == want, over
    torch.cuda.synchronize()
    _unwritten(*G)
    assert _call(f, order, base) == 0
    torch.cuda.synchronize()
    for g in G:
        assert_untouched(g, "local_min out")
    found, la, lo, v = (g.payload().reshape(3).numpy() for g in G)
    assert _decode(found, la, lo, v) == [O.find_local_minimum(fields[fidx[q]], centers[q], inner[q], lat, lon) for q in range(3)]
    # the public wrapper refuses the sentinel sizes before any launch
    from ladcast_amd.evaluate.track import find_local_minima

    for bad in (-1, 31):
        with pytest.raises(ValueError):
            find_local_minima(fd, [(0.5, 120.5)], [bad], [0], lat=lat, lon=lon)
