"""Regenerate tests/golden/track_ref.npz from the reference's OWN tracking code (needs the reference tree at REF; not run by the tests).

    python tests/golden/make_track_golden.py [REFERENCE_ROOT]     (default: the reference checkout make_golden.py reads)
    python tests/golden/make_track_golden.py --edges [REFERENCE_ROOT]     writes tests/golden/track_edge_ref.npz only (see edges())

`round_to_grid`, `select_box`, `find_local_minimum` and `track_first_n_steps` are compiled from the syntax tree of
ladcast/evaluate/track.py (the module imports cartopy, requests and xarray, which this tree does not have) and run on synthetic,
seeded fields: a flat background plus moving Gaussian lows, rounded to 1 Pa / 1 m^2 s^-2 so that plateaus of equal values occur.

The datasets they walk are a minimal xarray stand-in written below.  It implements only what those four functions touch:
coordinate comparisons to masks and their `&` / `|`; `where(mask, drop=True)` with an order-preserving drop; `.size`, `.values`,
`.compute()`; `.min()` with skipna; `.sel(latitude=, longitude=, method="nearest")` through pandas' own get_indexer (its tie rule);
`.sel(time=, prediction_timedelta=)`, `ds[var]`, `.dims`, `.sel({ens_dim: m})`, `.sel(level=700)`; `.load()` and `.mean(dim=)` as
np.nanmean.  The stand-in's fidelity to xarray is the one link of this fixture that is not pinned to reference code - as with the
diffusers leaves of DESIGN.md section 2: the stand-in is small enough to read against xarray's documented semantics.
"""
import ast
import os
import sys
import warnings
from datetime import datetime, timedelta

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
_ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REF = os.path.join(_ARGS[0] if _ARGS else "/root/reference", "ladcast", "evaluate", "track.py")

LAT = np.arange(-88.5, 90 + 1e-6, 1.5)
LON = np.arange(0, 358.5 + 1e-6, 1.5)


# ---- the xarray stand-in ----------------------------------------------------------------------------------------------------
class Mask:
    """a boolean array over named dims (the result of comparing coordinates)"""

    def __init__(self, dims, values):
        self.dims, self.values = tuple(dims), np.asarray(values, dtype=bool)

    def _bin(self, other, op):
        dims = self.dims + tuple(d for d in other.dims if d not in self.dims)
        return Mask(dims, op(self._expand(dims), other._expand(dims)))

    def _expand(self, dims):
        v = self.values
        src = list(self.dims)
        for d in dims:
            if d not in src:
                v = v[..., None]
                src.append(d)
        return np.transpose(v, [src.index(d) for d in dims])

    def __and__(self, other):
        return self._bin(other, np.logical_and)

    def __or__(self, other):
        return self._bin(other, np.logical_or)


class Coord:
    def __init__(self, name, values):
        self.name, self.values = name, np.asarray(values)

    def _cmp(self, x, op):
        return Mask((self.name,), op(self.values, x))

    def __ge__(self, x):
        return self._cmp(x, np.greater_equal)

    def __le__(self, x):
        return self._cmp(x, np.less_equal)

    def __gt__(self, x):
        return self._cmp(x, np.greater)

    def __lt__(self, x):
        return self._cmp(x, np.less)


def _label_index(coord_values, label, method=None):
    if method == "nearest":
        i = int(pd.Index(coord_values).get_indexer([label], method="nearest")[0])
    else:
        hits = [i for i, c in enumerate(coord_values) if c == label]
        if len(hits) != 1:
            raise KeyError(label)
        i = hits[0]
    return i


class DataArray:
    def __init__(self, values, dims, coords):
        self.values = np.asarray(values)
        self.dims = tuple(dims)
        self.coords = {d: coords[d] for d in dims}
        assert self.values.shape == tuple(len(coords[d]) for d in dims)

    def __getattr__(self, name):
        coords = self.__dict__.get("coords", {})
        if name in coords:
            return Coord(name, coords[name])
        raise AttributeError(name)

    @property
    def size(self):
        return self.values.size

    def compute(self):
        return self

    def load(self):
        return self

    def __float__(self):
        return float(self.values)

    def sel(self, indexers=None, method=None, **kw):
        idx = dict(indexers or {}, **kw)
        v, dims, coords = self.values, list(self.dims), dict(self.coords)
        for name, label in idx.items():
            if name not in dims:
                raise KeyError(name)
            ax = dims.index(name)
            i = _label_index(coords[name], label, method)
            v = np.take(v, i, axis=ax)
            dims.pop(ax)
            coords.pop(name)
        return DataArray(v, dims, coords)

    def where(self, mask, drop=False):
        assert drop
        m = mask._expand(self.dims) if all(d in self.dims for d in mask.dims) else None
        assert m is not None
        m = np.broadcast_to(m, self.values.shape)
        v = np.where(m, self.values, np.nan).astype(self.values.dtype)
        coords = dict(self.coords)
        for ax, d in enumerate(self.dims):  # drop the labels along each dim where the mask is False everywhere (order kept)
            keep = np.nonzero(m.any(axis=tuple(a for a in range(m.ndim) if a != ax)))[0]
            v = np.take(v, keep, axis=ax)
            m = np.take(m, keep, axis=ax)
            coords[d] = np.asarray(coords[d])[keep] if isinstance(coords[d], np.ndarray) else [coords[d][k] for k in keep]
        return DataArray(v, self.dims, coords)

    def min(self, skipna=True):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            return DataArray(np.nanmin(self.values), (), {})

    def mean(self, dim):
        ax = self.dims.index(dim)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            v = np.nanmean(self.values, axis=ax)
        return DataArray(v, [d for d in self.dims if d != dim], {d: c for d, c in self.coords.items() if d != dim})


class Dataset:
    def __init__(self, data_vars):
        self.data_vars = dict(data_vars)

    @property
    def dims(self):
        out = {}
        for da in self.data_vars.values():
            for d in da.dims:
                out[d] = len(da.coords[d])
        return out

    def __getitem__(self, name):
        return self.data_vars[name]

    def sel(self, indexers=None, **kw):
        idx = dict(indexers or {}, **kw)
        out = {}
        for name, da in self.data_vars.items():
            mine = {k: v for k, v in idx.items() if k in da.dims}
            out[name] = da.sel(mine) if mine else da
        return Dataset(out)

    def mean(self, dim):
        return Dataset({k: (da.mean(dim) if dim in da.dims else da) for k, da in self.data_vars.items()})


# ---- the reference's functions ----------------------------------------------------------------------------------------------
def reference_functions():
    names = {"round_to_grid", "select_box", "find_local_minimum", "track_first_n_steps"}
    tree = ast.parse(open(REF).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == names
    consts = [n for n in tree.body if isinstance(n, ast.Assign) and any(getattr(t, "id", "") in ("GRID_RES", "NEIGHBOR_DEG") for t in n.targets)]
    assert len(consts) == 2
    ns = {"np": np, "timedelta": timedelta, "warnings": warnings, "xr": None}
    exec(compile(ast.Module(body=consts + body, type_ignores=[]), REF, "exec"), ns)
    return ns


# ---- synthetic fields -------------------------------------------------------------------------------------------------------
def lows(T, centres, depth, radius, background, rng=None, noise=0.0, cut=4.0, lat=LAT, lon=LON):
    """(T, H, W) float32: background + Gaussian lows moving along `centres` [(T, 2) per low], noise inside their support;
    rounded to whole units"""
    la, lo = lat[:, None], lon[None, :]
    out = np.full((T, lat.size, lon.size), background, dtype=np.float64)
    support = np.zeros(out.shape, dtype=bool)
    for path, d, r in zip(centres, depth, radius):
        for t in range(T):
            c_la, c_lo = path[t]
            dlo = (lo - c_lo + 180) % 360 - 180
            d2 = ((la - c_la) ** 2 + dlo**2) / r**2
            out[t] -= np.where(d2 < cut**2, d * np.exp(-0.5 * d2), 0.0)
            support[t] |= d2 < cut**2
    if noise:  # inside the lows' support only: the flat background compresses to nothing
        out += np.where(support, rng.standard_normal(out.shape) * noise, 0.0)
    return np.round(out).astype(np.float32)


def path(start, velocity, T):
    return [(start[0] + velocity[0] * t, (start[1] + velocity[1] * t) % 360) for t in range(T)]


def make_dataset(t0, lat, lon, mslp, z700=None, lsm=None, members=None):
    """the layout latent_ens_to_xarr builds: (idx,) time, prediction_timedelta, [level,] latitude, longitude"""
    T = mslp.shape[-3]
    coords = {"time": [t0], "prediction_timedelta": [timedelta(hours=6 * k) for k in range(T)], "level": [700], "latitude": lat,
              "longitude": lon}
    lead = ("time", "prediction_timedelta")
    if members is not None:
        coords["idx"] = list(range(members))
        lead = ("idx",) + lead
    v = {"mean_sea_level_pressure": DataArray(mslp[..., None, :, :, :] if members is None else mslp[:, None], lead + ("latitude", "longitude"), coords)}
    if z700 is not None:
        z = z700[None, :, None] if members is None else z700[:, None, :, None]
        v["geopotential"] = DataArray(z, lead + ("level", "latitude", "longitude"), coords)
    if lsm is not None:
        v["land_sea_mask"] = DataArray(lsm, ("latitude", "longitude"), coords)
    return Dataset(v)


def main():
    ns = reference_functions()
    rng = np.random.default_rng(20181001)
    t0 = datetime(2018, 10, 1, 0)
    out = {"lat": LAT, "lon": LON}

    def dataset(mslp, z700=None, lsm=None, members=None):
        return make_dataset(t0, LAT, LON, mslp, z700, lsm, members)

    # -- tracks ---------------------------------------------------------------------------------------------------------------
    cases = []
    T = 9
    # 0: crossing 0/360 eastward near 15N
    cases.append(dict(mslp=lows(T, [path((15.0, 352.0), (0.6, 2.1), T)], [2500], [2.5], 101300), start=(15.2, 352.3), boxes=[7, 4, 1]))
    # 1: raw_lon0 rounding to 360.0, low drifting west across 0
    cases.append(dict(mslp=lows(T, [path((-20.0, 2.0), (-0.4, -1.6), T)], [3000], [3.0], 101000), start=(-19.6, 359.4), boxes=[7, 4, 1]))
    # 2: near the north edge
    cases.append(dict(mslp=lows(T, [path((86.0, 100.0), (0.5, 3.0), T)], [1800], [2.0], 100900), start=(86.4, 100.2), boxes=[7, 4, 1]))
    # 3: at -88.5, the southernmost row, and below it
    cases.append(dict(mslp=lows(T, [path((-87.0, 200.0), (-0.3, -4.0), T)], [2200], [2.5], 99800), start=(-88.6, 199.0), boxes=[7, 4, 1]))
    # 4: inner sizes [7, 5, 1] (half-boxes off the grid), two lows competing
    cases.append(dict(mslp=lows(T, [path((25.0, 130.0), (0.9, -1.3), T), path((29.0, 124.0), (0.2, 0.5), T)], [2000, 2600], [2.0, 3.5], 101200),
                      start=(25.3, 130.6), boxes=[7, 5, 1]))
    # 5: inner sizes [6, 3, 0]: half-boxes on the grid, so the edge drop fires; noisy field
    cases.append(dict(mslp=lows(T, [path((-12.0, 60.0), (-1.1, 1.4), T)], [900], [2.0], 101000, rng=rng, noise=40.0, cut=6.0),
                      start=(-12.0, 60.0), boxes=[6, 3, 0]))
    # 6: plateaus of equal minima (coarse rounding), tie order
    pl = lows(T, [path((10.0, 300.0), (0.75, -1.5), T)], [60], [4.0], 1000, cut=8.0)
    pl = (np.round(pl / 10) * 10).astype(np.float32)
    cases.append(dict(mslp=pl, start=(10.0, 300.0), boxes=[7, 4, 1]))
    # 7: a NaN patch in the path of the low
    nanf = lows(T, [path((40.0, 20.0), (-0.8, 1.7), T)], [2400], [2.5], 101100)
    nanf[:, 85:89, 14:19] = np.nan
    nanf[5:, 80:84, 16:20] = np.nan
    cases.append(dict(mslp=nanf, start=(40.1, 19.8), boxes=[7, 4, 1]))
    # 8: enforce_msl=False: land-sea mask + Z700; the MSLP low fades out half way, Z700 carries on
    la, lo = LAT[:, None], LON[None, :]
    lsm = (((la - 30) ** 2 + ((lo - 262 + 180) % 360 - 180) ** 2) < 40).astype(np.float32)  # an island the track crosses
    m8 = lows(T, [path((27.0, 255.0), (0.7, 1.6), T)], [2000, ], [2.5], 101000)
    m8[5:] = 101000.0  # flat: no move from MSLP in the late steps
    z8 = lows(T, [path((27.5, 255.5), (0.7, 1.5), T)], [300], [3.0], 30000, rng=rng, noise=2.0)
    cases.append(dict(mslp=m8, z700=z8, lsm=lsm, start=(27.0, 255.0), boxes=[7, 4, 1], enforce_msl=False))
    # 9: enforce_msl=False with [6, 3, 0] and the wrap
    z9 = lows(T, [path((-5.0, 357.0), (0.3, 1.2), T)], [250], [2.5], 29800)
    m9 = lows(T, [path((-5.0, 357.0), (0.3, 1.2), T)], [1500], [2.5], 100800)
    m9[:, 50:70, :] = np.nan  # MSLP unusable around the track: Z700 decides
    lsm9 = np.zeros_like(lsm)
    lsm9[:, 235:] = 1.0
    cases.append(dict(mslp=m9, z700=z9, lsm=lsm9, start=(-5.1, 356.9), boxes=[6, 3, 0], enforce_msl=False))

    for i, c in enumerate(cases):
        em = c.get("enforce_msl", True)
        ds = dataset(c["mslp"], c.get("z700"), c.get("lsm"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            trk = ns["track_first_n_steps"](t0, c["start"][0], c["start"][1], ds=ds, n_steps=T - 1, inner_box_sizes=c["boxes"], enforce_msl=em)
        out[f"t{i}_mslp"] = c["mslp"]
        if not em:
            out[f"t{i}_z700"], out[f"t{i}_lsm"] = c["z700"], c["lsm"]
        out[f"t{i}_start"] = np.array(c["start"], dtype=np.float64)
        out[f"t{i}_boxes"] = np.array(c["boxes"], dtype=np.int32)
        out[f"t{i}_enforce_msl"] = np.array(int(em))
        out[f"t{i}_track"] = np.array([(la, lo) for _, la, lo in trk], dtype=np.float64)
        assert [t for t, _, _ in trk] == [t0 + timedelta(hours=6 * k) for k in range(T)]
    out["n_tracks"] = np.array(len(cases))

    # -- ensemble: member tracks and the mean track ----------------------------------------------------------------------------
    E, T = 4, 7
    mem = np.stack([lows(T, [path((18.0 + 0.5 * e, 140.0 - e), (0.6 + 0.1 * e, -1.4 + 0.2 * e), T)], [2000 + 200 * e], [2.5], 101000,
                         rng=rng, noise=3.0) for e in range(E)])
    mem[1, :, 70:74, 88:92] = np.nan  # a NaN in one member: the mean skips it
    mem[:, 2, 71, 90] = np.nan  # NaN in every member at one point: the mean is NaN there
    ds = dataset(mem, members=E)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        ens = [ns["track_first_n_steps"](t0, 18.2, 139.9, ds=ds, ens_member=e, n_steps=T - 1) for e in range(E)]
        mean_ds = ds.mean(dim="idx")
        mean_trk = ns["track_first_n_steps"](t0, 18.2, 139.9, ds=mean_ds, n_steps=T - 1)
    out["ens_members"] = mem
    out["ens_start"] = np.array([18.2, 139.9])
    out["ens_mean_field"] = mean_ds["mean_sea_level_pressure"].values[0]
    out["ens_tracks"] = np.array([[(la, lo) for _, la, lo in trk] for trk in ens], dtype=np.float64)
    out["ens_mean_track"] = np.array([(la, lo) for _, la, lo in mean_trk], dtype=np.float64)

    # -- single find_local_minimum queries -------------------------------------------------------------------------------------
    qf = [cases[0]["mslp"][3], cases[5]["mslp"][4], pl[2], nanf[6], cases[3]["mslp"][2]]
    grad = (np.arange(LON.size, dtype=np.float32)[None, :] * 3 + np.arange(LAT.size, dtype=np.float32)[:, None]).astype(np.float32)
    qf.append(grad)  # a monotone field: the minimum of every box lies on its edge -> None
    allnan = np.full_like(grad, np.nan)
    allnan[:, :120] = 5.0
    qf.append(allnan)
    qfields = np.stack(qf).astype(np.float32)
    queries = []
    for f in range(len(qf)):
        for _ in range(6):
            la0 = round_to_grid_py(rng.uniform(-92, 92))
            lo0 = round_to_grid_py(rng.uniform(-1, 361))
            queries.append((f, la0, lo0, int(rng.choice([0, 1, 3, 4, 5, 6, 7, 12, 30]))))
    queries += [(0, 17.0, 354.0, 7), (0, 17.0, 0.0, 4), (0, 120.0, 10.0, 7), (1, -12.0, 60.0, 6), (1, -13.5, 61.5, 3), (1, -12.0, 60.0, 0),
                (2, 12.0, 297.0, 7), (2, 12.0, 297.0, 1), (3, 35.5, 29.5, 4), (4, -88.5, 190.5, 7), (4, -90.0, 360.0, 4), (5, 10.5, 180.0, 7),
                (6, 0.0, 270.0, 4), (6, 0.0, 180.0, 7), (6, 0.0, 358.5, 5), (0, 89.0, 359.9, 3)]
    res = []
    for f, la0, lo0, inner in queries:
        ds = Dataset({"v": DataArray(qfields[f][None], ("time", "latitude", "longitude"), {"time": [t0], "latitude": LAT, "longitude": LON})})
        r = ns["find_local_minimum"](ds, "v", t0, (la0, lo0), inner)
        res.append((1, r[0], r[1], r[2]) if r else (0, 0.0, 0.0, 0.0))
    out["q_fields"] = qfields
    out["q_field_idx"] = np.array([q[0] for q in queries], dtype=np.int32)
    out["q_center"] = np.array([(q[1], q[2]) for q in queries], dtype=np.float64)
    out["q_inner"] = np.array([q[3] for q in queries], dtype=np.int32)
    out["q_found"] = np.array([r[0] for r in res], dtype=np.int32)
    out["q_latlon"] = np.array([(r[1], r[2]) for r in res], dtype=np.float64)
    out["q_value"] = np.array([r[3] for r in res], dtype=np.float32)
    # round_to_grid's half-to-even rule, from the reference function itself
    rv = np.array([0.75, 2.25, 3.75, -0.75, -2.25, 359.25, 359.4, 359.99, -88.6, 90.4, 0.0, 1.4999, -134.25], dtype=np.float64)
    out["round_in"], out["round_out"] = rv, np.array([ns["round_to_grid"](v) for v in rv])
    path_out = os.path.join(HERE, "track_ref.npz")
    np.savez_compressed(path_out, **out)
    print(f"wrote {path_out}: {os.path.getsize(path_out) / 1e6:.2f} MB, {len(cases)} tracks, {E} members + mean, {len(queries)} queries "
          f"({int(out['q_found'].sum())} found)")


def round_to_grid_py(v):
    return float(np.round(v / 1.5) * 1.5)


# ---- the edge fixture: custom grids, off-grid centres, exact ties -----------------------------------------------------------
EDGE_SEED = 20260117  # change the seed, never a condition, if the reference alone does not meet the assertions of edges()
G6_FORMULAS = [(7919, 104729, 50), (0, 0, 1), (1, 3, 10 ** 9)]  # ((r * a + c * b) % m): plateaus of 50 values; constant 0; monotone


def edge_grids(rng):
    g3_lat, g3_lon = np.sort(rng.uniform(-89, 89, 37)), np.sort(rng.uniform(0, 360, 53))
    assert np.all(np.diff(g3_lat) > 0) and np.all(np.diff(g3_lon) > 0)
    return {
        "G1": (LAT, LON),
        "G2": (np.arange(-10.0, 10.5, 1.0), np.arange(100.0, 140.5, 1.0)),  # regional: does not close the circle
        "G3": (g3_lat, g3_lon),  # irregular, non-dyadic
        "G4a": (np.array([12.0]), LON),  # one row
        "G4b": (LAT, np.array([181.5])),  # one column
        "G5": (LAT, np.arange(0, 360 + 1e-6, 1.5)),  # 0 and 360 both present
        "G6": (np.linspace(-60, 60, 1024), 0.25 * np.arange(1024)),  # the cap
    }


def edge_fields(lat, lon, rng):
    """small integers as fp32: constant; plateaus of four values; monotone; plateaus with an all-NaN patch -> (fields, patch centre)"""
    H, W = lat.size, lon.size
    f1 = rng.integers(0, 4, (H, W)).astype(np.float32)
    f2 = (np.arange(W, dtype=np.float32)[None, :] * 3 + np.arange(H, dtype=np.float32)[:, None]).astype(np.float32)
    f3 = f1.copy()
    r0, c0, nr, nc = H // 3, W // 3, max(1, H // 4), max(1, W // 4)
    f3[r0 : r0 + nr, c0 : c0 + nc] = np.nan
    return np.stack([np.full((H, W), 7.0, np.float32), f1, f2, f3]), (float(lat[r0 + nr // 2]), float(lon[c0 + nc // 2]))


def edge_centres(lat, lon, rng, dyadic):
    """(kind, lat0, lon0): on the grid, on cell centres, on the seam (unwrapped too), beside the first and last row, dyadic multiples of
    1/64 off the grid, outside the grid.  On a non-dyadic grid the cell centres are moved to the next multiple of 1/64, so that no two
    candidates are ALMOST equally far (the key precondition)."""
    H, W = lat.size, lon.size
    i, j = H // 2, W // 2
    snap = (lambda v: float(v)) if dyadic else (lambda v: float(np.floor(v * 64) / 64))
    mla, mlo = snap((lat[i] + lat[min(i + 1, H - 1)]) / 2), snap((lon[j] + lon[min(j + 1, W - 1)]) / 2)
    gla, glo = float(lat[i]), float(lon[j])
    out = [("grid", gla, glo), ("cell", mla, mlo), ("cell", mla, glo), ("cell", gla, mlo),
           ("seam", 0.75 if lat[0] < 0.75 < lat[-1] else mla, 359.25), ("seam", mla, -0.75), ("seam", mla, 360.75), ("seam", gla, 359.25),
           ("seam", gla, 0.0), ("seam", mla, 360.0),
           ("row", float(lat[0]) - 0.75, glo), ("row", snap(float(lat[0]) + 0.75), mlo), ("row", float(lat[-1]) + 0.75, glo),
           ("row", snap(float(lat[-1]) - 0.75), mlo)]
    for _ in range(6):
        out.append(("dyadic", float(np.round(rng.uniform(lat[0] - 2, lat[-1] + 2) * 64) / 64), float(np.round(rng.uniform(lon[0] - 2, lon[-1] + 2) * 64) / 64)))
    out += [("outside", 95.0, glo), ("outside", -95.0, glo), ("outside", gla, -3.0), ("outside", gla, 363.0), ("outside", gla, 720.5)]
    return out


def edge_queries(name, lat, lon, patch, rng, dyadic):
    """(field, lat0, lon0, inner).  Fields: 0 constant, 1 plateaus, 2 monotone, 3 plateaus with a NaN patch (G6: the three formulas)"""
    cs = edge_centres(lat, lon, rng, dyadic)
    q = []
    if name == "G6":  # inner 0 and 1 only: a few hundred candidates per search
        keep = [c for c in cs if c[0] in ("grid", "cell", "row")][:6] + [c for c in cs if c[0] == "dyadic"][:2] + [c for c in cs if c[0] == "outside"][:3]
        for k, (_, la, lo) in enumerate(keep):
            q += [(1, la, lo, 1), (0, la, lo, k % 2)]
        q += [(1, keep[1][1], keep[1][2], 0), (2, keep[0][1], keep[0][2], 1), (2, keep[1][1], keep[1][2], 0)]
        return q
    for kind, la, lo in cs:
        q += [(0, la, lo, 1), (0, la, lo, 12)]
        if kind != "outside":
            q += [(0, la, lo, 0), (1, la, lo, 5), (1, la, lo, 1)]
        if kind in ("dyadic", "seam"):
            q += [(1, la, lo, 12), (1, la, lo, 30), (3, la, lo, 5), (0, la, lo, 30)]
    gla, glo = float(lat[lat.size // 2]), float(lon[lon.size // 2])
    q += [(2, gla, glo, 5), (2, gla, glo, 12), (2, gla, glo, 0), (2, gla, glo, 30)]
    q += [(3, patch[0], patch[1], 0), (3, patch[0], patch[1], 5), (3, patch[0], patch[1], 30)]
    return q


def edges():
    """tests/golden/track_edge_ref.npz: find_local_minimum and track_first_n_steps of the reference on custom grids (edge_grids), with
    centres off the grid and fields of small integers, so that plateaus and exact ties are the rule.  Asserts that every grid has both
    outcomes, that enough searches are decided by the visiting order alone, and the two key preconditions of tests/track_oracle.py
    (key_check) on every search.  track_ref.npz is not touched."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from tests import track_oracle as O

    ns = reference_functions()
    rng = np.random.default_rng(EDGE_SEED)
    t0 = datetime(2018, 10, 1, 0)
    grids = edge_grids(rng)
    out = {"grid_names": np.array(list(grids)), "G6_formulas": np.array(G6_FORMULAS, dtype=np.int64)}
    Q = {k: [] for k in ("grid", "field", "center", "inner", "found", "latlon", "value", "ties", "wrapped")}
    n_tie = n_tie_wrapped = 0
    for gi, (name, (lat, lon)) in enumerate(grids.items()):
        dyadic = O.is_dyadic(lat, lon)
        assert dyadic == (name not in ("G3", "G6")), name
        out[f"{name}_lat"], out[f"{name}_lon"] = lat, lon
        if name == "G6":
            fields, patch = np.stack([O.formula_field(lat.size, lon.size, *f) for f in G6_FORMULAS]), None
        else:
            fields, patch = edge_fields(lat, lon, rng)
            out[f"{name}_fields"] = fields
        queries = edge_queries(name, lat, lon, patch, rng, dyadic)
        found = ties = wrapped_ties = 0
        for f, la0, lo0, inner in queries:
            ds = Dataset({"v": DataArray(fields[f][None], ("time", "latitude", "longitude"), {"time": [t0], "latitude": lat, "longitude": lon})})
            r = ns["find_local_minimum"](ds, "v", t0, (la0, lo0), inner)
            fin = O.survivors(fields[f], (la0, lo0), inner, lat, lon)
            n_min, problem = O.key_check(fin, (la0, lo0), dyadic and O.is_dyadic(la0, lo0))
            assert problem is None, (name, f, la0, lo0, inner, problem)
            assert (r is None) == (not fin) and (r is None or (r[0], r[1], r[2]) in fin), (name, f, la0, lo0, inner)
            half_o = (inner + 3.0) / 2
            wrapped = int((lo0 - half_o) % 360 > (lo0 + half_o) % 360)
            for k, v in zip(Q, (gi, f, (la0, lo0), inner, int(r is not None), (r[0], r[1]) if r else (0.0, 0.0), r[2] if r else 0.0, n_min, wrapped)):
                Q[k].append(v)
            found += r is not None
            ties += n_min >= 2
            wrapped_ties += n_min >= 2 and wrapped
        print(f"{name}: {lat.size} x {lon.size}, {len(queries)} queries, {found} found / {len(queries) - found} None, {ties} tie cases, "
              f"{wrapped_ties} of them in a wrapped box")
        assert 0 < found < len(queries), name  # both outcomes on every grid
        n_tie, n_tie_wrapped = n_tie + ties, n_tie_wrapped + wrapped_ties
    assert n_tie >= 12 and n_tie_wrapped >= 3, (n_tie, n_tie_wrapped)
    for k, dt in (("grid", np.int32), ("field", np.int32), ("center", np.float64), ("inner", np.int32), ("found", np.int32), ("latlon", np.float64),
                  ("value", np.float32), ("ties", np.int32), ("wrapped", np.int32)):
        out[f"q_{k}"] = np.array(Q[k], dtype=dt)
    # the constant field around (0.75, 359.25) with inner 1: four candidates equally far, the seam's small longitude visited first
    hit = [i for i in range(len(Q["grid"])) if Q["grid"][i] == 0 and Q["field"][i] == 0 and Q["center"][i] == (0.75, 359.25) and Q["inner"][i] == 1]
    assert hit and Q["latlon"][hit[0]] == (0.0, 0.0) and Q["ties"][hit[0]] == 4

    # -- tracks (T = 4) ---------------------------------------------------------------------------------------------------------
    T = 4
    tracks = []
    lat, lon = grids["G2"]
    la, lo = lat[:, None], lon[None, :]
    lsm2 = ((la >= 2) & (lo >= 122)).astype(np.float32)  # the start (1.5, 121.5) is the midpoint of four cells: only (2, 122) is land
    m2 = lows(T, [path((2.0, 122.0), (0.9, 1.3), T)], [30], [2.0], 50, lat=lat, lon=lon)
    z2 = lows(T, [path((1.0, 121.0), (-1.2, -0.8), T)], [20], [2.0], 90, lat=lat, lon=lon)
    tracks.append(dict(grid="G2", mslp=m2, start=(1.4, 121.6), boxes=[7, 4, 1]))
    tracks.append(dict(grid="G2", mslp=m2, z700=z2, lsm=lsm2, start=(1.4, 121.6), boxes=[7, 4, 1], enforce_msl=False))
    lat, lon = grids["G3"]
    m3 = lows(T, [path((20.0, 150.0), (4.0, 6.0), T)], [40], [9.0], 60, lat=lat, lon=lon)
    z3 = lows(T, [path((22.0, 148.0), (-3.0, 5.0), T)], [25], [9.0], 80, lat=lat, lon=lon)
    lsm3 = (rng.random((lat.size, lon.size)) < 0.5).astype(np.float32)
    tracks.append(dict(grid="G3", mslp=m3, start=(20.3, 150.2), boxes=[30, 12, 5]))
    tracks.append(dict(grid="G3", mslp=m3, z700=z3, lsm=lsm3, start=(20.3, 150.2), boxes=[30, 12, 5], enforce_msl=False))
    lat, lon = grids["G5"]
    m5 = lows(T, [path((15.0, 355.0), (0.6, 3.0), T)], [30], [2.5], 50, lat=lat, lon=lon)
    tracks.append(dict(grid="G5", mslp=m5, start=(15.2, 355.3), boxes=[7, 4, 1]))
    for i, c in enumerate(tracks):
        lat, lon = grids[c["grid"]]
        em = c.get("enforce_msl", True)
        ds = make_dataset(t0, lat, lon, c["mslp"], c.get("z700"), c.get("lsm"))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            trk = ns["track_first_n_steps"](t0, c["start"][0], c["start"][1], ds=ds, n_steps=T - 1, inner_box_sizes=c["boxes"], enforce_msl=em)
        dyadic = O.is_dyadic(lat, lon)

        def search(field, center, inner, la_, lo_):
            _, problem = O.key_check(O.survivors(field, center, inner, la_, lo_), center, dyadic)
            assert problem is None, (i, center, inner, problem)
            return O.find_local_minimum(field, center, inner, la_, lo_)

        O.track_first_n_steps(t0, c["start"][0], c["start"][1], c["mslp"], T - 1, c["boxes"], em, c.get("z700"), c.get("lsm"), lat, lon, search=search)
        out[f"t{i}_grid"] = np.array(c["grid"])
        out[f"t{i}_mslp"] = c["mslp"]
        if not em:
            out[f"t{i}_z700"], out[f"t{i}_lsm"] = c["z700"], c["lsm"]
        out[f"t{i}_start"] = np.array(c["start"], dtype=np.float64)
        out[f"t{i}_boxes"] = np.array(c["boxes"], dtype=np.int32)
        out[f"t{i}_enforce_msl"] = np.array(int(em))
        out[f"t{i}_track"] = np.array([(la_, lo_) for _, la_, lo_ in trk], dtype=np.float64)
        moved = int((np.diff(out[f"t{i}_track"], axis=0) != 0).any(axis=1).sum())
        print(f"track {i} on {c['grid']} (enforce_msl={em}): moved in {moved} of {T - 1} steps: {out[f't{i}_track'].tolist()}")
    assert out["t4_track"][0, 1] > 300 and out["t4_track"][-1, 1] < 60  # the G5 track crosses 360 -> 0
    assert not np.array_equal(out["t0_track"], out["t1_track"])  # the mask at the midpoint start decides (pandas' tie rule)
    out["n_tracks"] = np.array(len(tracks))
    path_out = os.path.join(HERE, "track_edge_ref.npz")
    np.savez_compressed(path_out, **out)
    nq = len(Q["grid"])
    print(f"wrote {path_out}: {os.path.getsize(path_out) / 1e3:.0f} kB, {nq} queries ({int(out['q_found'].sum())} found), {n_tie} tie cases "
          f"({n_tie_wrapped} in a wrapped box), {len(tracks)} tracks")
    assert os.path.getsize(path_out) < 200e3


if __name__ == "__main__":
    if "--edges" in sys.argv[1:]:
        edges()
    else:
        main()
