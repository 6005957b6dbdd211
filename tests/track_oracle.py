"""Plain numpy restatement of the reference's cyclone tracker (ladcast/evaluate/track.py:151-335) without xarray: the CPU yardstick
for the GPU tracker on many random cases that tests/golden/track_ref.npz cannot hold.  It is itself pinned to that fixture
(tests/test_track_cpu.py).  Coordinates are Python floats, so `%`, `abs` and `**` are Python's own.  Only numpy is imported here:
this module is loaded when the suite is collected."""
from datetime import timedelta

import numpy as np

NEIGHBOR_DEG = 1.5


def grid():
    return np.arange(-88.5, 90 + 1e-6, 1.5), np.arange(0, 358.5 + 1e-6, 1.5)


def round_to_grid(val, resolution=1.5):
    return float(np.round(val / resolution) * resolution)


def select_box(lat, lon, lat_lo, lat_hi, lon_start, lon_end):
    """the row and column indices `where(mask, drop=True)` keeps, in ascending coordinate order"""
    rows = np.nonzero((lat >= min(lat_lo, lat_hi)) & (lat <= max(lat_lo, lat_hi)))[0]
    if lon_start <= lon_end:
        cols = np.nonzero((lon >= lon_start) & (lon <= lon_end))[0]
    else:
        cols = np.nonzero((lon >= lon_start) | (lon <= lon_end))[0]
    return rows, cols


def find_local_minimum(field, center, inner_deg, lat=None, lon=None):
    """field: (H, W) float32 numpy plane -> (la, lo, v) or None"""
    if lat is None:
        lat, lon = grid()
    lat0, lon0 = center
    outer = inner_deg + NEIGHBOR_DEG * 2
    half_o = outer / 2
    half_i = inner_deg / 2
    lat_lo, lat_hi = lat0 - half_o, lat0 + half_o
    lon_s, lon_e = (lon0 - half_o) % 360, (lon0 + half_o) % 360
    rows, cols = select_box(lat, lon, lat_lo, lat_hi, lon_s, lon_e)
    if rows.size * cols.size == 0:
        return None
    finals = []
    for r in rows:
        la = float(lat[r])
        for c in cols:
            lo = float(lon[c])
            v = float(field[r, c])
            nr, nc = select_box(lat, lon, la - half_i, la + half_i, (lo - half_i) % 360, (lo + half_i) % 360)
            if nr.size * nc.size == 0:
                continue
            block = field[np.ix_(nr, nc)]
            ok = ~np.isnan(block)
            m = float(block[ok].min()) if ok.any() else float("nan")
            if not v == m:
                continue
            if (abs(la - lat_lo) < 1e-6 or abs(la - lat_hi) < 1e-6 or abs((lo - lon_s) % 360) < 1e-6
                    or abs((lo - lon_e) % 360) < 1e-6):
                continue
            finals.append((la, lo, v))
    if not finals:
        return None
    return min(finals, key=lambda t: (t[0] - lat0) ** 2 + (((t[1] - lon0 + 180) % 360 - 180) ** 2))


def nearest_index(coord, x):
    """pandas' Index.get_indexer([x], method="nearest") on an ascending index: the pad / backfill neighbours, the left one only when
    strictly closer or when there is no right one; index -1 reads the last entry (tests/test_track_cpu.py holds it to pandas)"""
    n = coord.size
    pad = int(np.searchsorted(coord, x, side="right")) - 1
    bf = int(np.searchsorted(coord, x, side="left"))
    bf = -1 if bf == n else bf
    ld, rd = abs(coord[pad] - x), abs(coord[bf] - x)
    return pad if (ld < rd or bf == -1) else bf


def track_first_n_steps(t0, raw_lat0, raw_lon0, mslp, n_steps, inner_box_sizes=(7, 4, 1), enforce_msl=True, z700=None,
                        land_sea_mask=None, lat=None, lon=None, return_codes=False):
    """mslp / z700: (T, H, W) numpy float32 frames, frame k = lead 6 h * k.  -> [(time, lat, lon), ...] (and the codes of
    ldc_track_storms: 0 stayed, 1 + k moved on MSLP with box k, 1 + nbox + k on Z700)"""
    if lat is None:
        lat, lon = grid()
    lat0, lon0 = round_to_grid(raw_lat0), round_to_grid(raw_lon0)
    track = [(t0, lat0, lon0)]
    codes = []
    current = (lat0, lon0)
    nb = len(inner_box_sizes)
    for step in range(1, n_steps + 1):
        prev = current
        code = 0
        mval = 0 if enforce_msl else land_sea_mask[nearest_index(lat, current[0]), nearest_index(lon, current[1])]
        if mval < 0.5:
            for k, inner in enumerate(inner_box_sizes):
                res = find_local_minimum(mslp[step], current, inner, lat, lon)
                if res and ((prev[0] != res[0]) or (prev[1] != res[1])):
                    current, code = (res[0], res[1]), 1 + k
                    break
        if not code and not enforce_msl:
            for k, inner in enumerate(inner_box_sizes):
                res = find_local_minimum(z700[step], current, inner, lat, lon)
                if res and ((prev[0] != res[0]) or (prev[1] != res[1])):
                    current, code = (res[0], res[1]), 1 + nb + k
                    break
        codes.append(code)
        track.append((t0 + timedelta(hours=6 * step), *current))
    return (track, codes) if return_codes else track


def nanmean_members(x):
    """the reference's ds.mean(dim="idx") on float32 without bottleneck: np.nanmean over axis 0"""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(x, axis=0)
