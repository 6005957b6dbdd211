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
    return closest(survivors(field, center, inner_deg, lat, lon), center)


def closest(finals, center):
    """the reference's pick among the surviving minima: Python's min keeps the first of equal keys"""
    if not finals:
        return None
    lat0, lon0 = center
    return min(finals, key=lambda t: (t[0] - lat0) ** 2 + (((t[1] - lon0 + 180) % 360 - 180) ** 2))


def key_terms(cand, center):
    """the two differences whose squares form the distance key of candidate (la, lo, ...) around `center`"""
    return cand[0] - center[0], (cand[1] - center[1] + 180) % 360 - 180


def survivors(field, center, inner_deg, lat=None, lon=None):
    """the local minima of the outer box that are not on its edge, in the reference's visiting order (rows ascending, then the
    columns `where(..., drop=True)` keeps: ascending, so the small longitudes of a wrapped box come first)"""
    if lat is None:
        lat, lon = grid()
    lat0, lon0 = center
    outer = inner_deg + NEIGHBOR_DEG * 2
    half_o = outer / 2
    half_i = inner_deg / 2
    lat_lo, lat_hi = lat0 - half_o, lat0 + half_o
    lon_s, lon_e = (lon0 - half_o) % 360, (lon0 + half_o) % 360
    rows, cols = select_box(lat, lon, lat_lo, lat_hi, lon_s, lon_e)
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
    return finals


def is_dyadic(*values):
    """every value is a multiple of 2**-20 below 4096 in magnitude (a grid or centre of this kind is "dyadic"); that the squares of
    the differences are exact is checked per search (key_check), not assumed from this"""
    v = np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in values])
    return bool(np.all(np.isfinite(v)) and np.all(v * 2.0 ** 20 == np.round(v * 2.0 ** 20)) and np.all(np.abs(v) < 4096))


def key_check(finals, center, dyadic):
    """The builder preconditions of tests/golden/track_edge_ref.npz on one search -> (number of survivors sharing the minimal key,
    None or a message).  dyadic: every difference d entering a key has d * d == d ** 2 (the kernel's key is the reference's, bit for
    bit).  Otherwise: the winning key is exactly equal to a runner-up's under both d * d and d ** 2, or more than 4 ulp away from it
    (the kernel's d * d is within 2 ulp of d ** 2 per key, so it cannot change the winner)."""
    if not finals:
        return 0, None
    terms = [key_terms(c, center) for c in finals]
    kp = [a ** 2 + b ** 2 for a, b in terms]
    km = [a * a + b * b for a, b in terms]
    best = min(kp)
    if dyadic:
        for a, b in terms:
            if a * a != a ** 2 or b * b != b ** 2:
                return 0, f"d * d != d ** 2 for a term of {(a, b)}"
    else:
        w = kp.index(best)
        for i in range(len(finals)):
            same = kp[i] == best and km[i] == km[w]
            if not same and not abs(kp[i] - best) > 4 * np.spacing(best):
                return 0, f"keys {kp[i]!r} and {best!r} are within 4 ulp and not identical"
    return sum(1 for k in kp if k == best), None


def formula_field(H, W, a, b, m):
    """the (H, W) fp32 plane ((r * a + c * b) % m) of small integers that both the fixture's builder and the tests rebuild"""
    r, c = np.arange(H, dtype=np.int64)[:, None], np.arange(W, dtype=np.int64)[None, :]
    return ((r * int(a) + c * int(b)) % int(m)).astype(np.float32)


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
                        land_sea_mask=None, lat=None, lon=None, return_codes=False, search=None, round_start=True):
    """mslp / z700: (T, H, W) numpy float32 frames, frame k = lead 6 h * k.  -> [(time, lat, lon), ...] (and the codes of
    ldc_track_storms: 0 stayed, 1 + k moved on MSLP with box k, 1 + nbox + k on Z700).  round_start=False: the start as given, which is
    what ldc_track_storms takes (the reference rounds it to the 1.5 degree grid first)"""
    if lat is None:
        lat, lon = grid()
    search = search or find_local_minimum  # a wrapper may record the searches a track makes
    lat0, lon0 = (round_to_grid(raw_lat0), round_to_grid(raw_lon0)) if round_start else (float(raw_lat0), float(raw_lon0))
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
                res = search(mslp[step], current, inner, lat, lon)
                if res and ((prev[0] != res[0]) or (prev[1] != res[1])):
                    current, code = (res[0], res[1]), 1 + k
                    break
        if not code and not enforce_msl:
            for k, inner in enumerate(inner_box_sizes):
                res = search(z700[step], current, inner, lat, lon)
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
