"""Host reference of the sphere fields (`ladcast_amd.evaluate.derived`, `ldc_derive_sphere`: relative vorticity and divergence), numpy
only (a helper module, not a conftest).

Inputs are de-normalised in fp32 by `derived_refs.denorm` and widened to float64; every operation below is one IEEE double operation
in the order include/ladcast_hip.h states at ldc_derive_sphere, the result rounded once to fp32: a non-pole row of the device is
bit-equal to this.  The per-row constants come from `sphere_row_tables` (so kernel and reference share their bits); `row_tables` here
restates them from the formulas, independently, to check that function.  The pole-row sum is `math.fsum`, the correctly rounded sum."""
from __future__ import annotations

import math

import numpy as np

from tests.derived_refs import denorm

R_EARTH = 6_371_000.0
KINDS = ("vorticity", "divergence")


def row_tables(lat_deg, W):
    """c, q, r, pc (each (H,)) and k from the formulas, one row at a time with `math`"""
    lat = [float(v) for v in lat_deg]
    H = len(lat)
    phi = [math.radians(v) for v in lat]
    pole = [90.0 - abs(v) < 1e-6 for v in lat]
    c = [0.0 if pole[j] else math.cos(phi[j]) for j in range(H)]
    q = [1.0 / (phi[min(j + 1, H - 1)] - phi[max(j - 1, 0)]) for j in range(H)]
    r = [0.0 if pole[j] else 1.0 / (R_EARTH * c[j]) for j in range(H)]
    pc = [0.0] * H
    for j in range(H):
        if pole[j]:
            jp, s = (1 if j == 0 else H - 2), (1.0 if lat[j] > 0 else -1.0)
            pc[j] = s * c[jp] / (R_EARTH * (1.0 - s * math.sin(phi[jp])))
    return np.array(c), np.array(q), np.array(r), np.array(pc), 1.0 / (2.0 * (2.0 * math.pi / W))


def vorticity(a, b, tables, k):
    """zeta of (a, b): float64 arrays (..., H, W), already de-normalised and widened -> fp32 (..., H, W)"""
    c, q, r, pc = (np.asarray(t, dtype=np.float64) for t in tables)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    H, W = a.shape[-2:]
    out = np.empty(a.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(H):
            if r[j] == 0.0:
                jp = 1 if j == 0 else H - 2
                rows = a[..., jp, :].reshape(-1, W)
                sums = np.array([math.fsum(row) if np.isfinite(row).all() else float(np.sum(row)) for row in rows]).reshape(a.shape[:-2])
                out[..., j, :] = (sums / float(W) * pc[j]).astype(np.float32)[..., None]
                continue
            jn, js = min(j + 1, H - 1), max(j - 1, 0)
            dl = (np.roll(b[..., j, :], -1, axis=-1) - np.roll(b[..., j, :], 1, axis=-1)) * k
            dp = (a[..., jn, :] * c[jn] - a[..., js, :] * c[js]) * q[j]
            out[..., j, :] = ((dl - dp) * r[j]).astype(np.float32)
    return out


def field(kind, u, v, tables, k):
    """one sphere field of the de-normalised fp32 wind (u, v) -> fp32; divergence(u, v) = vorticity(-v, u)"""
    u, v = np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)
    if kind == "vorticity":
        return vorticity(u.astype(np.float64), v.astype(np.float64), tables, k)
    assert kind == "divergence"
    return vorticity((-v).astype(np.float64), u.astype(np.float64), tables, k)


def divergence_direct(u, v, tables, k):
    """the divergence written out on its own, 1 / (R cos) (du/dlambda + d(v cos)/dphi), the pole row the outward flux over the cap"""
    c, q, r, pc = (np.asarray(t, dtype=np.float64) for t in tables)
    u, v = np.asarray(u, dtype=np.float32).astype(np.float64), np.asarray(v, dtype=np.float32).astype(np.float64)
    H, W = u.shape[-2:]
    out = np.empty(u.shape, dtype=np.float32)
    for j in range(H):
        if r[j] == 0.0:
            jp = 1 if j == 0 else H - 2
            out[..., j, :] = np.float32(-(math.fsum(v[..., jp, :].reshape(-1))) / float(W) * pc[j])
            continue
        jn, js = min(j + 1, H - 1), max(j - 1, 0)
        dl = (np.roll(u[..., j, :], -1, axis=-1) - np.roll(u[..., j, :], 1, axis=-1)) * k
        dp = (v[..., jn, :] * c[jn] - v[..., js, :] * c[js]) * q[j]
        out[..., j, :] = ((dl + dp) * r[j]).astype(np.float32)
    return out


def derive(x, fields, axis, tables, k, mean=None, std=None, target_std=1.0):
    """x: fp32 array with the channels on `axis` and (H, W) last; fields: (name, kind, (u, v)[, scale]) -> the fields stacked on `axis`"""
    x = np.asarray(x, dtype=np.float32)

    def plane(ch):
        return denorm(np.take(x, ch, axis=axis), None if mean is None else float(mean[ch]), None if std is None else float(std[ch]), target_std)

    return np.stack([field(f[1], plane(int(f[2][0])), plane(int(f[2][1])), tables, k) for f in fields], axis=axis)


def pole_rows(tables):
    return [j for j, v in enumerate(np.asarray(tables[2])) if v == 0.0]


def pole_bound(a_row, pc_j, want):
    """what a pole value may differ by from the fsum reference: 1 fp32 ulp of it + (W - 1) 2^-53 sum|a_i| |pc| / W"""
    a_row = np.abs(np.asarray(a_row, dtype=np.float64))
    W = a_row.shape[-1]
    ulp = np.spacing(np.abs(np.asarray(want, dtype=np.float32))).astype(np.float64)
    return ulp + (W - 1) * 2.0 ** -53 * a_row.sum(axis=-1) * abs(float(pc_j)) / W
