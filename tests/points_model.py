"""The point-cloud contract ("Point clouds") restated in numpy: the checker of the splat renderer, of the
automatic radius and of the nearest-point snap.  It shares nothing with mvlm_amd/csrc/raster_points_math.h; the one thing it
imports is the oracle's view rotation.

A point: M v in float64, rounded to float32; window (x + 150) * (256 / 300) * 2^bits + 0.5, floored, in float32, on the 1/256
lattice; z = (500 - zv) / 1500.  Radius r model units -> R = floor(r * 256 / 300 * 256 + 0.5) steps, 192 <= R <= 2048.  Pixel
(i, j), centre (256 i + 128, 256 j + 128), is covered iff dx^2 + dy^2 <= R^2; its depth is z + float32(d2) * c, two float32
roundings, c = float32(r / 1500 / R^2); kept iff 0 <= depth <= 1.  Smallest depth wins, the higher id on ties.  Output: the
winner's colour bytes (white without), depth byte (256 - trunc(255 depth)) mod 256, white background, rows flipped, / 255."""
import math

import numpy as np

from oracle.estimator import view_rotation

SIZE = 256
R_MIN, R_MAX = 192, 2048
F = np.float32


def radius_steps(r: float) -> int:
    return int(math.floor(float(r) * 256.0 / 300.0 * 256.0 + 0.5))


def px_to_model(px: float) -> float:
    return float(px) * 300.0 / 256.0


def auto_radius(verts) -> float:
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    s = 0.0
    if len(v):
        ez, ey, ex = sorted(v.max(axis=0) - v.min(axis=0))
        s = math.sqrt(ex * ey / len(v))
    return min(max(1.25 * s, 0.75), 8.0) * 300.0 / 256.0


def rotations(transform_stack) -> np.ndarray:
    t = np.asarray(transform_stack)
    return np.stack([view_rotation(*t[i, :3]).ravel() for i in range(t.shape[0])]).astype(np.float64)


def transform(verts, m, bits: int = 8):
    """float32 [V,3], one rotation f64[9] -> (X, Y int64 lattice coordinates, z float32); finite points only."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    xv = ((m[0] * x + m[1] * y) + m[2] * z).astype(F)
    yv = ((m[3] * x + m[4] * y) + m[5] * z).astype(F)
    zv = ((m[6] * x + m[7] * y) + m[8] * z).astype(F)
    k, sub = F(256.0) / F(300.0), F(1 << bits)
    lim = F((1 << 22) >> (8 - bits))
    with np.errstate(over="ignore", invalid="ignore"):
        fx = np.clip(np.floor(((xv + F(150.0)) * k) * sub + F(0.5)), -lim, lim)
        fy = np.clip(np.floor(((yv + F(150.0)) * k) * sub + F(0.5)), -lim, lim)
        zz = (F(500.0) - zv) / F(1500.0)
    step = 256 >> bits
    return fx.astype(np.int64) * step, fy.astype(np.int64) * step, zz.astype(F)


def render(verts, transform_stack, radius=None, colors=None, subpixel_bits: int = 8) -> np.ndarray:
    """-> [N,256,256,4] float32, what render_device gives for the cloud."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    r = auto_radius(verts) if radius is None else float(radius)
    R = radius_steps(r)
    assert R_MIN <= R <= R_MAX, (r, R)
    c = F(r / 1500.0 / (float(R) * float(R)))
    rot = rotations(transform_stack)
    finite = np.isfinite(verts).all(axis=1)
    ids = np.nonzero(finite)[0].astype(np.uint64)
    good = verts[finite]
    w = 2 * (R // 256) + 3                       # a box of 2R + 1 steps holds at most this many centres
    off = np.arange(w, dtype=np.int64)
    out = np.empty((rot.shape[0], SIZE, SIZE, 4), np.float32)
    for n in range(rot.shape[0]):
        X, Y, z = transform(good, rot[n], subpixel_bits)
        i0 = -((-(X - R - 128)) // 256)          # the first centre at or right of X - R
        j0 = -((-(Y - R - 128)) // 256)
        i = (i0[:, None] + off[None, :])[:, None, :] + np.zeros((1, w, 1), np.int64)
        j = (j0[:, None] + off[None, :])[:, :, None] + np.zeros((1, 1, w), np.int64)
        dx, dy = 256 * i + 128 - X[:, None, None], 256 * j + 128 - Y[:, None, None]
        d2 = dx * dx + dy * dy
        with np.errstate(over="ignore", invalid="ignore"):
            zp = (z[:, None, None] + d2.astype(F) * c).astype(F)
            keep = (d2 <= R * R) & (i >= 0) & (i < SIZE) & (j >= 0) & (j < SIZE) & (zp >= F(0.0)) & (zp <= F(1.0))
        key = (zp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids)[:, None, None]
        plane = np.full(SIZE * SIZE, np.uint64(0xFFFFFFFFFFFFFFFF))
        np.minimum.at(plane, (j[keep] * SIZE + i[keep]), key[keep])
        plane = plane.reshape(SIZE, SIZE)
        hit = plane != np.uint64(0xFFFFFFFFFFFFFFFF)
        win = (np.uint64(0xFFFFFFFF) - (plane & np.uint64(0xFFFFFFFF))).astype(np.int64)
        zwin = np.where(hit, (plane >> np.uint64(32)).astype(np.uint32).view(F), F(1.0))
        depth = np.where(hit, (256 - (255.0 * zwin.astype(np.float64)).astype(np.int64)) & 255, 1)  # (far plane: 256 - 255)
        img = np.empty((SIZE, SIZE, 4), np.float32)
        rgb = np.full((SIZE, SIZE, 3), 255, np.int64)
        if colors is not None:
            rgb[hit] = np.asarray(colors, np.uint8).reshape(-1, 3)[win[hit]]
        img[..., :3] = rgb.astype(F) / F(255.0)
        img[..., 3] = depth.astype(F) / F(255.0)
        out[n] = img[::-1]
    return out


def nearest(verts, queries) -> np.ndarray:
    """The snap: float64 brute force, lowest id on ties, non-finite points never, a query without a finite distance unchanged."""
    v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    out = q.copy()
    for k in range(len(q)):
        with np.errstate(invalid="ignore", over="ignore"):
            d = v - q[k]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2 = np.where(np.isfinite(d2), d2, np.inf)
        best = int(np.argmin(d2))                # the first minimum
        if np.isfinite(d2[best]):
            out[k] = v[best]
    return out
