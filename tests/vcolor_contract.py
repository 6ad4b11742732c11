"""Comparison of a coloured render with tests/golden/gl_raster_vcolor.npz (test infrastructure, shared by the CPU test of the
model, tests/test_gl_vcolor_contract.py, and the -m gpu test of the HIP rasteriser, tests/test_gpu_vertex_colors.py).

gl_raster_vcolor.npz holds the RGB bytes SwiftShader's OpenGL ES 3.0 draws for meshes with per-vertex colours and no texture
(tools/make_gl_vcolor_golden.py): four scenes of gl_raster.npz by name, with colours of their own and a subset of their views,
`face40_ms4` (one view of face40 through a 4-sample target) and the `ramp` and `fine` probes, stored whole.  The depth plane does not
depend on colours: it is gl_raster.npz's.  A pixel whose RGB differs falls into one of

  clip     the view has vertices outside the window: this GL clips geometrically, snaps the new vertices and interpolates
           the colour to them (tests/gl_contract.py)
  interp   same coverage, depth byte within 1 (the GL does not name its winning triangle: with a colour of its own on every
           vertex these stand for "the same triangle"), every channel within 1 code value: two float evaluations of one plane
           disagree in a byte where the exact value lies within their error of a boundary of the conversion

  ztie     at a sample point of the pixel two triangles that both cover it have the SAME exact depth (a fold: a back-facing
           triangle and its neighbour meet in the edge the sample lies on) - the depth test sees two float evaluations of one
           value, and which triangle is seen hangs on their last bits

anything else is `unexplained`."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

import gl_contract

GOLDEN = Path(__file__).resolve().parent / "golden" / "gl_raster_vcolor.npz"


def load():
    """-> meta, {scene: verts, tris, poses (the views drawn), colors, rgb u8 [n,256,256,3] image rows, depth u8 [n,256,256] or
    None (4 samples: not readable), samples}"""
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    _, base = gl_contract.load()
    out = {}
    for name in g["scenes"]:
        name = str(name)
        src = name[:-4] if name.endswith("_ms4") else name
        views = g[f"{name}.views"]
        if f"{name}.verts" in g:
            sc = {k: g[f"{name}.{k}"] for k in ("verts", "tris", "colors")}
            sc["poses"] = g[f"{name}.poses"][views]
            sc["depth"] = None
        else:
            sc = {"verts": base[src]["verts"], "tris": base[src]["tris"], "colors": g[f"{src}.colors"],
                  "poses": base[src]["poses"][views], "depth": base[src]["image_u8"][views][..., 3]}
        sc["samples"] = int(meta["samples"].get(name, 1))
        if sc["samples"] != 1:
            sc["depth"] = None
        sc["rgb"] = g[f"{name}.rgb"]
        out[name] = sc
    return meta, out


SAMPLE_POINTS = {1: [(8, 8)], 4: [(3, 6), (13, 10), (6, 13), (10, 3)]}     # 1/16 pixel


def _depth_tie(scene: dict, view: int, x: int, y: int, bits: int) -> bool:
    """do two triangles cover one sample point of pixel (x, image row y) with depths that agree to 2^-22, in exact arithmetic
    on the snapped vertices (the projection of DESIGN.md 5.1)?"""
    from fractions import Fraction as F

    from oracle.estimator import view_rotation

    f32 = np.float32
    m = view_rotation(*scene["poses"][view, :3])
    V = scene["verts"].astype(np.float64)
    xv, yv, zv = (((m[k, 0] * V[:, 0] + m[k, 1] * V[:, 1]) + m[k, 2] * V[:, 2]).astype(f32) for k in range(3))
    sub = f32(1 << bits)
    X = np.floor(((xv + f32(150)) * (f32(256) / f32(300))) * sub + f32(0.5)).astype(np.int64)
    Y = np.floor(((yv + f32(150)) * (f32(256) / f32(300))) * sub + f32(0.5)).astype(np.int64)
    Z = ((f32(500) - zv) / f32(1500)).astype(f32)
    a, b, c = scene["tris"].T.astype(np.int64)
    area = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
    for sx, sy in SAMPLE_POINTS[scene["samples"]]:
        px, py = (x * 16 + sx) * (1 << bits) // 16, ((255 - y) * 16 + sy) * (1 << bits) // 16
        w = [(X[q] - X[p]) * (py - Y[p]) - (Y[q] - Y[p]) * (px - X[p]) for p, q in ((b, c), (c, a), (a, b))]
        inside = (area != 0) & np.all([np.sign(wk) * np.sign(area) >= 0 for wk in w], 0)
        zs = sorted(sum(F(int(wk[t])) * F(float(Z[v[t]])) for wk, v in zip(w, (a, b, c))) / F(int(area[t])) for t in np.nonzero(inside)[0])
        if any(z1 - z0 <= F(1, 1 << 22) for z0, z1 in zip(zs, zs[1:])):
            return True
    return False


def compare(scene: dict, stack: np.ndarray, bits: int = 4) -> dict:
    """stack f32 [n,256,256,4]: the render of the scene's views (with its colours, at its sample count and at `bits` sub-pixel
    bits, the GL's) -> counts per class"""
    from oracle.estimator import view_rotation

    got = np.round(stack * 255.0).astype(np.uint8)
    assert np.array_equal(got.astype(np.float32) / np.float32(255), stack), "the stack's values are not k / 255"
    gl = scene["rgb"]
    assert got.shape[:3] == gl.shape[:3]
    covered = got[..., 3] != 1 if scene["depth"] is None else scene["depth"] != 1
    out = {"pixels": int(gl[..., 0].size), "covered": int(covered.sum()), "differ": 0, "clip": 0, "interp": 0, "ztie": 0, "unexplained": 0,
           "coloured": int(((gl != 255).any(-1) & covered).sum())}
    for v in range(gl.shape[0]):
        xy = (scene["verts"].astype(np.float64) @ view_rotation(*scene["poses"][v, :3]).T)[:, :2]
        clipped = bool((np.abs(xy) > 150.0).any())
        diff = (got[v, ..., :3] != gl[v]).any(-1)
        if scene["depth"] is not None:            # a coverage difference shows in the depth plane even where both are white
            diff |= (got[v, ..., 3] != 1) != (scene["depth"][v] != 1)
        n = int(diff.sum())
        out["differ"] += n
        if clipped:
            out["clip"] += n
            continue
        close = (np.abs(got[v, ..., :3].astype(np.int32) - gl[v].astype(np.int32)) <= 1).all(-1)
        if scene["depth"] is not None:
            d = np.abs(got[v, ..., 3].astype(np.int32) - scene["depth"][v].astype(np.int32))
            close &= ((got[v, ..., 3] != 1) == (scene["depth"][v] != 1)) & (np.minimum(d, 256 - d) <= 1)
        out["interp"] += int((diff & close).sum())
        for y, x in zip(*np.nonzero(diff & ~close)):
            out["ztie" if _depth_tie(scene, v, int(x), int(y), bits) else "unexplained"] += 1
    return out
