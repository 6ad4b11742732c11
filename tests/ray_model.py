"""ctypes loader of tests/native/ray_view.c, the CPU model of the ray view (test infrastructure): the landmark view's model
(view_model.py, tests/native/landmark_view.c) with the rays between the mesh and the spheres.

`load(directory)` compiles it with gcc -O2 -ffp-contract=off into the given directory - a pytest temporary directory, once per
session - and `render` takes mvlm_render_ray_view's arguments (poses in degrees, host arrays for the rays) and returns the image,
both count tables, the per-pixel winner and the winner's depth."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import view_model

SRC = Path(__file__).resolve().parent / "native" / "ray_view.c"
RAY_CODE_BASE = -1000000  # winner plane: ray r is RAY_CODE_BASE - r
DEFAULT_RAY_RGB = (26, 230, 26)
_lib = None


def load(directory: Path):
    global _lib
    if _lib is None:
        so = Path(directory) / "libray_view.so"
        r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", str(SRC), "-o", str(so), "-lm"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building the ray-view model failed:\n{r.stderr}")
        _lib = C.CDLL(str(so))
        _lib.ray_view.restype = C.c_int
    return _lib


def ray_of(winner) -> np.ndarray:
    """winner plane -> the ray's index per pixel, -1 where no ray won"""
    w = np.asarray(winner)
    return np.where(w <= RAY_CODE_BASE, RAY_CODE_BASE - w, -1)


def render(verts, tris, uvs, texture, poses, size, frame=view_model.NETWORK_FRAME, landmarks=None, radius=0.0, lm_rgb=None,
           starts=None, ends=None, ray_radius=0.5, ray_rgb=None, colors=None, shading: str = "texture", subpixel_bits: int = 8):
    """-> (image u8 [N,S,S,4], lm_counts i32 [N,NL], ray_counts i32 [N,NR], winner i32 [N,S,S], depth f32 [N,S,S]); image rows.
    winner: the triangle's id, -1 = background, -2 - l = landmark l's sphere, RAY_CODE_BASE - r = ray r."""
    assert _lib is not None, "ray_model.load(directory) first"
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    rot = view_model.rotations(poses)
    n = rot.shape[0]
    fr = view_model.frames_for(n, frame)
    use_tex = uvs is not None and texture is not None
    uv = np.ascontiguousarray(uvs, np.float32) if uvs is not None else None
    tex = np.ascontiguousarray(texture, np.uint8) if use_tex else None
    col = np.ascontiguousarray(colors, np.uint8) if colors is not None else None
    lm = np.ascontiguousarray(landmarks, np.float64).reshape(-1, 3) if landmarks is not None else np.zeros((0, 3))
    nl = lm.shape[0]
    rgb = np.ascontiguousarray(lm_rgb, np.uint8).reshape(nl, 3) if lm_rgb is not None else None
    a = np.ascontiguousarray(starts, np.float64).reshape(-1, 3) if starts is not None else np.zeros((0, 3))
    b = np.ascontiguousarray(ends, np.float64).reshape(-1, 3) if ends is not None else np.zeros((0, 3))
    nr = a.shape[0]
    assert b.shape[0] == nr
    rrgb = np.ascontiguousarray(ray_rgb, np.uint8).reshape(nr, 3) if ray_rgb is not None else None
    out = np.empty((n, size, size, 4), np.uint8)
    counts = np.zeros((n, nl), np.int32)
    rcounts = np.zeros((n, nr), np.int32)
    winner = np.empty((n, size, size), np.int32)
    depth = np.empty((n, size, size), np.float32)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t)) if x is not None and x.size else None
    rc = _lib.ray_view(p(verts, C.c_float), p(uv, C.c_float), C.c_int(verts.shape[0]), p(tris, C.c_int32),
                       C.c_int(tris.shape[0]), p(tex, C.c_uint8), C.c_int(tex.shape[0] if use_tex else 0),
                       C.c_int(tex.shape[1] if use_tex else 0), p(col, C.c_uint8), p(rot, C.c_double), C.c_int(n),
                       C.c_int(size), p(fr, C.c_float), p(lm, C.c_double), C.c_int(nl), C.c_float(radius), p(rgb, C.c_uint8),
                       p(a, C.c_double), p(b, C.c_double), C.c_int(nr), C.c_float(ray_radius), p(rrgb, C.c_uint8),
                       C.c_int(1 if shading == "geometry" else 0), C.c_int(subpixel_bits), p(out, C.c_uint8),
                       p(counts, C.c_int32), p(rcounts, C.c_int32), p(winner, C.c_int32), p(depth, C.c_float))
    if rc != 0:
        raise ValueError(f"ray_view failed ({rc})")
    return out, counts, rcounts, winner, depth
