"""ctypes loader of tests/native/vcolor_raster.c, the CPU model of the renderer contract with per-vertex colours, at one and
at four samples per pixel (test infrastructure).

`load(directory)` compiles it with the flags oracle/Makefile uses (gcc -O2 -ffp-contract=off) into the given directory - a
pytest temporary directory, once per session - and `render` takes oracle.raster.multiview_render's arguments plus `samples`
(1: one sample at the pixel centre = oracle/raster.c; 4: the multisampled contract) and `colors` (uint8 [V,3] or None: they
shade the RGB planes when shading is "texture" and `uvs` or `texture` is missing - DESIGN.md 5.1)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

SRC = Path(__file__).resolve().parent / "native" / "vcolor_raster.c"
_lib = None


def load(directory: Path):
    global _lib
    if _lib is None:
        so = Path(directory) / "libvcolor_raster.so"
        r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", str(SRC), "-o", str(so), "-lm"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"building the vertex-colour model failed:\n{r.stderr}")
        _lib = C.CDLL(str(so))
        _lib.vcolor_render.restype = C.c_int
    return _lib


def render(verts, tris, uvs, texture, transform_stack, shading: str = "texture", subpixel_bits: int = 8, samples: int = 1,
           per_sample: bool = False, colors=None):
    """-> image stack f32 [N,256,256,4] like oracle.raster.multiview_render; with per_sample also (win_tri i32 [N,256,256,S],
    win_rgb u8 [N,256,256,S,3]), GL rows (row 0 = bottom): each sample's winning triangle (-1 = uncovered) and colour."""
    from oracle.estimator import view_rotation

    assert _lib is not None, "vcolor_model.load(directory) first"
    verts = np.ascontiguousarray(verts, np.float32)
    tris = np.ascontiguousarray(tris, np.int32)
    n = int(np.asarray(transform_stack).shape[0])
    rot = np.ascontiguousarray(np.stack([view_rotation(*transform_stack[i, :3]).ravel() for i in range(n)]), np.float64)
    out = np.empty((n, 256, 256, 4), np.float32)
    use_tex = uvs is not None and texture is not None
    uv = np.ascontiguousarray(uvs, np.float32) if uvs is not None else None
    tex = np.ascontiguousarray(texture, np.uint8) if use_tex else None
    col = np.ascontiguousarray(colors, np.uint8) if colors is not None else None
    assert col is None or col.shape == (verts.shape[0], 3)
    win_tri = np.empty((n, 256, 256, samples), np.int32) if per_sample else None
    win_rgb = np.empty((n, 256, 256, samples, 3), np.uint8) if per_sample else None
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = _lib.vcolor_render(p(verts, C.c_float), p(uv, C.c_float), C.c_int(verts.shape[0]), p(tris, C.c_int32),
                          C.c_int(tris.shape[0]), p(tex, C.c_uint8), C.c_int(tex.shape[0] if use_tex else 0),
                          C.c_int(tex.shape[1] if use_tex else 0), p(col, C.c_uint8), p(rot, C.c_double), C.c_int(n),
                          C.c_int(1 if shading == "geometry" else 0), C.c_int(subpixel_bits), C.c_int(samples),
                          p(out, C.c_float), p(win_tri, C.c_int32), p(win_rgb, C.c_uint8))
    if rc != 0:
        raise ValueError(f"vcolor_render failed ({rc})")
    return (out, win_tri, win_rgb) if per_sample else out
