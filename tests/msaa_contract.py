"""Comparison of a 4-sample image stack with tests/golden/gl_raster_msaa4.npz (test infrastructure, shared by the CPU test of
the model, tests/test_gl_msaa_contract.py, and the -m gpu test of the HIP rasteriser, tests/test_gpu_msaa.py).

gl_raster_msaa4.npz holds the resolved RGB bytes of the reference's GL work drawn by SwiftShader's OpenGL ES 3.0 into a 4-sample
target (tools/make_gl_msaa_golden.py); the scenes' inputs are those of gl_raster.npz, plus three probe scenes stored with it.
The resolved depth cannot be read back from this GL (meta "findings"), so only the colour planes are compared.  A pixel that
differs is classified PER SAMPLE, with the classes of tests/gl_contract.py:

  clip     the scene has vertices outside the window: this GL clips geometrically and snaps the new vertices
  texel    giving the samples of one or more winning triangles the colour of a texel adjacent to their own yields the GL's
           resolved bytes: those colours' (u, v) lie within the GL's interpolation error of a texel boundary
"""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden" / "gl_raster_msaa4.npz"


def load():
    """-> meta, {scene: {"rgb": u8 [N,256,256,3] image rows, and for the probe scenes their inputs}}"""
    g = np.load(GOLDEN)
    meta = json.loads(str(g["meta"]))
    out = {}
    for name in g["scenes"]:
        name = str(name)
        sc = {"rgb": g[f"{name}.rgb"]}
        if f"{name}.verts" in g:
            for k in ("verts", "tris", "uvs", "tex", "poses"):
                sc[k] = g[f"{name}.{k}"]
            sc["lattice"] = True
        out[name] = sc
    return meta, out


def resolve(c: np.ndarray) -> np.ndarray:
    """the GL's resolve of [..., 4] sample bytes (meta findings "colour_resolve")"""
    c = c.astype(np.int32)
    return ((((c[..., 0] + c[..., 1] + 1) >> 1) + ((c[..., 2] + c[..., 3] + 1) >> 1) + 1) >> 1).astype(np.uint8)


def _neighbour_colours(tex: np.ndarray, colour: np.ndarray) -> list:
    h, w = tex.shape[:2]
    out = []
    for y, x in np.argwhere((tex == colour).all(-1)):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy or dx:
                    out.append(tex[(y + dy) % h, (x + dx) % w])
    return out


def compare(scene: dict, stack: np.ndarray, win_tri: np.ndarray, win_rgb: np.ndarray, gl_rgb: np.ndarray) -> dict:
    """stack f32 [N,256,256,4] (the 4-sample render), win_tri / win_rgb its per-sample winners and colours (GL rows, from the
    model), gl_rgb u8 [N,256,256,3] the GL's resolved bytes (image rows) -> counts per class + `unexplained`"""
    from oracle.estimator import view_rotation

    got = np.round(stack * 255.0).astype(np.uint8)
    assert np.array_equal(got.astype(np.float32) / np.float32(255), stack), "the stack's values are not k / 255"
    out = {"pixels": int(gl_rgb[..., 0].size), "differ": 0, "clip": 0, "texel": 0, "unexplained": 0}
    for v in range(gl_rgb.shape[0]):
        xy = (scene["verts"].astype(np.float64) @ view_rotation(*scene["poses"][v, :3]).T)[:, :2]
        clipped = bool((np.abs(xy) > 150.0).any())
        for y, x in zip(*np.nonzero((got[v, ..., :3] != gl_rgb[v]).any(-1))):
            out["differ"] += 1
            if clipped:
                out["clip"] += 1
                continue
            j = 255 - y                                        # GL row of image row y
            tri, cols = win_tri[v, j, x], win_rgb[v, j, x].astype(np.int32)   # [4], [4, 3]
            explained = False
            if scene["tex"] is not None:
                import itertools

                tris = sorted(set(int(k) for k in tri if k >= 0))
                options = [[None] + _neighbour_colours(scene["tex"], cols[np.argmax(tri == t)]) for t in tris]
                for pick in itertools.product(*options):
                    c = cols.copy()
                    for t, alt in zip(tris, pick):
                        if alt is not None:
                            c[tri == t] = alt
                    if any(a is not None for a in pick) and np.array_equal(resolve(c.T), gl_rgb[v, y, x]):
                        explained = True
                        break
            out["texel" if explained else "unexplained"] += 1
    return out
