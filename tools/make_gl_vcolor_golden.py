"""Write tests/golden/gl_raster_vcolor.npz: meshes with per-vertex colours and no texture, drawn by the same OpenGL as
gl_raster.npz the way VTK's mapper draws point scalars (tools/gl_reference.py: a normalised unsigned-byte vertex attribute
through a varying; ambient 1, diffuse 0).

BUILD-CONTAINER TOOL (SwiftShader's OpenGL ES 3.0).  Four scenes of tools/make_gl_golden.py are reused by name - `face40`
(sub-pixel-free 4-pixel triangles, silhouettes), `coarse` (triangles of ~100 pixels), `offscreen` (triangles leaving the window)
and `centres` (both windings, edges through pixel centres) - with colours from a seeded generator; their geometry is not stored
again, only the colours, the views drawn (`views`, indices into the scene's poses: the file has to stay small) and the RGB
bytes.  `face40` is also drawn into a 4-sample target (`face40_ms4`).  Two probe scenes are stored whole; the bytes read back
tell how this GL converts an interpolated colour to a byte (`meta` "findings"):
  ramp    a quad over the whole window, red 0 -> 255 left to right, green 0 -> 255 bottom to top, blue 255 -> 0 left to right:
          the exact value at pixel centre i is 255 (i + 0.5) / 256, never closer than 1/512 to k or to k + 0.5 - every byte
          value, but nothing near a rounding boundary;
  fine    128 strips of two pixel rows, each 240 pixels wide with its colour rising by ONE code value from left to right
          (k -> k + 1, k from 8 base values per channel on both sides of 128), its left edge at 8 + s/16 pixels, s = 0..15: the
          exact value at pixel centre i is k + (i + 0.5 - 8 - s/16) / 240, which steps through k + 1/2 in units of 1/3840 of a
          code value - what happens at and around a rounding boundary.

    python tools/make_gl_vcolor_golden.py [--out tests/golden/gl_raster_vcolor.npz]
"""
from __future__ import annotations

import argparse
import json
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from gl_reference import GLReference, MultisampleTarget  # noqa: E402
from make_gl_golden import px, rotation, scenes  # noqa: E402

SEED = 20
VIEWS = {"face40": [0, 3], "coarse": [0, 1, 2], "offscreen": [0, 1], "centres": [0]}
MS_SCENE, MS_VIEWS, SAMPLES = "face40", [3], 4


def ramp_scene():
    v = np.array([[px(0.0), px(0.0), 7.0], [px(256.0), px(0.0), 7.0], [px(256.0), px(256.0), 7.0], [px(0.0), px(256.0), 7.0]], np.float32)
    c = np.array([[0, 0, 255], [255, 0, 0], [255, 255, 0], [0, 255, 255]], np.uint8)
    return dict(verts=v, tris=np.array([[0, 1, 2], [0, 2, 3]], np.int32), colors=c, poses=np.zeros((1, 3)))


FINE_BASES = [(3, 127, 250), (40, 128, 200), (77, 126, 161), (100, 129, 130), (120, 64, 254), (126, 200, 0), (127, 1, 128),
              (60, 180, 90)]                                  # (k of red, green, blue) per group of 16 strips


def fine_scene():
    verts, tris, colors = [], [], []
    for g, base in enumerate(FINE_BASES):
        for s in range(16):
            y0, x0 = 2 * (16 * g + s), 8 + s / 16
            n = len(verts)
            verts += [[px(x0), px(y0), 7.0], [px(x0 + 240), px(y0), 7.0], [px(x0 + 240), px(y0 + 2), 7.0], [px(x0), px(y0 + 2), 7.0]]
            tris += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
            colors += [base, [k + 1 for k in base], [k + 1 for k in base], base]
    return dict(verts=np.asarray(verts, np.float32), tris=np.asarray(tris, np.int32), colors=np.asarray(colors, np.uint8),
                poses=np.zeros((1, 3)))


def fine_values():
    """exact value (Fraction, in code values) per covered pixel of the fine probe: {(row j, column i, channel): value}"""
    out = {}
    for g, base in enumerate(FINE_BASES):
        for s in range(16):
            x0 = Fraction(8) + Fraction(s, 16)
            for i in range(256):
                d = Fraction(2 * i + 1, 2) - x0
                if 0 < d < 240:                                  # (no pixel centre lies on a strip's left or right edge)
                    for ch in range(3):
                        for j in (2 * (16 * g + s), 2 * (16 * g + s) + 1):
                            out[(j, i, ch)] = base[ch] + d / 240
    return out


def to_byte_16(v: Fraction) -> int:
    """through 16-bit fixed point: c16 = trunc(65535 f), byte = (c16 - (c16 >> 8) + 128) >> 8, f = v / 255"""
    c16 = int(v * 65535 / 255)
    return (c16 - (c16 >> 8) + 128) >> 8


RULES = {"round to nearest: (int)(255 f + 0.5)": lambda v: int(v + Fraction(1, 2)),
         "truncate: (int)(255 f)": lambda v: int(v),
         "round up: ceil(255 f)": lambda v: -int(-v // 1),
         "16-bit fixed point: c16 = trunc(65535 f), (c16 - (c16 >> 8) + 128) >> 8": to_byte_16}


def conversion_rule(ramp_bottom_up: np.ndarray, fine_bottom_up: np.ndarray) -> tuple:
    """which float -> byte conversion the probes' bytes show (exact values in rationals): hits per rule over the ramp's
    3 x 65 536 bytes and over the fine probe's covered bytes"""
    exact = [Fraction(255 * (2 * i + 1), 512) for i in range(256)]
    fine = fine_values()
    ramp_hits, fine_hits = {}, {}
    for name, rule in RULES.items():
        t = np.asarray([rule(e) for e in exact], np.uint8)
        want = np.empty((256, 256, 3), np.uint8)
        want[..., 0] = t[None, :]
        want[..., 1] = t[:, None]
        want[..., 2] = t[None, ::-1]
        ramp_hits[name] = int((want == ramp_bottom_up).sum())
        fine_hits[name] = sum(int(rule(v) == int(fine_bottom_up[j, i, ch])) for (j, i, ch), v in fine.items())
    return ramp_hits, fine_hits, len(fine)


def draw(target, sc, views):
    out = []
    for rx, ry, rz in np.asarray(sc["poses"])[views]:
        m = rotation(rx, ry, rz)
        v = sc["verts"].astype(np.float64)
        vv = np.stack([(m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2] for k in range(3)], 1).astype(np.float32)
        out.append(target.draw(vv)[0])
    return np.stack(out)                                                    # GL rows (row 0 = bottom)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "tests" / "golden" / "gl_raster_vcolor.npz"))
    args = ap.parse_args()
    gl = GLReference(256)
    rs = np.random.RandomState(SEED)
    base = scenes()
    store, names = {}, []
    for name, views in VIEWS.items():
        sc = base[name]
        colors = rs.randint(0, 256, (len(sc["verts"]), 3)).astype(np.uint8)
        gl.set_mesh(None, sc["tris"], None, colors)
        store[f"{name}.colors"] = colors
        store[f"{name}.views"] = np.asarray(views, np.int32)
        store[f"{name}.rgb"] = np.ascontiguousarray(np.flip(draw(gl, sc, views), 1))     # image rows, like the stack
        names.append(name)
        print(f"{name}: views {views}")
    ramp = ramp_scene()
    gl.set_mesh(None, ramp["tris"], None, ramp["colors"])
    ramp_rgb = draw(gl, ramp, [0])
    fine = fine_scene()
    gl.set_mesh(None, fine["tris"], None, fine["colors"])
    fine_rgb = draw(gl, fine, [0])
    hits, fine_hits, fine_n = conversion_rule(ramp_rgb[0], fine_rgb[0])
    rule = [k for k in RULES if hits[k] == 3 * 65536 and fine_hits[k] == fine_n]
    for probe, sc, rgb in (("ramp", ramp, ramp_rgb), ("fine", fine, fine_rgb)):
        for k in ("verts", "tris", "colors", "poses"):
            store[f"{probe}.{k}"] = np.asarray(sc[k])
        store[f"{probe}.views"] = np.array([0], np.int32)
        store[f"{probe}.rgb"] = np.ascontiguousarray(np.flip(rgb, 1))
        names.append(probe)
    # the 4-sample scene: drawn last (the multisampled target rebinds the framebuffer)
    ms = MultisampleTarget(gl, SAMPLES)
    sc = base[MS_SCENE]
    gl.set_mesh(None, sc["tris"], None, store[f"{MS_SCENE}.colors"])
    store[f"{MS_SCENE}_ms4.views"] = np.asarray(MS_VIEWS, np.int32)
    store[f"{MS_SCENE}_ms4.rgb"] = np.ascontiguousarray(np.flip(draw(ms, sc, MS_VIEWS), 1))
    names.append(f"{MS_SCENE}_ms4")
    findings = {
        "colour_to_byte": rule[0] if len(rule) == 1 else None,
        "colour_to_byte_hits": hits,
        "colour_to_byte_pixels": 3 * 65536,
        "colour_to_byte_fine_hits": fine_hits,
        "colour_to_byte_fine_pixels": fine_n,
        "attribute": "GL_UNSIGNED_BYTE x 4, normalised, through a smooth varying; fragColour = vec4(colour.rgb, 1) when not textured",
    }
    store["meta"] = np.array(json.dumps({"gl": gl.info, "generator": "tools/make_gl_vcolor_golden.py", "seed": SEED,
                                         "samples": {f"{MS_SCENE}_ms4": SAMPLES}, "findings": findings}))
    store["scenes"] = np.array(names)
    np.savez_compressed(args.out, **store)
    print(f"wrote {args.out} ({Path(args.out).stat().st_size} bytes); {json.dumps(findings)}")


if __name__ == "__main__":
    main()
