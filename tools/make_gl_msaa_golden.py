"""Write tests/golden/gl_raster_msaa4.npz: the reference renderer's GL work drawn by the same OpenGL as gl_raster.npz, into a
4-sample target resolved before the read-back the way VTK resolves (a blit to a single-sample target, render3d.py:157-168).

BUILD-CONTAINER TOOL (SwiftShader's OpenGL ES 3.0, tools/gl_reference.py).  The eleven scenes of tools/make_gl_golden.py are not
stored again (the tests take their inputs from gl_raster.npz by name); three small probe scenes are, and this script reads the
choices OpenGL leaves to a multisampling implementation off them and stores them in `meta`:
  positions  half-planes on the 1/16-pixel lattice stepped across a pixel: the resolved colour counts the covered samples;
  tie rule   the same steps from the other side: every sample on a shared edge belongs to exactly one side (LEFT / BOTTOM);
  resolve    four 1/16-pixel quads per pixel, one around each sample, random colours: which rounding of the average;
  colour     a textured triangle whose texels are 1/16 pixel: where in the pixel the colour is evaluated;
  depth      read back through a DEPTH_COMPONENT32F texture if this GL allows the blit into one.

    python tools/make_gl_msaa_golden.py [--out tests/golden/gl_raster_msaa4.npz]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from gl_reference import GLReference, MultisampleTarget  # noqa: E402
from make_gl_golden import merge, px, rotation, scenes  # noqa: E402

SAMPLES = 4


def quad(x0, y0, x1, y1, z=7.0, uv=(0.5, 0.5)):
    v = np.array([[px(x0), px(y0), z], [px(x1), px(y0), z], [px(x1), px(y1), z], [px(x0), px(y1), z]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([uv] * 4, np.float32)


def position_scene(upper: bool):
    """pixel (4 + 4a, 4 + 4b) covered by [p - 2, p + a/16] x [p - 2, p + b/16] (upper=False: right / top edges through the
    lattice point) or by [p + a/16, p + 2] x [p + b/16, p + 2] (upper=True: left / bottom edges), a, b = 0..16"""
    parts = []
    for a in range(17):
        for b in range(17):
            X, Y = 4 + 4 * a, 4 + 4 * b
            if not upper and a and b:
                parts.append(quad(X - 2, Y - 2, X + a / 16, Y + b / 16))
            if upper and a < 16 and b < 16:
                parts.append(quad(X + a / 16, Y + b / 16, X + 2, Y + 2))
    v, t, u = merge(parts)
    return dict(verts=v, tris=t, uvs=u, tex=np.zeros((1, 1, 3), np.uint8), poses=np.zeros((1, 3)), lattice=True)


def counts(rgb):
    """covered samples per probe pixel, [17, 17] over (a, b): black on white resolves to 255 (4 - k) / 4 in some rounding"""
    return np.array([[int(round((255 - int(rgb[4 + 4 * b, 4 + 4 * a, 0])) / 63.75)) for b in range(17)] for a in range(17)])


def positions_from(lo, hi):
    """lo[a, b] = #{s: x < a, y < b}, hi[a, b] = #{s: x >= a, y >= b} -> sample points (x, y) in 1/16 pixel"""
    pts = []
    for a in range(1, 17):
        for b in range(1, 17):
            for _ in range(lo[a, b] - lo[a - 1, b] - lo[a, b - 1] + lo[a - 1, b - 1]):
                pts.append((a - 1, b - 1))
    hi = np.pad(hi, ((0, 1), (0, 1)))
    pts_hi = []
    for a in range(16):
        for b in range(16):
            for _ in range(hi[a, b] - hi[a + 1, b] - hi[a, b + 1] + hi[a + 1, b + 1]):
                pts_hi.append((a, b))
    return sorted(pts), sorted(pts_hi)


def resolve_scene(pos, seed=0):
    """16 x 32 pixels, four quads of 2/16 pixel per pixel, one around each sample, each with its own random texel"""
    tex = np.random.RandomState(seed).randint(0, 256, (64, 64, 3)).astype(np.uint8)
    parts = []
    for yy in range(16):
        for xx in range(32):
            X, Y = 100 + 2 * xx, 100 + 2 * yy
            for s, (sx, sy) in enumerate(pos):
                k = (yy * 32 + xx) * 4 + s
                uv = (((k % 64) + 0.5) / 64, ((k // 64) + 0.5) / 64)
                parts.append(quad(X + (sx - 1) / 16, Y + (sy - 1) / 16, X + (sx + 1) / 16, Y + (sy + 1) / 16, z=7.0 + s, uv=uv))
    v, t, u = merge(parts)
    return dict(verts=v, tris=t, uvs=u, tex=tex, poses=np.zeros((1, 3)), lattice=True)


def resolve_rule(rgb, sc, pos):
    """which rounding of the four samples' average the resolved bytes show, over every probe pixel"""
    tex = sc["tex"]
    avg = lambda a, b: (a + b + 1) >> 1
    rules = {"(a+b+c+d+2)>>2": lambda c: (sum(c) + 2) >> 2, "(a+b+c+d)>>2": lambda c: sum(c) >> 2}
    for p, q in (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2))):
        rules[f"avg(avg(s{p[0]},s{p[1]}),avg(s{q[0]},s{q[1]}))"] = lambda c, p=p, q=q: avg(avg(c[p[0]], c[p[1]]), avg(c[q[0]], c[q[1]]))
    hits = dict.fromkeys(rules, 0)
    for yy in range(16):
        for xx in range(32):
            c = []
            for s in range(len(pos)):
                k = (yy * 32 + xx) * 4 + s
                c.append(tex[63 - k // 64, k % 64].astype(int))
            got = rgb[100 + 2 * yy, 100 + 2 * xx].astype(int)
            for name, f in rules.items():
                hits[name] += int(np.array_equal(f(c), got))
    return hits


def centre_scene():
    """one triangle (vertices on the 1/16 lattice, edges at every offset) over a 256 x 256 texture whose texel (x, y) has the
    colour (x, y, 128); u = (x + 0.03) / 16, v = (y + 0.03) / 16 in window pixels: texels of 1/16 pixel, no sample point or
    pixel centre within 0.03 pixel of a texel boundary"""
    tex = np.zeros((256, 256, 3), np.uint8)
    tex[:, :, 0] = np.arange(256)[None, :]
    tex[:, :, 1] = np.arange(256)[::-1, None]
    tex[:, :, 2] = 128
    p = [(20 + 3 / 16, 30 + 5 / 16), (200 + 11 / 16, 60 + 1 / 16), (70 + 7 / 16, 220 + 13 / 16)]
    v = np.array([[px(a), px(b), 7.0] for a, b in p], np.float32)
    u = np.array([((a + 0.03) / 16, (b + 0.03) / 16) for a, b in p], np.float32)
    return dict(verts=v, tris=np.array([[0, 1, 2]], np.int32), uvs=u, tex=tex, poses=np.zeros((1, 3)), lattice=True)


def draw(gl, ms, sc):
    gl.set_mesh(sc["uvs"], sc["tris"], sc["tex"])
    rgbs, zs = [], []
    for rx, ry, rz in sc["poses"]:
        m = rotation(rx, ry, rz)
        v = sc["verts"].astype(np.float64)
        vv = np.stack([(m[k, 0] * v[:, 0] + m[k, 1] * v[:, 1]) + m[k, 2] * v[:, 2] for k in range(3)], 1).astype(np.float32)
        rgb, z = ms.draw(vv)
        rgbs.append(rgb)
        zs.append(z)
    return np.stack(rgbs), zs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "tests" / "golden" / "gl_raster_msaa4.npz"))
    args = ap.parse_args()
    gl = GLReference(256)
    ms = MultisampleTarget(gl, SAMPLES)
    probes = {"ms_positions_lo": position_scene(False), "ms_positions_hi": position_scene(True)}
    lo = counts(draw(gl, ms, probes["ms_positions_lo"])[0][0])
    hi = counts(draw(gl, ms, probes["ms_positions_hi"])[0][0])
    pos, pos_hi = positions_from(lo, hi)
    assert len(pos) == SAMPLES and pos == pos_hi, (pos, pos_hi)   # item 5: each lattice sample on an edge goes to ONE side
    probes["ms_resolve"] = resolve_scene(pos)
    hits = resolve_rule(draw(gl, ms, probes["ms_resolve"])[0][0], probes["ms_resolve"], pos)
    rule = [k for k, v in hits.items() if v == 512]
    assert len(rule) == 1, hits
    # order the samples as the resolve pairs them: (0, 1), (2, 3)
    pairs = [tuple(int(d) for d in part.replace("avg", "").replace("(", "").replace(")", "").replace("s", "").split(",") if d)
             for part in rule[0][4:-1].split("),avg(")]
    order = [pos[i] for pr in pairs for i in pr]
    probes["ms_centre"] = centre_scene()
    findings = {
        "sample_positions_16th": order,
        "position_origin": "lower-left pixel corner, window coordinates (y up); samples ordered as the resolve pairs them",
        "tie_rule": "left / bottom edge owns a sample on a shared edge, as at pixel centres",
        "colour_resolve": "per byte avg(avg(s0, s1), avg(s2, s3)) with avg(a, b) = (a + b + 1) >> 1",
        "colour_resolve_hits": hits,
        "colour_evaluated_at": "pixel centre, once per pixel (extrapolated when the centre lies outside the triangle)",
        "depth_resolve": None,
    }
    store = {}
    names = []
    all_scenes = dict(scenes())
    all_scenes.update(probes)
    for name, sc in all_scenes.items():
        rgbs, zs = draw(gl, ms, sc)
        if ms.depth_readable:
            findings["depth_resolve"] = "readable"
            store[f"{name}.zbits"] = np.stack([np.flip(z, 0) for z in zs]).view(np.uint32)
        store[f"{name}.rgb"] = np.ascontiguousarray(np.flip(rgbs, 1))      # resolved RGB bytes, image rows like the stack
        if name in probes:
            for k in ("verts", "tris", "uvs", "tex", "poses"):
                store[f"{name}.{k}"] = np.asarray(sc[k])
            store[f"{name}.lattice"] = np.array(True)
        names.append(name)
        print(f"{name}: {len(sc['poses'])} views")
    if findings["depth_resolve"] is None:
        findings["depth_resolve"] = ("not readable: this GL refuses the blit of a multisampled depth buffer into a depth texture "
                                     "(GL_INVALID_OPERATION); sample 0 assumed")
    store["meta"] = np.array(json.dumps({"gl": gl.info, "samples": SAMPLES, "generator": "tools/make_gl_msaa_golden.py",
                                         "findings": findings}))
    store["scenes"] = np.array(names)
    np.savez_compressed(args.out, **store)
    print(f"wrote {args.out} ({Path(args.out).stat().st_size} bytes); {json.dumps(findings)}")


if __name__ == "__main__":
    main()
