#!/usr/bin/env python3
"""Time the device PNG encoder (mvlm_png_encode) against Pillow on the pictures the views draw of the bench mesh,
face_like_mesh(224, 256, seed=0), textured: the 1024^2 landmark view with 84 landmarks and the ray view's three 1024^2 pictures
(84 x 8 rays).  Per picture set: Pillow's encode and write of the same pixels (the copy to the host stated beside it), the device
encoder end to end - encode, copy of the files' bytes, write -, its stages by the library's events (filter, deflate, gather, copy
to host) beside the view's own draw time, and the files' sizes.

    tools/png_encode_bench.py                 the table above
    tools/png_encode_bench.py --step [steps]  a configs[2] step (96 views, 84 landmarks) with Pipeline(visualize_img=True, one
                                              1024^2 view) under view_png_encoder "host" and "device", three rounds, alternating
It prints; profiles/png_encode_time.txt is that output."""
import ctypes as C
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd.utils import HipEstimator3D, HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh
from mvlm_amd.utils.viewer import write_view_png

SIZE = 1024
POSES = ((0, 0, 0), (0, 60, 0), (0, -60, 0))
STAGES = ("filter", "deflate", "gather", "copy to host")


def median_ms(call, n):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t))
    return float(np.median(out)), float(min(out))


def pictures():
    base = face_like_mesh(224, 256, seed=0)
    mesh = Mesh(base.verts, base.tris, base.uvs, base.texture)
    r = HipRenderer3D(n_views=1, verbose=False)
    e3 = HipEstimator3D(verbose=False)
    lib, h = r.ctx.lib, r.ctx.handle
    rs = np.random.RandomState(0)
    lm = np.asarray(base.verts, np.float64)[rs.permutation(len(base.verts))[:84]]
    view_poses = rs.uniform(-60.0, 60.0, (8, 3))
    maxima = np.concatenate([rs.uniform(70.0, 186.0, (84, 8, 2)), np.ones((84, 8, 1))], axis=2).astype(np.float32)
    starts, ends = e3.lines_device(torch.from_numpy(maxima).cuda(), view_poses, 256)
    ends, _ = e3.clip_rays_device(mesh, starts, ends)
    sets = (("landmark view, one 1024^2 picture", lambda: r.render_landmark_view_device(mesh, lm, size=SIZE),
             lib.mvlm_landmark_view_stage_ms, 7),
            ("ray view, three 1024^2 pictures", lambda: r.render_ray_view_device(mesh, lm, starts, ends, poses=POSES, size=SIZE),
             lib.mvlm_ray_view_stage_ms, 8))
    with tempfile.TemporaryDirectory() as td:
        for what, draw, view_stages, n_stages in sets:
            rgba = draw()
            r.check()
            n = int(rgba.shape[0])
            paths = [Path(td) / f"p{i}.png" for i in range(n)]
            copy_ms, _ = median_ms(lambda: rgba.cpu(), 5)
            host = rgba.cpu().numpy()[..., :3].copy()
            pillow_ms, pillow_min = median_ms(lambda: [write_view_png(im, q) for im, q in zip(host, paths)], 5)
            pillow_bytes = [q.stat().st_size for q in paths]
            for _ in range(3):
                write_view_png(rgba, paths, encoder="device", renderer=r)
            dev_ms, dev_min = median_ms(lambda: write_view_png(rgba, paths, encoder="device", renderer=r), 20)
            dev_bytes = [q.stat().st_size for q in paths]
            enc_ms, _ = median_ms(lambda: r.encode_png(rgba), 20)
            lib.mvlm_render_set_profiling(h, 1)
            rows = []
            for _ in range(20):
                r.encode_png(rgba)
                rows.append(r.png_stage_ms())
            draw()
            ms = (C.c_float * n_stages)()
            r.ctx.check(view_stages(h, ms))
            lib.mvlm_render_set_profiling(h, 0)
            draw_ms = float(sum(ms[i] for i in range(n_stages)))
            med = np.median(np.array(rows), axis=0)
            print(f"{what}: the view's own draw {1e3 * draw_ms:.1f} us")
            print(f"  host   copy of the RGBA pixels {copy_ms:8.3f} ms; Pillow encode + write {pillow_ms:8.3f} ms (min {pillow_min:.3f}); "
                  f"files {pillow_bytes} B")
            print(f"  device encode + copy of the files + write {dev_ms:8.3f} ms (min {dev_min:.3f}); without the write {enc_ms:.3f} ms; "
                  f"files {dev_bytes} B")
            print("  device stages (events): " + "  ".join(f"{s} {1e3 * m:8.1f} us" for s, m in zip(STAGES, med))
                  + f"  | sum {1e3 * med.sum():.1f} us")
            above = [s for s, m in zip(STAGES, med) if m > draw_ms]
            print(f"  stages above the view's own draw time: {', '.join(above) if above else 'none'}", flush=True)


def step(steps):
    from mvlm_amd import config

    mesh = face_like_mesh(224, 2048, seed=0)
    pipe = config.load_config(config.default_config("BU_3DFE", "RGB+depth", n_views=96)).build_pipeline(weights="synthetic:0", verbose=False)
    pipe.visualize_size = 1024
    pipe.visualize_img = True
    np.random.seed(0)
    poses = pipe.renderer_3d.generate_3d_transformations()
    ms = {"host": [], "device": []}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for rnd in range(3):
                for enc in ("host", "device"):
                    pipe.view_png_encoder = enc
                    for _ in range(3):
                        np.random.seed(1)
                        pipe.predict_mesh_device(mesh, poses)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(steps):
                        np.random.seed(1)
                        pipe.predict_mesh_device(mesh, poses)
                    torch.cuda.synchronize()
                    ms[enc].append(1e3 * (time.perf_counter() - t) / steps)
        finally:
            os.chdir(cwd)
    for enc, r in ms.items():
        print(f"configs[2] step (96 views, 84 landmarks, visualize_img at 1024^2), view_png_encoder={enc!r}: median {np.median(r):.3f} ms "
              f"per step (rounds {', '.join(f'{v:.3f}' for v in r)})")
    pairs = list(zip(ms["host"], ms["device"]))
    print(f"device shorter than host in every round: {all(d < h for h, d in pairs)}; host / device per round: "
          + ", ".join(f"{h / d:.2f} x" for h, d in pairs))


if __name__ == "__main__":
    if "--step" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--step"]
        step(int(rest[0]) if rest else 10)
    else:
        pictures()
