#!/usr/bin/env python3
"""Time the ray view (mvlm_render_ray_view) on the bench mesh, face_like_mesh(224, 256, seed=0), textured: three poses (front,
60 degrees left and right) at 1024^2 with 84 landmarks and 0, 672 (84 x 8), 8 064 (84 x 96) and 61 184 (478 x 128) view rays of
seeded heat-map maxima, clipped on the device - per stage from the library's own HIP events (mvlm_render_set_profiling,
mvlm_ray_view_stage_ms), median of 40 after 3 warm-up calls.  In the same run: mvlm_render_landmark_view of the same poses as the
yardstick, and the host's PNG encode of the three pictures (Pillow, as Pipeline writes them).

The one condition: at 8 064 rays the GPU time of the ray view stays below the PNG encode of its pictures.

It prints; profiles/ray_view_time.txt is that output."""
import ctypes as C
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

STAGES = ("fill", "transform", "classify", "scan", "bin_fill", "project", "ray_project", "tile")
POSES = ((0, 0, 0), (0, 60, 0), (0, -60, 0))
SIZE = 1024
RAYS = ((0, 0), (84, 8), (84, 96), (478, 128))


def rays_for(e3, mesh, nl, n, seed=0):
    """nl x n view rays of seeded maxima in seeded poses, clipped to the mesh: device tensors f64 [nl * n, 3]"""
    if nl * n == 0:
        z = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
        return z, z
    rs = np.random.RandomState(seed)
    poses = rs.uniform(-60.0, 60.0, (n, 3))
    maxima = np.concatenate([rs.uniform(70.0, 186.0, (nl, n, 2)), np.ones((nl, n, 1))], axis=2).astype(np.float32)
    starts, ends = e3.lines_device(torch.from_numpy(maxima).cuda(), poses, 256)
    ends, hit = e3.clip_rays_device(mesh, starts, ends)
    return starts.reshape(-1, 3).contiguous(), ends.reshape(-1, 3).contiguous()


def main():
    base = face_like_mesh(224, 256, seed=0)
    mesh = Mesh(base.verts, base.tris, base.uvs, base.texture)
    r = HipRenderer3D(n_views=1, verbose=False)
    e3 = HipEstimator3D(verbose=False)
    lib, h = r.ctx.lib, r.ctx.handle
    rs = np.random.RandomState(0)
    lm = np.asarray(base.verts, np.float64)[rs.permutation(len(base.verts))[:84]]

    def timed(call, fetch, n_stages):
        for _ in range(3):
            call()
        r.check()
        lib.mvlm_render_set_profiling(h, 1)
        rows = []
        for _ in range(40):
            call()
            ms = (C.c_float * n_stages)()
            r.ctx.check(fetch(h, ms))
            rows.append([1e3 * ms[i] for i in range(n_stages)])
        lib.mvlm_render_set_profiling(h, 0)
        r.check()
        return np.array(rows)

    rows = timed(lambda: r.render_landmark_view_device(mesh, lm, poses=POSES, size=SIZE, return_pixels=True),
                 lib.mvlm_landmark_view_stage_ms, 7)
    yard = float(np.median(rows.sum(axis=1)))
    print(f"landmark view, 3 poses of {SIZE}^2, 84 landmarks (the yardstick): median {yard:9.1f} us  min {rows.sum(axis=1).min():9.1f} us",
          flush=True)
    gpu_at = {}
    image = None
    for nl, n in RAYS:
        starts, ends = rays_for(e3, mesh, nl, n)
        rows = timed(lambda: r.render_ray_view_device(mesh, lm, starts, ends, poses=POSES, size=SIZE, return_pixels=True),
                     lib.mvlm_ray_view_stage_ms, 8)
        total, med = float(np.median(rows.sum(axis=1))), np.median(rows, axis=0)
        gpu_at[nl * n] = total
        shares = "  ".join(f"{s} {m:8.1f} us ({100 * m / med.sum():4.1f} %)" for s, m in zip(STAGES, med))
        print(f"ray view, 3 poses of {SIZE}^2, 84 landmarks, {nl * n:6d} rays ({nl} x {n}): median {total:9.1f} us  "
              f"min {rows.sum(axis=1).min():9.1f} us  {total / yard:6.2f} x the yardstick | {shares}", flush=True)
        if nl * n == 8064:
            image = r.render_ray_view(mesh, lm, starts, ends, poses=POSES, size=SIZE)
    enc = []
    with tempfile.TemporaryDirectory() as td:
        for _ in range(5):
            t = time.perf_counter()
            for i, im in enumerate(image):
                write_view_png(im, Path(td) / f"encode_{i}.png")
            enc.append(1e3 * (time.perf_counter() - t))
    enc_ms = float(np.median(enc))
    print(f"PNG encode and write of the three {SIZE}^2 pictures with 8064 rays (Pillow, host): median {enc_ms:.3f} ms")
    ok = gpu_at[8064] / 1e3 < enc_ms
    print(f"condition: GPU time at 8064 rays {gpu_at[8064] / 1e3:.3f} ms {'<' if ok else '>='} PNG encode {enc_ms:.3f} ms: "
          f"{'met with ballot compaction over all rays per tile - the rays are not binned' if ok else 'NOT met - bin the rays'}")


if __name__ == "__main__":
    main()
