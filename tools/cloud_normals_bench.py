#!/usr/bin/env python3
"""Time a point cloud's normals: the estimate's three stages (grid build, search, solve: mvlm_normals_stage_ms), the 96-view
geometry render with them and - the yardstick - the same cloud's texture-mode render, whose two kernels are the ones from before
normals existed (raster_points.hip is unchanged device code).  Median and minimum of RUNS runs by the library's own events.

    tools/cloud_normals_bench.py                 the table (profiles/cloud_normals_time.txt)
    tools/cloud_normals_bench.py --once N        one estimate and one geometry render of the N-point cloud, nothing else: the
                                                 program to put behind `rocprofv3 --kernel-trace --stats --` for the kernels' times

Clouds: the vertices of face_like_mesh(317) (100 489 points) and of face_like_mesh(1000) (1 000 000 points), faces dropped.  One
extra estimate runs the search kernel's counting form (mvlm_points_set_counting, mvlm_normals_get_stats): shells walked, candidates
tested and candidates that entered a list, per point - what says whether the search is bound by the cells it visits or by the
insertions into its 16-entry list."""
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd.utils import HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh

RUNS = 20
NONE = np.zeros((0, 3), np.int32)
GRIDS = {100489: 317, 1000000: 1000}


def stats(ms):
    t = sorted(ms)
    return f"median {1e3 * t[len(t) // 2]:9.1f} us  min {1e3 * t[0]:9.1f} us"


def cloud(n_points):
    return face_like_mesh(GRIDS[n_points], 16, seed=0).verts


def poses96(r):
    np.random.seed(0)
    return r.generate_3d_transformations()


def render_times(r, mesh, poses, out):
    lib, h = r.ctx.lib, r.ctx.handle
    for _ in range(3):
        r.render_device(mesh, poses, out=out)
    r.check()
    lib.mvlm_render_set_profiling(h, 1)
    splat, tile = [], []
    for _ in range(RUNS):
        r.render_device(mesh, poses, out=out)
        ms2 = (C.c_float * 2)()
        r.ctx.check(lib.mvlm_points_stage_ms(h, ms2))
        splat.append(ms2[0])
        tile.append(ms2[1])
    r.check()
    nv, nve, nt, ms = (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_float * 64)()
    k = lib.mvlm_render_get_profile(h, nv, nve, nt, ms, 64)
    lib.mvlm_render_set_profiling(h, 0)
    return [ms[i] for i in range(k)], splat, tile


def table(n_points):
    verts = cloud(n_points)
    name = f"{n_points:9,d} points".replace(",", " ")
    geo = HipRenderer3D(n_views=96, verbose=False, shading="geometry", point_normals="estimate")
    tex = HipRenderer3D(n_views=96, verbose=False)
    lib, h = geo.ctx.lib, geo.ctx.handle
    poses = poses96(geo)
    out = torch.empty((96, 256, 256, 4), dtype=torch.float32, device="cuda")
    mesh = Mesh(verts, NONE)
    geo.estimate_point_normals(mesh)                       # (warm: scratch, code objects)
    lib.mvlm_render_set_profiling(h, 1)
    stage = []
    for _ in range(RUNS):
        geo.estimate_point_normals(mesh)
        stage.append(geo.normals_stage_ms().copy())
    lib.mvlm_render_set_profiling(h, 0)
    stage = np.array(stage)
    print(f"estimate, {name}:  grid build {stats(stage[:, 0])}   search {stats(stage[:, 1])}   solve {stats(stage[:, 2])}")
    print(f"                              all three  {stats(stage.sum(axis=1))}")
    lib.mvlm_points_set_counting(h, 1)
    geo.estimate_point_normals(mesh)
    s3 = (C.c_uint64 * 3)()
    geo.ctx.check(lib.mvlm_normals_get_stats(h, s3))
    lib.mvlm_points_set_counting(h, 0)
    search_us = 1e3 * float(np.median(stage[:, 1]))
    print(f"    search, per point: {s3[0] / n_points:.2f} shells walked, {s3[1] / n_points:.1f} candidates tested, "
          f"{s3[2] / n_points:.1f} entered the list; {1e3 * search_us / n_points:.2f} ns per point, "
          f"{s3[1] / search_us / 1e3:.1f} G candidates and {s3[2] / search_us / 1e3:.1f} G insertions per second")
    total, splat, tile = render_times(geo, Mesh(verts, NONE, normals=mesh.normals), poses, out)
    print(f"render 96 views, geometry: {stats(total)}   splat {stats(splat)}   tile {stats(tile)}")
    total, splat, tile = render_times(tex, Mesh(verts, NONE), poses, out)
    print(f"render 96 views, texture:  {stats(total)}   splat {stats(splat)}   tile {stats(tile)}   (the yardstick)", flush=True)


def once(n_points):
    r = HipRenderer3D(n_views=96, verbose=False, shading="geometry", point_normals="estimate")
    out = torch.empty((96, 256, 256, 4), dtype=torch.float32, device="cuda")
    r.render_device(Mesh(cloud(n_points), NONE), poses96(r), out=out)   # the upload estimates, then the render
    r.check()


if __name__ == "__main__":
    if "--once" in sys.argv:
        once(int(sys.argv[sys.argv.index("--once") + 1]))
    else:
        for n in GRIDS:
            table(n)
