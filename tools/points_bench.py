#!/usr/bin/env python3
"""Time the point-cloud path beside the triangle path it stands next to: median and minimum of 40 runs, renders by the
library's own events, snaps by events on the stream.

    tools/points_bench.py
    MVLM_HIP_LIB=<a build from before point clouds> tools/points_bench.py     the triangle cases only (the yardsticks)

Cases: 96 views of the bench mesh (face_like_mesh(224, 256, seed=0)) as triangles - the yardstick - and of its vertices as a
cloud; a 1 M-point cloud (the vertices of face_like_mesh(1000)) at 96 views; the snap at 84 and 478 landmarks against the
triangles and against the points.  For the clouds also the split between the splat and the tile kernel
(mvlm_points_stage_ms) and, from one extra render with the counting form of the splat kernel, how many of the covered pixels
still issued their atomic (mvlm_points_get_stats).  Run alternately with an older build to compare (profiles/point_cloud_render_time.txt)."""
import ctypes as C
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd import _lib

older = bool(os.environ.get("MVLM_HIP_LIB"))   # a build without the point-cloud entry points: do not ask it for them
if older:
    for k in ("mvlm_mesh_set_point_radius", "mvlm_mesh_point_radius", "mvlm_points_auto_radius", "mvlm_points_set_counting",
              "mvlm_points_get_stats", "mvlm_points_stage_ms"):
        _lib.SIGNATURES.pop(k)
from mvlm_amd.utils import HipEstimator3D, HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh

TAG = "older" if older else "this "
RUNS = 40


def stats(ms):
    t = sorted(ms)
    return f"median {1e3 * t[len(t) // 2]:8.1f} us  min {1e3 * t[0]:8.1f} us"


def time_render(name, mesh):
    r = HipRenderer3D(n_views=96, verbose=False)
    np.random.seed(0)
    poses = r.generate_3d_transformations()
    out = torch.empty((96, 256, 256, 4), dtype=torch.float32, device="cuda")
    lib, h = r.ctx.lib, r.ctx.handle
    for _ in range(3):
        r.render_device(mesh, poses, out=out)
    r.check()
    lib.mvlm_render_set_profiling(h, 1)
    total, splat, tile = [], [], []
    for _ in range(RUNS):
        r.render_device(mesh, poses, out=out)
        if mesh.n_tris == 0:
            ms2 = (C.c_float * 2)()
            r.ctx.check(lib.mvlm_points_stage_ms(h, ms2))
            splat.append(ms2[0])
            tile.append(ms2[1])
    r.check()
    nv, nve, nt, ms = (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_float * 64)()
    k = lib.mvlm_render_get_profile(h, nv, nve, nt, ms, 64)
    lib.mvlm_render_set_profiling(h, 0)
    total = [ms[i] for i in range(k)]
    line = f"{TAG} render 96 views, {name:34s} {stats(total)}"
    if splat:
        lib.mvlm_points_set_counting(h, 1)
        r.render_device(mesh, poses, out=out)
        covered, issued = C.c_uint64(), C.c_uint64()
        r.ctx.check(lib.mvlm_points_get_stats(h, C.byref(covered), C.byref(issued)))
        lib.mvlm_points_set_counting(h, 0)
        rad = C.c_double()
        from mvlm_amd.utils.render3d import upload_mesh

        lib.mvlm_mesh_point_radius(upload_mesh(r.ctx, mesh), C.byref(rad))
        line += (f"\n{TAG}     splat {stats(splat)}   tile {stats(tile)}   radius {rad.value * 256 / 300:.3f} px"
                 f"\n{TAG}     covered pixels {covered.value}, atomics issued {issued.value} "
                 f"({100.0 * (1 - issued.value / max(covered.value, 1)):.1f} % skipped after reading the key)")
    print(line, flush=True)


def time_snap(name, mesh, n_queries):
    e3 = HipEstimator3D(verbose=False)
    rs = np.random.RandomState(1)
    pts = torch.from_numpy(rs.uniform(-100, 100, size=(n_queries, 3))).cuda()
    out = torch.empty_like(pts)
    for _ in range(3):
        e3.project_device(mesh, pts, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e3.project_device(mesh, pts, out=out)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    print(f"{TAG} snap {n_queries:3d} landmarks, {name:31s} {stats(ms)}", flush=True)


base = face_like_mesh(224, 256, seed=0)
triangles = Mesh(base.verts, base.tris, base.uvs, base.texture)
time_render("bench mesh, 99 458 triangles", triangles)
for n in (84, 478):
    time_snap("bench mesh, 99 458 triangles", triangles, n)
if not older:
    none = np.zeros((0, 3), np.int32)
    cloud = Mesh(base.verts, none)
    time_render("its 50 176 vertices as a cloud", cloud)
    big = Mesh(face_like_mesh(1000, 16, seed=0).verts, none)
    time_render("a cloud of 1 000 000 points", big)
    for n in (84, 478):
        time_snap("50 176 points", cloud, n)
        time_snap("1 000 000 points", big, n)
