#!/usr/bin/env python3
"""Time a point cloud's triangulation (mvlm_mesh_triangulate_points) and say what surface it gives.

    tools/cloud_mesh_bench.py [--out FILE]      the table (profiles/cloud_mesh_time.txt; FILE receives what is printed)
    tools/cloud_mesh_bench.py --once N          one estimate and one triangulation of the N-point cloud, nothing else: the program
                                                to put behind `rocprofv3 --kernel-trace --stats --` for the kernels' times

Clouds: the bench mesh's vertices, face_like_mesh(224) (50 176 points), and face_like_mesh(1000) (1 000 000 points), faces dropped.
Per cloud: the three stage times (star with the shift, count + scan, emit: mvlm_cloud_mesh_stage_ms), median and minimum of RUNS
runs by the library's own events, next to the yardstick - the normal estimate's three stages (grid build, search, solve:
mvlm_normals_stage_ms) of the same cloud in the same session, which the triangulation should not exceed; the triangle count; the
share of the original mesh's area.  For the bench mesh also the share of the 96 bench views' pixels whose depth byte differs between
the triangulated cloud and the original mesh."""
import ctypes as C
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd.utils import HipRenderer3D, Mesh
from mvlm_amd.utils.render3d import upload_mesh
from mvlm_amd.utils.synthetic import face_like_mesh

RUNS = 20
NONE = np.zeros((0, 3), np.int32)
GRIDS = {50176: 224, 1000000: 1000}
LINES: list = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def stats(ms):
    t = sorted(ms)
    return f"median {1e3 * t[len(t) // 2]:9.1f} us  min {1e3 * t[0]:9.1f} us"


def area(verts, tris) -> float:
    v = verts.astype(np.float64)
    return float(0.5 * np.linalg.norm(np.cross(v[tris[:, 1]] - v[tris[:, 0]], v[tris[:, 2]] - v[tris[:, 0]]), axis=1).sum())


def triangulate_raw(r, handle, table, tris, count):
    r.ctx.check(r.ctx.lib.mvlm_mesh_triangulate_points(r.ctx.handle, handle, C.c_void_p(table.data_ptr()), C.c_void_p(tris.data_ptr()),
                                                       C.c_longlong(tris.shape[0]), C.c_void_p(count.data_ptr())))


def table(n_points):
    face = face_like_mesh(GRIDS[n_points], 16, seed=0)
    name = f"{n_points:9,d} points".replace(",", " ")
    r = HipRenderer3D(n_views=96, verbose=False)
    lib, h = r.ctx.lib, r.ctx.handle
    dev = torch.device("cuda", r.ctx.device)
    cloud = Mesh(face.verts, NONE)
    handle = upload_mesh(r.ctx, cloud)
    r.ctx.bind_current_stream(torch, dev)
    nbr = torch.empty((n_points, 16), dtype=torch.int32, device=dev)
    tris = torch.empty((3 * n_points + 1024, 3), dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)

    def estimate():
        r.ctx.check(lib.mvlm_mesh_estimate_normals(h, handle, C.c_void_p(nbr.data_ptr())))

    estimate()                                              # (warm: scratch, code objects)
    triangulate_raw(r, handle, nbr, tris, count)
    torch.cuda.synchronize()
    lib.mvlm_render_set_profiling(h, 1)
    normals_ms, mesh_ms = [], []
    for _ in range(RUNS):
        estimate()
        normals_ms.append(r.normals_stage_ms().copy())
        triangulate_raw(r, handle, nbr, tris, count)
        mesh_ms.append(r.cloud_mesh_stage_ms().copy())
    lib.mvlm_render_set_profiling(h, 0)
    normals_ms, mesh_ms = np.array(normals_ms), np.array(mesh_ms)
    say(f"triangulate, {name}:  star {stats(mesh_ms[:, 0])}   count + scan {stats(mesh_ms[:, 1])}   emit {stats(mesh_ms[:, 2])}")
    say(f"                                 all three  {stats(mesh_ms.sum(axis=1))}")
    say(f"estimate,    {name}:  grid build {stats(normals_ms[:, 0])}   search {stats(normals_ms[:, 1])}   solve {stats(normals_ms[:, 2])}")
    say(f"                                 all three  {stats(normals_ms.sum(axis=1))}   (the yardstick)")
    ratio = float(np.median(mesh_ms.sum(axis=1)) / np.median(normals_ms.sum(axis=1)))
    say(f"    triangulation / estimate = {ratio:.2f};  {1e6 * float(np.median(mesh_ms.sum(axis=1))) / n_points:.2f} ns per point")
    n = int(count.item())
    got = tris[:n].cpu().numpy()
    uses = np.unique(np.sort(np.concatenate([got[:, [0, 1]], got[:, [1, 2]], got[:, [0, 2]]]), axis=1), axis=0, return_counts=True)[1]
    say(f"    {n} triangles (the mesh has {face.n_tris}), {100.0 * area(face.verts, got) / area(face.verts, face.tris):.3f} % of the mesh's "
        f"area, {int((uses == 1).sum())} boundary edges (the mesh has {4 * (GRIDS[n_points] - 1)}), {int((uses > 2).sum())} edges in more than two triangles")
    if n_points == 50176:
        np.random.seed(0)
        poses = r.generate_3d_transformations()
        out = torch.empty((96, 256, 256, 4), dtype=torch.float32, device=dev)
        depth = []
        for mesh in (Mesh(face.verts, face.tris), r.triangulate_point_cloud(Mesh(face.verts, NONE))):
            depth.append(torch.round(r.render_device(mesh, poses, out=out)[..., 3] * 255.0).to(torch.int32).cpu().numpy())
        r.check()
        differ = depth[0] != depth[1]
        covered = depth[0] != depth[0].max()
        say(f"    96 bench views: the depth byte differs in {int(differ.sum())} of {differ.size} pixels ({100.0 * differ.mean():.4f} %; "
            f"{100.0 * differ.sum() / max(int(covered.sum()), 1):.4f} % of the {int(covered.sum())} the mesh covers)")


def once(n_points):
    r = HipRenderer3D(n_views=1, verbose=False)
    r.triangulate_point_cloud(Mesh(face_like_mesh(GRIDS[n_points], 16, seed=0).verts, NONE))
    torch.cuda.synchronize()


if __name__ == "__main__":
    if "--once" in sys.argv:
        once(int(sys.argv[sys.argv.index("--once") + 1]))
    else:
        say("---- tools/cloud_mesh_bench.py ----")
        for points in GRIDS:
            table(points)
        if "--out" in sys.argv:
            target = Path(sys.argv[sys.argv.index("--out") + 1])
            target.parent.mkdir(parents=True, exist_ok=True)
            target.write_text("\n".join(LINES) + "\n")
