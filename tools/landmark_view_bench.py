#!/usr/bin/env python3
"""Time the landmark view (mvlm_render_landmark_view) on the bench mesh, face_like_mesh(224, 256, seed=0), textured, one front
view at frame="fit": sizes 256 / 1024 / 2048 with 0 / 84 / 478 landmarks on the surface - median of 40 calls by the library's own
events, per stage (the copies and fills in front of the kernels - the key plane is filled in every call -, transform, classify,
scan, bin fill, landmark projection, tile), with the nanoseconds per pixel.

    tools/landmark_view_bench.py                       the table above, then the yardstick below on this build
    MVLM_HIP_LIB=<parent's build> tools/landmark_view_bench.py     the yardstick alone: mvlm_render of ONE view and of 96 views
                                                       of that mesh (a build from before the entry has nothing else to time)
    tools/landmark_view_bench.py --step [steps]        what Pipeline(visualize_img=True) costs a whole configs[2] step (96
                                                       views, 84 landmarks, one 1024^2 view), off and on alternating, the PNG
                                                       encode included and stated separately
It prints; profiles/landmark_view_time.txt is that output."""
import ctypes as C
import os
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from mvlm_amd import _lib

older = bool(os.environ.get("MVLM_HIP_LIB"))   # a build without the landmark view: do not ask it for the entry points
if older:
    for k in ("mvlm_render_landmark_view", "mvlm_landmark_view_stage_ms"):
        _lib.SIGNATURES.pop(k)
from mvlm_amd.utils import HipRenderer3D, Mesh
from mvlm_amd.utils.synthetic import face_like_mesh

STAGES = ("fill", "transform", "classify", "scan", "bin_fill", "project", "tile")  # fill: the copies and memsets, the key plane's among them
TAG = "parent" if older else "this  "


def yardstick():
    base = face_like_mesh(224, 256, seed=0)
    mesh = Mesh(base.verts, base.tris, base.uvs, base.texture)
    for n in (1, 96):
        r = HipRenderer3D(n_views=n, verbose=False)
        np.random.seed(0)
        poses = np.zeros((1, 6), np.float32) if n == 1 else r.generate_3d_transformations()
        out = torch.empty((n, 256, 256, 4), dtype=torch.float32, device="cuda")
        for _ in range(3):
            r.render_device(mesh, poses, out=out)
        r.check()
        lib, h = r.ctx.lib, r.ctx.handle
        lib.mvlm_render_set_profiling(h, 1)
        for _ in range(40):
            r.render_device(mesh, poses, out=out)
        r.check()
        nv, nve, nt, ms = (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_int32 * 64)(), (C.c_float * 64)()
        k = lib.mvlm_render_get_profile(h, nv, nve, nt, ms, 64)
        lib.mvlm_render_set_profiling(h, 0)
        t = sorted(ms[i] for i in range(k))
        med = 1e3 * t[k // 2]
        print(f"{TAG} mvlm_render {n:2d} view(s) of 256^2: median {med:8.1f} us  min {1e3 * t[0]:8.1f} us  "
              f"{1e3 * med / (n * 65536):7.3f} ns per pixel", flush=True)


def views():
    base = face_like_mesh(224, 256, seed=0)
    mesh = Mesh(base.verts, base.tris, base.uvs, base.texture)
    r = HipRenderer3D(n_views=1, verbose=False)
    lib, h = r.ctx.lib, r.ctx.handle
    rs = np.random.RandomState(0)
    for size in (256, 1024, 2048):
        for nl in (0, 84, 478):
            lm = np.asarray(base.verts, np.float64)[rs.permutation(len(base.verts))[:nl]]
            for _ in range(3):
                r.render_landmark_view_device(mesh, lm, size=size, return_pixels=True)
            r.check()
            lib.mvlm_render_set_profiling(h, 1)
            rows = []
            for _ in range(40):
                r.render_landmark_view_device(mesh, lm, size=size, return_pixels=True)
                ms = (C.c_float * 7)()
                r.ctx.check(lib.mvlm_landmark_view_stage_ms(h, ms))
                rows.append([1e3 * ms[i] for i in range(7)])
            lib.mvlm_render_set_profiling(h, 0)
            r.check()
            rows = np.array(rows)
            total = np.median(rows.sum(axis=1))
            med = np.median(rows, axis=0)
            shares = "  ".join(f"{s} {m:7.1f} us ({100 * m / med.sum():4.1f} %)" for s, m in zip(STAGES, med))
            print(f"{TAG} view {size:4d}^2, {nl:3d} landmarks: median {total:8.1f} us  min {rows.sum(axis=1).min():8.1f} us  "
                  f"{1e3 * total / (size * size):7.3f} ns per pixel | {shares}", flush=True)


def step(steps):
    from mvlm_amd import config
    from mvlm_amd.utils.viewer import write_view_png

    mesh = face_like_mesh(224, 2048, seed=0)
    pipe = config.load_config(config.default_config("BU_3DFE", "RGB+depth", n_views=96)).build_pipeline(weights="synthetic:0", verbose=False)
    pipe.visualize_size = 1024
    np.random.seed(0)
    poses = pipe.renderer_3d.generate_3d_transformations()
    ms = {False: [], True: []}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for rnd in range(3):
                for on in (False, True):
                    pipe.visualize_img = on
                    for _ in range(3):
                        np.random.seed(1)
                        pipe.predict_mesh_device(mesh, poses)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(steps):
                        np.random.seed(1)
                        landmarks, _ = pipe.predict_mesh_device(mesh, poses)
                    torch.cuda.synchronize()
                    ms[on].append(1e3 * (time.perf_counter() - t) / steps)
            image = pipe.renderer_3d.render_landmark_view(mesh, landmarks, size=1024)[0]
            enc = []
            for _ in range(5):
                t = time.perf_counter()
                write_view_png(image, Path("visualization") / "encode_only.png")
                enc.append(1e3 * (time.perf_counter() - t))
        finally:
            os.chdir(cwd)
    off, on = np.median(ms[False]), np.median(ms[True])
    for flag, r in ms.items():
        print(f"configs[2] step (96 views, 84 landmarks), visualize_img={flag}: {np.median(r):.3f} ms per step "
              f"(rounds {', '.join(f'{v:.3f}' for v in r)})")
    print(f"configs[2] step: one 1024^2 landmark view adds {on - off:+.3f} ms per step ({100 * (on - off) / off:+.1f} %), of which the PNG "
          f"encode and write (Pillow, host) is {np.median(enc):.3f} ms")


if __name__ == "__main__":
    if "--step" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--step"]
        step(int(rest[0]) if rest else 10)
    else:
        if not older:
            views()
        yardstick()
